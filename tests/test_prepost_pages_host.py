"""The host half of "boxes on several pages in one batch" (prepost.plan_pages / *_pages, pipeline.edit_pages / edit_pages_verified): the
crop plan against per-page plan_edits on one stream, the page table (dmx_edit_page) and the item table through the C-ABI's host-only
entry dmx_edit_pages_prepare, the refusals of the four launch entries - by page index or by item index, before any launch, with dummy
addresses - and the argument checks of the Python functions, which run before anything touches the GPU.  Nothing here needs a GPU."""
import ctypes

import numpy as np
import pytest
import torch

# pages (h, w) and their boxes: the second page's short side caps the crop below the box width, so its origins are DRAWN
SIZES = [(1100, 1300), (300, 1400), (97, 131)]
BOXES = [[(100, 100, 180, 110), (40, 40, 400, 60), (1200, 1050, 1299, 1099)],
         [(100, 100, 1000, 110), (20, 30, 80, 44), (300, 200, 1350, 240), (100, 100, 1000, 110)],
         [(5, 5, 120, 20)]]
S = 64
# h x w of tests/test_prepost_pages_gpu.py's pages
PAGES = [(150, 300), (97, 131), (260, 90), (70, 260)]
ONE = ctypes.c_void_p(64)            # a dummy device address: the refusals return before any launch


def test_plan_pages_is_plan_edits_page_after_page_on_one_stream():
    from diffute_amd import prepost
    mine, rng = np.random.RandomState(7), np.random.RandomState(7)
    got = prepost.plan_pages(BOXES, SIZES, mine)
    want = [prepost.plan_edits(boxes, h, w, rng) for boxes, (h, w) in zip(BOXES, SIZES)]
    assert got == want and [len(p) for p in got] == [3, 4, 1]
    assert mine.randint(1 << 30) == rng.randint(1 << 30), "plan_pages drew more or fewer numbers than the per-page calls"
    assert got[1][0] != got[1][3], "equal boxes of one page: each must get a draw of its own (true for this seed)"
    with pytest.raises(ValueError):
        prepost.plan_pages(BOXES, SIZES[:2], mine)


def _tables(pages, items):
    """pages: [(h, w, item_lo, item_hi)], items: [(box, (x_s, y_s), crop)] -> (dmx_edit_page table with dummy addresses, dmx_edit_item table)"""
    from diffute_amd import _cabi
    pt = (_cabi.EditPage * max(len(pages), 1))()
    for pg, (h, w, lo, hi) in zip(pt, pages):
        pg.original, pg.out, pg.union_mask = 64, 128, 0
        pg.H, pg.W, pg.item_lo, pg.item_hi = h, w, lo, hi
    arr = (_cabi.EditItem * max(len(items), 1))()
    for it, (box, (x_s, y_s), crop) in zip(arr, items):
        it.x1, it.y1, it.x2, it.y2 = box
        it.x_s, it.y_s, it.crop_scale = x_s, y_s, crop
    return pt, arr


GOOD = ((10, 10, 40, 20), (0, 0), 64)
# six items on the four pages: 2 + 1 + 2 + 1
RANGES = [(0, 2), (2, 3), (3, 5), (5, 6)]
ITEMS = [((10, 10, 90, 30), (4, 2), 128), ((200, 100, 290, 120), (180, 60), 128),      # the second crop is clipped by the 150 x 300 page
         ((10, 10, 60, 30), (0, 0), 64),
         ((5, 160, 80, 200), (0, 150), 90), ((5, 10, 80, 40), (10, 0), 32),            # origin y = 150: outside both neighbouring pages
         ((100, 10, 240, 40), (100, 0), 128)]


def _good():
    return _tables([(h, w, lo, hi) for (h, w), (lo, hi) in zip(PAGES, RANGES)], ITEMS)


def test_page_table_layout_and_derived_fields():
    """dmx_edit_page as ctypes sees it is what the header declares (three addresses, six ints); the prepare entry fills every item's derived
    fields as dmx_edit_items_prepare does with that item's OWN page size, the page index in `reserved`, and the pages' block ranges"""
    from diffute_amd import _cabi
    assert ctypes.sizeof(_cabi.EditPage) == 3 * 8 + 6 * 4 and _cabi.EditPage.H.offset == 24
    assert ctypes.sizeof(_cabi.EditItem) == 12 * 4 + 4 * 8
    for elem in ("bf16", "fp16"):
        lib = _cabi.lib(elem)
        pt, arr = _good()
        _cabi.check(lib.dmx_edit_pages_prepare(pt, 4, arr, 6, S), "pages prepare", lib)
        derived = lambda it: (it.cw, it.ch, it.pre_area2, it.post_area2, it.pre_sx, it.pre_sy, it.post_sx, it.post_sy)
        for q, ((h, w), (lo, hi)) in enumerate(zip(PAGES, RANGES)):
            _, one = _tables([], ITEMS[lo:hi])
            _cabi.check(lib.dmx_edit_items_prepare(one, hi - lo, h, w, S), "items prepare", lib)
            for j in range(hi - lo):
                assert derived(arr[lo + j]) == derived(one[j]), f"item {lo + j} (page {q})"
                assert arr[lo + j].reserved == q and one[j].reserved == 0
        assert (arr[1].cw, arr[1].ch) == (120, 90) and (arr[3].cw, arr[3].ch) == (90, 90) and arr[4].post_area2 == 1
        assert (arr[3].x1, arr[3].y2, arr[3].y_s, arr[3].crop_scale) == (5, 200, 150, 90)          # the caller's fields are untouched
        # blocks of 256 pixels, one row at a time: 150 * 2, 97 * 1, 260 * 1, 70 * 2
        assert [(pg.block_lo, pg.blocks) for pg in pt] == [(0, 300), (300, 97), (397, 260), (657, 140)]
        assert [(pg.original, pg.out, pg.H, pg.W) for pg in pt] == [(64, 128, h, w) for h, w in PAGES]


def _refused(lib, pt, P, arr, B, *words):
    assert lib.dmx_edit_pages_prepare(pt, P, arr, B, S) != 0
    msg = lib.dmx_last_error().decode()
    assert all(w in msg for w in words), msg


def test_bad_pages_and_items_are_reported_by_index():
    from diffute_amd import _cabi
    lib = _cabi.lib()
    pages = lambda ranges, sizes=PAGES: [(h, w, lo, hi) for (h, w), (lo, hi) in zip(sizes, ranges)]
    # an origin outside its own page (97 x 131) but inside the larger neighbour before it (150 x 300)
    items = list(ITEMS); items[2] = ((10, 10, 60, 30), (140, 0), 64)
    pt, arr = _tables(pages(RANGES), items)
    _refused(lib, pt, 4, arr, 6, "item 2", "origin")
    items[2] = ((10, 10, 60, 30), (0, 100), 64)                      # ... and below its own 97 rows
    pt, arr = _tables(pages(RANGES), items)
    _refused(lib, pt, 4, arr, 6, "item 2", "origin")
    items = list(ITEMS); items[5] = ((100, 10, 240, 40), (100, 0), 0)
    pt, arr = _tables(pages(RANGES), items)
    _refused(lib, pt, 4, arr, 6, "item 5", "crop_scale")
    # item ranges that overlap, leave a gap, are out of order, end early or late; a page without items
    for ranges, q in (([(0, 2), (1, 3), (3, 5), (5, 6)], 1), ([(0, 2), (3, 4), (4, 5), (5, 6)], 1), ([(2, 3), (0, 2), (3, 5), (5, 6)], 0),
                      ([(0, 2), (2, 3), (3, 5), (5, 7)], 3), ([(0, 2), (2, 3), (3, 4), (4, 5)], 3), ([(0, 2), (2, 2), (2, 5), (5, 6)], 1),
                      ([(0, 2), (2, 3), (5, 3), (5, 6)], 2)):
        pt, arr = _tables(pages(ranges), ITEMS)
        _refused(lib, pt, 4, arr, 6, f"page {q}")
    # bad page sizes, by page index; H <= 65535 holds per page
    for bad, q in (((0, 131), 1), ((97, 0), 1), ((65536, 90), 2), ((97, (1 << 31) - 255), 1), ((1, (1 << 31) - 1), 3)):     # W + 255 stays an int
        sizes = list(PAGES); sizes[q] = bad
        pt, arr = _tables(pages(RANGES, sizes), ITEMS)
        _refused(lib, pt, 4, arr, 6, f"page {q}")
    # P = 0, P > 64, B > 64, B = 0
    pt, arr = _tables([(150, 300, i, i + 1) for i in range(65)], [GOOD] * 65)
    _refused(lib, pt, 0, arr, 6, "pages")
    _refused(lib, pt, 65, arr, 65, "pages")
    pt1, _ = _tables([(150, 300, 0, 65)], [])
    _refused(lib, pt1, 1, arr, 65, "items")
    _refused(lib, pt1, 1, arr, 0, "items")
    # the caps themselves pass: 64 pages of one item each, and 64 rows of 65535 pixels per page summed far past 65535 rows
    _cabi.check(lib.dmx_edit_pages_prepare(pt, 64, arr, 64, S), "64 pages")
    tall, arr = _tables([(65535, 90, i, i + 1) for i in range(64)], [GOOD] * 64)
    _cabi.check(lib.dmx_edit_pages_prepare(tall, 64, arr, 64, S), "64 tall pages")
    assert tall[63].block_lo == 63 * 65535


def test_launch_entries_refuse_a_table_spoiled_after_the_prepare():
    """the four entries check the HOST tables page by page and item by item and return before they launch: callable without a GPU.  Every
    call below is one that must be refused - the addresses are dummies."""
    from diffute_amd import _cabi
    lib = _cabi.lib()
    pa = (_cabi.ReadbackPass * 6)()
    for ps in pa:                                         # plausible pass tables (no box is 32 wide or high): the boxes are what is refused
        ps.h_off, ps.h_taps, ps.v_off, ps.v_taps = 0, 1, 0, 1

    def entries(pt, arr, P=4, B=6):
        return (lib.dmx_preprocess_crop_pages(pt, ONE, P, arr, ONE, B, S, ONE, ONE, ONE, ONE, None),
                lib.dmx_postprocess_paste_pages(ONE, S, pt, ONE, P, arr, ONE, B, None),
                lib.dmx_readback_pixel_values_pages(ONE, S, pt, ONE, P, arr, ONE, B, 2, ONE, 1 << 20, ONE, pa, ONE, 8, 32, 32, ONE, None, None),
                lib.dmx_postprocess_paste_select_pages(ONE, S, ONE, float("-inf"), ONE, pt, ONE, P, arr, ONE, B, 2, None))

    def spoiled(change, *words):
        pt, arr = _good()
        _cabi.check(lib.dmx_edit_pages_prepare(pt, 4, arr, 6, S), "prepare")
        change(pt, arr)
        for call in range(4):                             # one at a time: each call leaves its own message
            assert entries(pt, arr)[call] != 0, (call, words)
            msg = lib.dmx_last_error().decode()
            assert all(w in msg for w in words), (call, msg)

    def item(b, **kw):
        def f(pt, arr):
            for k, v in kw.items():
                setattr(arr[b], k, v)
        return f

    def page(q, **kw):
        def f(pt, arr):
            for k, v in kw.items():
                setattr(pt[q], k, v)
        return f
    spoiled(item(2, x_s=131), "item 2", "origin")          # inside page 0's width, outside its own
    spoiled(item(3, y_s=260), "item 3", "origin")
    spoiled(item(4, cw=33), "item 4", "derived")
    spoiled(item(5, reserved=2), "item 5", "page")
    spoiled(page(1, W=300), "page 1", "derived")          # another width: the block counts no longer belong to the table
    spoiled(page(2, H=70), "page 2")
    spoiled(page(2, item_hi=4), "page 3")                 # page 3's items no longer follow page 2's
    spoiled(page(3, block_lo=656), "page 3", "derived")
    spoiled(page(0, original=0), "page 0", "null")
    # what only some entries ask: an output of its own for the pastes, a box inside ITS page for the read-back
    pt, arr = _good()
    _cabi.check(lib.dmx_edit_pages_prepare(pt, 4, arr, 6, S), "prepare")
    pt[1].out = 0
    assert lib.dmx_postprocess_paste_pages(ONE, S, pt, ONE, 4, arr, ONE, 6, None) != 0 and "page 1" in lib.dmx_last_error().decode()
    assert lib.dmx_postprocess_paste_select_pages(ONE, S, ONE, 0.0, ONE, pt, ONE, 4, arr, ONE, 6, 2, None) != 0 and "page 1" in lib.dmx_last_error().decode()
    pt[1].out = pt[1].original
    assert lib.dmx_postprocess_paste_pages(ONE, S, pt, ONE, 4, arr, ONE, 6, None) != 0 and "page 1" in lib.dmx_last_error().decode()
    pt[1].out = 128
    arr[2].x2 = 140                                        # inside page 0 (300 wide), outside page 1 (131 wide)
    assert lib.dmx_readback_pixel_values_pages(ONE, S, pt, ONE, 4, arr, ONE, 6, 2, ONE, 1 << 20, ONE, pa, ONE, 8, 32, 32, ONE, None, None) != 0
    assert "item 2" in lib.dmx_last_error().decode() and "outside" in lib.dmx_last_error().decode()
    arr[2].x2 = 60
    assert lib.dmx_preprocess_crop_pages(pt, ONE, 4, arr, ONE, 6, 100, ONE, ONE, ONE, ONE, None) != 0, "S must be a multiple of 8"
    assert lib.dmx_postprocess_paste_select_pages(ONE, S, ONE, float("nan"), ONE, pt, ONE, 4, arr, ONE, 6, 2, None) != 0
    assert lib.dmx_postprocess_paste_select_pages(ONE, S, ONE, 0.0, ONE, pt, ONE, 4, arr, ONE, 6, 17, None) != 0
    assert lib.dmx_preprocess_crop_pages(pt, ONE, 3, arr, ONE, 6, S, ONE, ONE, ONE, ONE, None) != 0, "three pages cover five of the six items"


def test_paged_functions_check_their_lists_first_and_refuse_host_tensors():
    from diffute_amd import prepost, processing
    img = torch.zeros(64, 80, 3, dtype=torch.uint8)
    ip = processing.ViTImageProcessor(size=32)
    box, org = [(4, 4, 30, 12)], [(0, 0)]
    calls = {
        "pre": lambda *a: prepost.preprocess_pages(*a),
        "post": lambda imgs, *a: prepost.postprocess_pages(torch.zeros(1, 3, 16, 16), imgs, *a),
        "readback": lambda imgs, *a: prepost.readback_pixel_values_pages(torch.zeros(1, 2, 3, 16, 16), imgs, *a, ip),
        "select": lambda imgs, *a: prepost.postprocess_select_pages(torch.zeros(1, 2, 3, 16, 16), torch.zeros(1, 2), imgs, *a),
    }
    for name, fn in calls.items():
        with pytest.raises(ValueError):
            fn([], [], [], [])                                              # P = 0
        with pytest.raises(ValueError):
            fn([img] * 65, [box] * 65, [org] * 65, [[32]] * 65)             # P > 64
        with pytest.raises(ValueError):
            fn([img] * 2, [box * 33] * 2, [org * 33] * 2, [[32] * 33] * 2)  # N = 66 > 64
        with pytest.raises(ValueError):
            fn([img] * 2, [box], [org] * 2, [[32]] * 2)                     # mismatched page lists
        with pytest.raises(ValueError):
            fn([img] * 2, [box] * 2, [org] * 2, [[32]])
        with pytest.raises(ValueError, match="page 1"):
            fn([img] * 2, [box, box * 2], [org, org], [[32], [32] * 2])     # mismatched lists inside a page
        with pytest.raises(ValueError, match="page 1"):
            fn([img] * 2, [box, []], [org, []], [[32], []])                 # a page without boxes
        with pytest.raises(TypeError):
            fn([img], [box], [org], [[32]])                                 # host tensors: no CPU fallback
        with pytest.raises(TypeError):
            fn([img] * 64, [box] * 64, [org] * 64, [[32]] * 64)             # 64 pages pass the list checks
    with pytest.raises(ValueError, match="page 1"):                         # the read-back's box checks run per page, with that page's size
        prepost.check_readback_boxes_pages([(4, 4, 30, 12), (4, 4, 81, 12)], [1, 1], [(64, 100), (64, 80)])
    prepost.check_readback_boxes_pages([(4, 4, 100, 12), (4, 4, 80, 12)], [1, 1], [(64, 100), (64, 80)])


def test_edit_pages_raises_its_argument_errors_without_a_gpu():
    """the models are never reached: None stands in for them"""
    import diffute_amd as D
    imgs = [torch.zeros(64, 80, 3, dtype=torch.uint8), torch.zeros(50, 90, 3, dtype=torch.uint8)]
    boxes = [[(4, 4, 30, 12), (40, 20, 70, 30)], [(4, 4, 30, 12)]]
    ctx = torch.zeros(3, 77, 128)

    def run(exc, images=imgs, locations=boxes, ctx=ctx, **kw):
        with pytest.raises(exc):
            D.edit_pages(None, None, None, images, locations, ctx, 3, size=64, **kw)
    run(ValueError, batch_size=0)
    run(ValueError, locations=boxes[:1])
    run(ValueError, images=imgs[:1])
    run(ValueError, ctx=ctx[:2])                                            # 3 boxes, 2 contexts
    run(ValueError, origins=[[(0, 0)] * 2])
    run(ValueError, origins=[[(0, 0)], [(0, 0)]])                           # page 0 has two boxes
    run(ValueError, crop_scales=[[32, 32], [32, 32]])
    run(TypeError, images=[imgs[0], torch.zeros(50, 90, dtype=torch.uint8)])
    run(ValueError, locations=[boxes[0], []], ctx=ctx[:2])                  # a page without boxes
    run(TypeError)                                                          # every list is fine: the first thing that touches a tensor refuses the host pages


def test_a_refused_verified_call_draws_nothing_from_rng():
    """every argument check of edit_boxes_verified / edit_pages_verified runs before a crop is planned: after the ValueError the caller's
    rng stands where it stood, so the next - corrected - call plans the crops the first one would have.  Origins and crop scales are
    left out, and planning these pages does draw (the second page's origins)."""
    from types import SimpleNamespace
    import diffute_amd as D
    from diffute_amd import prepost
    ocr = SimpleNamespace(encoder=SimpleNamespace(config=SimpleNamespace(image_size=32)),
                          decoder=SimpleNamespace(config=SimpleNamespace(vocab_size=300, max_position_embeddings=64)))
    imgs = [torch.zeros(h, w, 3, dtype=torch.uint8) for h, w in SIZES]
    N = sum(len(b) for b in BOXES)
    ctx, labels, proc = torch.zeros(N, 77, 128), torch.full((N, 5), 7, dtype=torch.int64), D.TrOCRProcessor(size=32)
    empty = [list(b) for b in BOXES]
    empty[0][1] = (40, 40, 40, 60)
    drawn, twin = np.random.RandomState(11), np.random.RandomState(11)
    prepost.plan_pages(BOXES, SIZES, drawn)
    assert drawn.randint(1 << 30) != twin.randint(1 << 30), "planning these pages draws nothing: the checks below would show nothing"
    for n, images, boxes, call in ((N, imgs, BOXES, D.edit_pages_verified), (len(BOXES[0]), imgs[0], BOXES[0], D.edit_boxes_verified)):
        one_page = call is D.edit_boxes_verified
        for bad in (dict(labels=labels[:n - 1]),                                       # one row of labels too few
                    dict(locations=empty[0] if one_page else empty),                   # an empty box: nothing to read back
                    dict(processor=D.TrOCRProcessor(size=384))):                       # the encoder reads 32 x 32
            a = dict(processor=proc, locations=boxes, labels=labels[:n])
            a.update(bad)
            mine, twin = np.random.RandomState(7), np.random.RandomState(7)
            with pytest.raises(ValueError):
                call(None, None, None, ocr, a["processor"], images, a["locations"], ctx[:n], a["labels"], 3, size=S, rng=mine)
            assert mine.randint(1 << 30) == twin.randint(1 << 30), f"{call.__name__} refused {sorted(bad)} after drawing from rng"


def test_public_names():
    import diffute_amd as D
    from diffute_amd import _cabi, edit_pages, edit_pages_verified, prepost
    assert "edit_pages" in D.__all__ and "edit_pages_verified" in D.__all__ and callable(edit_pages) and callable(edit_pages_verified)
    for name in ("plan_pages", "preprocess_pages", "postprocess_pages", "readback_pixel_values_pages", "postprocess_select_pages"):
        assert callable(getattr(prepost, name)) and callable(getattr(D.prepost, name))
    for name in ("dmx_edit_pages_prepare", "dmx_preprocess_crop_pages", "dmx_postprocess_paste_pages", "dmx_readback_pixel_values_pages",
                 "dmx_postprocess_paste_select_pages"):
        assert name in _cabi.exported_symbols()
