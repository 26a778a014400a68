"""Boxes on SEVERAL pages per launch (the *_pages kernels of csrc/prepost_batch.hip and csrc/readback.hip through prepost.preprocess_pages
/ postprocess_pages / readback_pixel_values_pages / postprocess_select_pages) against the numpy restatements (oracle/prepost.py,
tests/readback_restatement.py) and the single-box kernels, each applied to an item's OWN page - bit-exact, on both builds.  Four small
pages of odd, non-monotone sizes at S = 64: two are wider than the paste's 256-column tile (a partial last tile), one is taller than its
neighbours have rows, so a row computed with a neighbour's H, W or pointer shows in the bytes.  The paste writes into views of one
sentinel-filled slab with guard bands between and around the pages."""
import numpy as np
import pytest
import torch

import readback_restatement as RB

pytestmark = pytest.mark.gpu

S, K, SIZE = 64, 2, 32
PAGES = [(150, 300), (97, 131), (260, 90), (70, 260)]            # h x w
# per page: name, box (x1, y1, x2, y2), crop origin, crop_scale.  Eleven items, page-major; every path of tests/test_prepost_batch_gpu.py's lists
ITEMS = [
    [("up_40_first", (20, 20, 50, 32), (15, 10), 40),               # crop < S: enlarged; the first item of the table
     ("area_128", (120, 40, 200, 70), (100, 10), 128),              # crop = 2S: the exact-2x path of the preprocess
     ("down_100_overlap", (150, 50, 230, 80), (140, 30), 100),      # overlaps area_128's box: the later one wins
     ("clipped_corner", (260, 100, 298, 120), (250, 90), 64),       # the crop is cut to 50 x 60 by the page; lies in the partial column tile
     ("same_box", (10, 30, 60, 50), (5, 2), 64)],                   # crop = S: identity; the same box and origin as on the last page
    [("corner_odd_77", (0, 0, 60, 20), (0, 0), 77)],                # a box at (0, 0), an odd crop; the only item of its page
    [("half_32_deep", (10, 200, 40, 220), (8, 195), 32),            # crop = S/2: the exact-2x path of the paste; y >= 150: outside both neighbours
     ("out_of_crop", (5, 160, 85, 180), (30, 150), 40),             # the box sticks out of its crop on both sides
     ("clipped_bottom", (20, 235, 80, 258), (10, 230), 64)],        # 64 x 30 after the clip: non-square
    [("same_box", (10, 30, 60, 50), (5, 2), 64),
     ("tile_edge_last", (200, 20, 259, 60), (190, 0), 70)],         # columns 200 .. 258: both sides of the 256-column tile; the last item
]
FLAT = [(p, it) for p, items in enumerate(ITEMS) for it in items]
N = len(FLAT)
GUARD = 4096
nan, inf = float("nan"), float("inf")
# a tie (row 0), one NaN (row 1), all NaN (row 5); with threshold -1.0 rows 3 and 7 fall below it on pages where other boxes are kept
SCORES = [[-0.5, -0.5], [nan, -0.7], [-0.2, -0.9], [-3.0, -2.0], [-0.4, -0.3], [nan, nan], [-0.9, -0.1], [-1.5, -1.25], [-0.6, -0.8], [-0.3, -0.2],
          [-0.75, -0.5]]
THRESHOLD = -1.0


def _lists():
    return ([[list(i[1]) for i in items] for items in ITEMS], [[i[2] for i in items] for items in ITEMS], [[i[3] for i in items] for items in ITEMS])


@pytest.fixture(scope="module")
def ref():
    """pages, decoder outputs and the host pipeline's results, computed once and only read afterwards"""
    from oracle import prepost as OP
    rs = np.random.RandomState(20250131)
    pages = [rs.randint(0, 256, (h, w, 3), dtype=np.uint8) for h, w in PAGES]
    vae = (torch.randn(N, K, 3, S, S, generator=torch.Generator().manual_seed(5)) * 0.6).clamp(-1.3, 1.3)      # some values leave [-1, 1]
    pre = [OP.preprocess(pages[p], list(box), org[0], org[1], crop, S) for p, (_, box, org, crop) in FLAT]
    chains, unions, outside = [], [], []
    b = 0
    for p, items in enumerate(ITEMS):
        chain, union, out = pages[p], np.zeros(PAGES[p], np.uint8), np.ones(PAGES[p], bool)
        for _, box, org, crop in items:
            chain = OP.postprocess(vae[b, 0].numpy(), chain, list(box), org[0], org[1], crop)
            union |= OP.generate_mask((PAGES[p][1], PAGES[p][0]), box)
            out[box[1]:box[3], box[0]:box[2]] = False
            b += 1
        chains.append(chain); unions.append(union); outside.append(out)
    for a in pages + chains + unions + [v for d in pre for v in d.values()]:
        a.setflags(write=False)
    return dict(pages=pages, vae=vae, pre=pre, chains=chains, unions=unions, outside=outside)


@pytest.fixture(params=["bf16", "fp16"])
def build(request, monkeypatch, cuda):
    """route every prepost call of the test - single-box and paged - through one build of the library"""
    from diffute_amd import _cabi
    real = _cabi.lib
    real(request.param)
    monkeypatch.setattr(_cabi, "lib", lambda elem=None: real(request.param))
    return request.param


def _dev_pages(ref, cuda):
    return [torch.from_numpy(p.copy()).to(cuda) for p in ref["pages"]]


def _slab(fill, cuda):
    """one sentinel-filled uint8 buffer: guard | page 0 | guard | page 1 | ... | guard -> (buffer, the pages as views, the guards' slices)"""
    n = sum(h * w * 3 for h, w in PAGES) + GUARD * (len(PAGES) + 1)
    buf = torch.full((n,), fill, dtype=torch.uint8, device=cuda)
    views, guards, off = [], [], 0
    for h, w in PAGES:
        guards.append(slice(off, off + GUARD)); off += GUARD
        views.append(buf[off:off + h * w * 3].view(h, w, 3)); off += h * w * 3
    guards.append(slice(off, off + GUARD))
    return buf, views, guards


def _guards_intact(buf, guards, fill):
    return all(bool((buf[g] == fill).all()) for g in guards)


def test_items_cover_what_they_claim():
    names = [it[0] for _, it in FLAT]
    assert 8 <= N <= 12 and names[0] == "up_40_first" and names[-1] == "tile_edge_last" and [len(i) for i in ITEMS] == [5, 1, 3, 2]
    assert ITEMS[0][4][1:] == ITEMS[3][0][1:] and PAGES[2][0] > 150 >= max(PAGES[1][0], PAGES[3][0]) and ITEMS[2][0][1][1] >= 150
    assert sum(w > 256 and w % 256 != 0 for _, w in PAGES) == 2
    a, b = ITEMS[0][1][1], ITEMS[0][2][1]
    assert a[0] < b[2] and b[0] < a[2] and a[1] < b[3] and b[1] < a[3]
    for p, (_, box, org, crop) in FLAT:
        h, w = PAGES[p]
        assert 0 <= box[0] < box[2] <= w and 0 <= box[1] < box[3] <= h and 0 <= org[0] < w and 0 <= org[1] < h
    choice = RB.select(SCORES, THRESHOLD).tolist()
    assert choice == [0, 1, 0, -1, 1, 0, 1, -1, 0, 1, 1] and RB.select(SCORES).tolist() == [0, 1, 0, 1, 1, 0, 1, 1, 0, 1, 1]


def test_preprocess_pages_rows(cuda, build, ref):
    import diffute_amd as D
    imgs = _dev_pages(ref, cuda)
    boxes, origins, crops = _lists()
    got = D.prepost.preprocess_pages(imgs, boxes, origins, crops, size=S)
    D.synchronize()
    assert sorted(got) == ["image", "mask", "mask_latent", "masked_image"]
    assert got["image"].shape == (N, 3, S, S) and got["masked_image"].shape == (N, 3, S, S)
    assert got["mask"].shape == (N, 1, S, S) and got["mask"].dtype == torch.uint8 and got["mask_latent"].shape == (N, 1, S // 8, S // 8)
    host = {k: v.cpu().numpy() for k, v in got.items()}
    for b, (p, (name, box, org, crop)) in enumerate(FLAT):
        want = ref["pre"][b]
        for k in ("image", "masked_image", "mask", "mask_latent"):
            row = host[k][b] if k in ("image", "masked_image") else host[k][b, 0]
            assert np.array_equal(row, want[k]), f"{name}: {k} of row {b} (page {p}) differs from the host pipeline on its own page"
        one = D.prepost.preprocess(imgs[p], list(box), org[0], org[1], crop, size=S)
        for k in ("image", "masked_image", "mask", "mask_latent"):
            assert torch.equal(got[k][b:b + 1], one[k]), f"{name}: {k} of row {b} (page {p}) differs from the single-box kernel"
    assert not torch.equal(got["image"][4], got["image"][9]), "the same box on two pages shows two different pages"
    assert torch.equal(got["mask"][4], got["mask"][9])


def test_postprocess_pages_is_the_chain_of_single_pastes_per_page(cuda, build, ref):
    import diffute_amd as D
    imgs = _dev_pages(ref, cuda)
    vae = ref["vae"][:, 0].contiguous().to(cuda)
    boxes, origins, crops = _lists()
    for fill in (0, 255):                                  # a byte nobody wrote shows under one fill or the other
        buf, views, guards = _slab(fill, cuda)
        got, unions = D.prepost.postprocess_pages(vae, imgs, boxes, origins, crops, return_mask=True, out=views)
        D.synchronize()
        assert all(g.data_ptr() == v.data_ptr() for g, v in zip(got, views))
        assert _guards_intact(buf, guards, fill), "a guard band between the pages was written"
        b = 0
        for p, items in enumerate(ITEMS):
            host = got[p].cpu().numpy()
            assert host.shape == PAGES[p] + (3,) and got[p].dtype == torch.uint8
            assert np.array_equal(host, ref["chains"][p]), f"page {p} differs from oracle.prepost.postprocess chained over its items"
            chain = imgs[p]
            for _, box, org, crop in items:
                chain = D.prepost.postprocess(vae[b:b + 1], chain, list(box), org[0], org[1], crop)
                b += 1
            assert torch.equal(got[p], chain), f"page {p} differs from the single-box paste chained over its items"
            assert np.array_equal(host[ref["outside"][p]], ref["pages"][p][ref["outside"][p]]), "pixels outside every text box must be untouched"
            assert (host[~ref["outside"][p]] != ref["pages"][p][~ref["outside"][p]]).any()
            assert np.array_equal(unions[p].cpu().numpy(), ref["unions"][p]), f"union mask of page {p} differs from the OR of PIL's rectangles"
    plain = D.prepost.postprocess_pages(vae, imgs, boxes, origins, crops)              # pages of its own, no mask: the same bytes
    assert all(torch.equal(a, b_) for a, b_ in zip(plain, got))
    # where the two overlapping boxes of page 0 meet the later one wins: that patch is down_100_overlap's resize alone
    alone = D.prepost.postprocess(vae[2:3], imgs[0], boxes[0][2], origins[0][2][0], origins[0][2][1], crops[0][2])
    assert torch.equal(got[0][50:70, 150:200], alone[50:70, 150:200])


def test_readback_pages_rows(cuda, build, ref):
    import diffute_amd as D
    imgs = _dev_pages(ref, cuda)
    vae = ref["vae"].to(cuda)
    boxes, origins, crops = _lists()
    ip = D.TrOCRProcessor(size=SIZE, resample=RB.BILINEAR)
    n, shape = N * K * 3 * SIZE * SIZE, (N * K, 3, SIZE, SIZE)
    want = [RB.readback(ref["vae"][b, k].numpy(), ref["pages"][p], (it[1], it[2], it[3]), SIZE, RB.BILINEAR) for b, (p, it) in enumerate(FLAT)
            for k in range(K)]
    for fill in (0, 255):
        fbuf = torch.full((n + 2 * GUARD,), 12345.0, dtype=torch.float32, device=cuda)
        ubuf = torch.full((n + 2 * GUARD,), fill, dtype=torch.uint8, device=cuda)
        pv, u8 = D.prepost.readback_pixel_values_pages(vae, imgs, boxes, origins, crops, ip, out=fbuf[GUARD:GUARD + n].view(shape),
                                                       out_resized=ubuf[GUARD:GUARD + n].view(shape))
        D.synchronize()
        assert pv.data_ptr() == fbuf[GUARD:].data_ptr() and u8.data_ptr() == ubuf[GUARD:].data_ptr()
        assert bool((pv != 12345.0).all()), "an element of pixel_values was not written"
        for buf, f in ((fbuf, 12345.0), (ubuf, fill)):
            assert bool((buf[:GUARD] == f).all()) and bool((buf[-GUARD:] == f).all()), "a guard band was written"
        pv_h, u8_h = pv.cpu().numpy(), u8.cpu().numpy()
        for r, (r_u8, r_pv) in enumerate(want):
            p, it = FLAT[r // K]
            assert np.array_equal(u8_h[r], r_u8), f"{it[0]} (page {p}), candidate {r % K}: resized bytes differ from the chain on its own page"
            assert np.array_equal(pv_h[r].view(np.uint32), r_pv.view(np.uint32)), f"{it[0]} (page {p}), candidate {r % K}: pixel_values differ"
    assert torch.equal(D.prepost.readback_pixel_values_pages(vae, imgs, boxes, origins, crops, ip), pv)
    # ... and each page's rows are what the one-page kernel gives for that page alone
    b = 0
    for p, items in enumerate(ITEMS):
        one = D.prepost.readback_pixel_values(vae[b:b + len(items)], imgs[p], boxes[p], origins[p], crops[p], ip)
        assert torch.equal(pv[b * K:(b + len(items)) * K], one), f"page {p}"
        b += len(items)


@pytest.mark.parametrize("threshold", [None, THRESHOLD], ids=["none", "thr-1"])
def test_select_pages(cuda, build, ref, threshold):
    import diffute_amd as D
    imgs = _dev_pages(ref, cuda)
    vae = ref["vae"].to(cuda)
    boxes, origins, crops = _lists()
    scores = np.array(SCORES, dtype=np.float32)
    want = RB.select(scores, -np.inf if threshold is None else threshold)
    buf, views, guards = _slab(0x5A, cuda)
    got, choice, unions = D.prepost.postprocess_select_pages(vae, torch.from_numpy(scores).to(cuda), imgs, boxes, origins, crops, threshold=threshold,
                                                             return_mask=True, out=views)
    D.synchronize()
    assert choice.dtype == torch.int32 and choice.shape == (N,) and choice.cpu().numpy().tolist() == want.tolist()
    assert _guards_intact(buf, guards, 0x5A)
    b = 0
    for p, items in enumerate(ITEMS):
        chain = imgs[p]
        for _, box, org, crop in items:                   # the chain of single pastes of the chosen rows; a skipped box keeps the original
            if want[b] >= 0:
                chain = D.prepost.postprocess(vae[b, int(want[b])], chain, list(box), org[0], org[1], crop)
            b += 1
        assert torch.equal(got[p], chain), f"page {p} differs from the chain of single pastes of the chosen rows"
        assert np.array_equal(unions[p].cpu().numpy(), ref["unions"][p]), "the union mask covers the boxes of ALL items, skipped ones included"
    if threshold is not None:
        x1, y1, x2, y2 = ITEMS[0][3][1]                      # clipped_corner fell below the threshold: original pixels, its neighbours pasted
        assert torch.equal(got[0][y1:y2, x1:x2], imgs[0][y1:y2, x1:x2]) and not torch.equal(got[0], imgs[0])
    got2, choice2 = D.prepost.postprocess_select_pages(vae, torch.from_numpy(scores).to(cuda), imgs, boxes, origins, crops, threshold=threshold)
    assert torch.equal(choice2, choice) and all(torch.equal(a, b_) for a, b_ in zip(got2, got))


class _Recorder:
    """the library, noting the name of every dmx_* function called through it"""

    def __init__(self, lib, names):
        self._lib, self._names = lib, names

    def __getattr__(self, name):
        fn = getattr(self._lib, name)
        if not name.startswith("dmx_"):
            return fn

        def call(*args):
            self._names.append(name)
            return fn(*args)
        return call


def test_each_function_reaches_its_own_entry(cuda, build, ref, monkeypatch):
    """a one-page function prepares an item table and runs the one-page entry (its kernel), a paged one a page table and the *_pages
    entry: one prepare and one launch per call, nothing else"""
    import diffute_amd as D
    from diffute_amd import _cabi
    P = D.prepost
    names = []
    rec = _Recorder(_cabi.lib(), names)
    monkeypatch.setattr(_cabi, "lib", lambda elem=None: rec)
    imgs = _dev_pages(ref, cuda)
    boxes, origins, crops = _lists()
    n0 = len(ITEMS[0])
    vae = ref["vae"].to(cuda)
    v0, scores = vae[:, 0].contiguous(), torch.tensor(SCORES, device=cuda)
    ip = D.TrOCRProcessor(size=SIZE, resample=RB.BILINEAR)
    one, pages = (imgs[0], boxes[0], origins[0], crops[0]), (imgs, boxes, origins, crops)
    calls = [("dmx_preprocess_crop_batch", lambda: P.preprocess_batch(*one, size=S)),
             ("dmx_postprocess_paste_batch", lambda: P.postprocess_batch(v0[:n0], *one)),
             ("dmx_readback_pixel_values", lambda: P.readback_pixel_values(vae[:n0], *one, ip)),
             ("dmx_postprocess_paste_select", lambda: P.postprocess_select_batch(vae[:n0], scores[:n0], *one)),
             ("dmx_preprocess_crop_pages", lambda: P.preprocess_pages(*pages, size=S)),
             ("dmx_postprocess_paste_pages", lambda: P.postprocess_pages(v0, *pages)),
             ("dmx_readback_pixel_values_pages", lambda: P.readback_pixel_values_pages(vae, *pages, ip)),
             ("dmx_postprocess_paste_select_pages", lambda: P.postprocess_select_pages(vae, scores, *pages))]
    for entry, fn in calls:
        del names[:]
        fn()
        got = [n for n in names if not ("readback" in entry and n == "dmx_glyph_max_taps")]
        assert got == ["dmx_edit_pages_prepare" if entry.endswith("_pages") else "dmx_edit_items_prepare", entry], entry
    D.synchronize()


def test_one_page_in_the_paged_form_is_the_one_page_form(cuda, build, ref):
    """page 0 alone, passed as a list of one page: every output equals the one-page function's, bit for bit"""
    import diffute_amd as D
    P = D.prepost
    img = _dev_pages(ref, cuda)[0]
    boxes, origins, crops = (l[0] for l in _lists())
    n0 = len(ITEMS[0])
    vae = ref["vae"][:n0].to(cuda)
    v0, scores = vae[:, 0].contiguous(), torch.tensor(SCORES[:n0], device=cuda)
    ip = D.TrOCRProcessor(size=SIZE, resample=RB.BILINEAR)
    one, paged = (img, boxes, origins, crops), ([img], [boxes], [origins], [crops])
    a, b = P.preprocess_batch(*one, size=S), P.preprocess_pages(*paged, size=S)
    assert sorted(a) == sorted(b) and all(torch.equal(a[k], b[k]) for k in a)
    (a, am), (b, bm) = P.postprocess_batch(v0, *one, return_mask=True), P.postprocess_pages(v0, *paged, return_mask=True)
    assert len(b) == 1 and len(bm) == 1 and torch.equal(a, b[0]) and torch.equal(am, bm[0])
    (a, au), (b, bu) = P.readback_pixel_values(vae, *one, ip, return_resized=True), P.readback_pixel_values_pages(vae, *paged, ip, return_resized=True)
    assert torch.equal(a, b) and torch.equal(au, bu)
    a, ac, am = P.postprocess_select_batch(vae, scores, *one, threshold=THRESHOLD, return_mask=True)
    b, bc, bm = P.postprocess_select_pages(vae, scores, *paged, threshold=THRESHOLD, return_mask=True)
    D.synchronize()
    assert ac.tolist() == [0, 1, 0, -1, 1], "page 0's scores hold a tie, a NaN and a box below the threshold"
    assert len(b) == 1 and len(bm) == 1 and torch.equal(a, b[0]) and torch.equal(ac, bc) and torch.equal(am, bm[0])


def test_refusals_launch_nothing(cuda, ref):
    """a bad item, a bad output list and a host table spoiled after the prepare: an error, and the sentinel-filled slab stays as it was"""
    import diffute_amd as D
    from diffute_amd import _cabi, prepost
    imgs = _dev_pages(ref, cuda)
    vae = ref["vae"].to(cuda)
    boxes, origins, crops = _lists()
    ip = D.TrOCRProcessor(size=SIZE, resample=RB.BILINEAR)
    buf, views, guards = _slab(0x5A, cuda)
    scores = torch.zeros(N, K, device=cuda)
    bad = [list(o) for o in origins]
    bad[1][0] = (140, 0)                                   # outside its own 131-wide page, inside the 300-wide one before it: item 5
    with pytest.raises(RuntimeError, match="item 5"):
        prepost.postprocess_pages(vae[:, 0].contiguous(), imgs, boxes, bad, crops, out=views)
    with pytest.raises(RuntimeError, match="item 5"):
        prepost.postprocess_select_pages(vae, scores, imgs, boxes, bad, crops, out=views)
    with pytest.raises(RuntimeError, match="item 5"):
        prepost.preprocess_pages(imgs, boxes, bad, crops, size=S)
    with pytest.raises(RuntimeError, match="item 5"):
        prepost.readback_pixel_values_pages(vae, imgs, boxes, bad, crops, ip)
    wide = [[list(b) for b in bs] for bs in boxes]
    wide[1][0][2] = 140                                    # the box ends outside its own page: the read-back's per-page check
    with pytest.raises(ValueError, match="page 1"):
        prepost.readback_pixel_values_pages(vae, imgs, wide, origins, crops, ip)
    # the output list: too short, a page as its own output, two outputs that share memory, another dtype
    for out in (views[:3], views[:3] + [imgs[3]], views[:3] + [views[2].reshape(-1)[:70 * 260 * 3].view(70, 260, 3)],
                [v.to(torch.int8) for v in views]):
        with pytest.raises(ValueError):
            prepost.postprocess_pages(vae[:, 0].contiguous(), imgs, boxes, origins, crops, out=out)
    with pytest.raises(TypeError):
        prepost.postprocess_pages(ref["vae"][:, 0], imgs, boxes, origins, crops, out=views)
    # the launch entries themselves, with real addresses and good device tables: only the host tables are spoiled
    lib = _cabi.lib()
    flat = lambda ll: [x for l in ll for x in l]
    v0 = vae[:, 0].contiguous()
    choice = torch.full((N,), 77, dtype=torch.int32, device=cuda)
    for spoil in ("item", "page"):
        host, pages, stage, dbuf, offs = prepost._upload_pages(imgs, flat(boxes), flat(origins), flat(crops), [len(b) for b in boxes], S, cuda, views, None)
        if spoil == "item":
            host[6].y_s = 260                              # the first row below page 2
        else:
            pages[3].W = 131
        base = dbuf.data_ptr()
        assert lib.dmx_postprocess_paste_pages(_cabi.ptr(v0), S, pages, base + offs[0], 4, host, base, N, _cabi.current_stream()) == -1
        assert ("item 6" if spoil == "item" else "page 3") in lib.dmx_last_error().decode()
        assert lib.dmx_postprocess_paste_select_pages(_cabi.ptr(vae), S, _cabi.ptr(scores), -inf, _cabi.ptr(choice), pages, base + offs[0], 4,
                                                      host, base, N, K, _cabi.current_stream()) == -1
    _cabi.synchronize()
    assert bool((buf == 0x5A).all()), "refused, yet something was written"
    assert bool((choice == 77).all())
