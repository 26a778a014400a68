"""The host half of "several text boxes of one image in one batch" (prepost.plan_edits / preprocess_batch / postprocess_batch,
pipeline.edit_boxes): the crop plan against the oracle's restatement of the notebook, the argument checks that run before anything
touches the GPU, and the item table (dmx_edit_item) through the C-ABI's host-only entry.  Nothing here needs a GPU."""
import ctypes

import numpy as np
import pytest
import torch

# (h, w), boxes: every rung of the ladder (6 * height < 128, 256, 384, 512, 640, 784, 1000, and past the last one), a box wider
# than its rung, and - on the flat image, whose short side caps the crop below the box width - two origins that are DRAWN
LADDER = ((1100, 1300), [(100, 100, 180, 110), (100, 100, 180, 130), (100, 100, 180, 150), (100, 100, 180, 170), (100, 100, 180, 190),
                         (100, 100, 180, 220), (100, 100, 180, 250), (100, 100, 180, 300), (40, 40, 400, 60), (0, 0, 60, 12),
                         (1200, 1050, 1299, 1099)])
DRAWN = ((300, 1400), [(100, 100, 1000, 110), (20, 30, 80, 44), (300, 200, 1350, 240), (100, 100, 1000, 110)])


@pytest.mark.parametrize("case", [LADDER, DRAWN], ids=["ladder", "drawn_origins"])
def test_plan_edits_is_the_reference_rule_per_box(case):
    from diffute_amd import prepost
    from oracle import prepost as OP
    (h, w), boxes = case
    mine, rng = np.random.RandomState(7), np.random.RandomState(7)
    got = prepost.plan_edits(boxes, h, w, mine)
    want = []
    for box in boxes:                                   # one stream, consumed in box order, as N reference calls would
        crop = OP.crop_scale_for(box, h, w)
        want.append(OP.crop_origin(box, crop, w, rng) + (crop,))
    assert got == want
    assert all(isinstance(v, int) for plan in got for v in plan)
    assert mine.randint(1 << 30) == rng.randint(1 << 30), "plan_edits drew more or fewer numbers than the per-box calls"
    if case is LADDER:
        assert [p[2] for p in got[:8]] == [128, 256, 384, 512, 640, 784, 1000, 1100]
    else:
        assert got[0] != got[3], "boxes 0 and 3 are equal: each must get a draw of its own (true for this seed)"


def test_batched_functions_check_their_lists_first_and_refuse_host_tensors():
    from diffute_amd import prepost
    img = torch.zeros(64, 80, 3, dtype=torch.uint8)
    vae = torch.zeros(1, 3, 16, 16)
    box, org = [(4, 4, 30, 12)], [(0, 0)]
    for fn, first in ((prepost.preprocess_batch, img), (prepost.postprocess_batch, vae)):
        args = (first,) if fn is prepost.preprocess_batch else (first, img)
        with pytest.raises(ValueError):
            fn(*args, [], [], [])                                   # B = 0
        with pytest.raises(ValueError):
            fn(*args, box * 65, org * 65, [32] * 65)                # B > 64
        with pytest.raises(ValueError):
            fn(*args, box * 2, org, [32, 32])                       # mismatched lengths
        with pytest.raises(ValueError):
            fn(*args, box * 2, org * 2, [32])
        with pytest.raises(TypeError):
            fn(*args, box, org, [32])                               # host tensors: no CPU fallback
        with pytest.raises(TypeError):
            fn(*args, box * 64, org * 64, [32] * 64)                # B = 64 passes the list checks


def test_public_names():
    import diffute_amd as D
    from diffute_amd import edit_boxes, prepost
    assert "edit_boxes" in D.__all__ and callable(edit_boxes)
    for name in ("plan_edits", "preprocess_batch", "postprocess_batch"):
        assert callable(getattr(prepost, name)) and callable(getattr(D.prepost, name))


def _items(rows):
    from diffute_amd import _cabi
    arr = (_cabi.EditItem * len(rows))()
    for it, (box, (x_s, y_s), crop) in zip(arr, rows):
        it.x1, it.y1, it.x2, it.y2 = box
        it.x_s, it.y_s, it.crop_scale = x_s, y_s, crop
    return arr


def test_item_table_layout_and_derived_fields():
    """dmx_edit_item as ctypes sees it is what the header declares (12 ints, 4 doubles), and the prepare entry fills the derived fields
    with the host arithmetic of the single-box entries: extent clipped at the border, double scales, the exact-2x flags."""
    from diffute_amd import _cabi
    assert ctypes.sizeof(_cabi.EditItem) == 12 * 4 + 4 * 8 and _cabi.EditItem.pre_sx.offset == 48
    arr = _items([((150, 120, 230, 138), (120, 60), 128), ((400, 500, 900, 620), (70, 40), 1024), ((950, 1020, 1100, 1060), (900, 1000), 256),
                  ((10, 10, 40, 20), (0, 0), 256)])
    for elem in ("bf16", "fp16"):
        lib = _cabi.lib(elem)
        _cabi.check(lib.dmx_edit_items_prepare(arr, 4, 1100, 1300, 512), "prepare", lib)
        assert [(it.cw, it.ch, it.pre_area2, it.post_area2) for it in arr] == [(128, 128, 0, 0), (1024, 1024, 1, 0), (256, 100, 0, 0), (256, 256, 0, 1)]
        assert (arr[2].pre_sx, arr[2].pre_sy, arr[2].post_sx, arr[2].post_sy) == (256 / 512, 100 / 512, 512 / 256, 512 / 100)
        assert (arr[0].x1, arr[0].y2, arr[0].x_s, arr[0].crop_scale) == (150, 138, 120, 128)       # the caller's fields are untouched


def test_bad_item_is_reported_by_index_before_any_launch():
    """the entries check the HOST table item by item and return before they launch: callable without a GPU, with dummy addresses"""
    from diffute_amd import _cabi
    lib = _cabi.lib()
    one = ctypes.c_void_p(64)
    good = ((10, 10, 40, 20), (0, 0), 64)
    for bad, word in ((((10, 10, 40, 20), (1300, 0), 64), "origin"), (((10, 10, 40, 20), (0, 1100), 64), "origin"),
                      (((10, 10, 40, 20), (-1, 0), 64), "origin"), (((10, 10, 40, 20), (0, 0), 0), "crop_scale")):
        arr = _items([good, good, bad, good])
        assert lib.dmx_edit_items_prepare(arr, 4, 1100, 1300, 512) != 0
        msg = lib.dmx_last_error().decode()
        assert "item 2" in msg and word in msg, msg
    arr = _items([good, good])
    assert lib.dmx_edit_items_prepare(arr, 0, 1100, 1300, 512) != 0 and lib.dmx_edit_items_prepare(arr, 65, 1100, 1300, 512) != 0
    assert lib.dmx_edit_items_prepare(arr, 2, 65536, 1300, 512) != 0, "H <= 65535: the paste's grid has one row of blocks per image row"
    _cabi.check(lib.dmx_edit_items_prepare(arr, 2, 1100, 1300, 512), "prepare")
    arr[1].x_s = 1300                                   # spoiled after the prepare: both launch entries refuse it, by index
    assert lib.dmx_preprocess_crop_batch(one, 1100, 1300, arr, one, 2, 512, one, one, one, one, None) != 0
    assert "item 1" in lib.dmx_last_error().decode()
    assert lib.dmx_postprocess_paste_batch(one, 512, one, one, None, 1100, 1300, arr, one, 2, None) != 0
    assert "item 1" in lib.dmx_last_error().decode()
    arr[1].x_s = 0
    arr[1].cw = 63                                      # a table prepared for another image / S is refused as well
    assert lib.dmx_preprocess_crop_batch(one, 1100, 1300, arr, one, 2, 512, one, one, one, one, None) != 0
    assert "item 1" in lib.dmx_last_error().decode() and "derived" in lib.dmx_last_error().decode()
    arr[1].cw = 64
    assert lib.dmx_preprocess_crop_batch(one, 1100, 1300, arr, one, 65, 512, one, one, one, one, None) != 0
    assert lib.dmx_preprocess_crop_batch(one, 1100, 1300, arr, one, 2, 100, one, one, one, one, None) != 0, "S must be a multiple of 8"
