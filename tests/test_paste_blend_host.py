"""The feathered, colour-matched paste without a GPU: the integer restatement (tests/paste_blend_restatement.py) against the oracle's plain
paste and against the properties the rule promises, injected faults that must each show in the bytes of a case, PasteBlend's own checks,
and the new entries of the C ABI - present in both builds and in the header's parse, and refusing bad parameters before any launch."""
import ctypes

import numpy as np
import pytest
import torch

import paste_blend_cases as PC
import paste_blend_restatement as PB

ONE = ctypes.c_void_p(64)            # a dummy device address: the refusals return before any launch
SYMBOLS = ("dmx_paste_color_stats", "dmx_paste_color_stats_pages", "dmx_postprocess_paste_blend", "dmx_postprocess_paste_blend_pages",
           "dmx_select_choices")


@pytest.fixture(scope="module")
def cases():
    return {c.name: c for c in PC.cases()}


@pytest.fixture(scope="module")
def expected(cases):
    return {name: c.expected() for name, c in cases.items()}


def test_everything_off_is_the_chain_of_the_oracles_pastes(cases):
    """feather = grow = 0 without match_color, for the geometry of EVERY case: oracle.prepost.postprocess chained in item order, a later item
    winning where boxes overlap"""
    from oracle import prepost as OP
    for c in cases.values():
        off = PC.Case(c.name, c.S, c.pages, c.items, c.rows, PB.Blend(), c.choice)
        b = 0
        for pg, its, (out, mask, stats) in zip(c.pages, c.items, off.expected()):
            chain = pg
            for box, org, crop in its:
                if c.chosen(b) is not None:
                    chain = OP.postprocess(c.chosen(b), chain, list(box), org[0], org[1], crop)
                b += 1
            assert stats is None and np.array_equal(out, chain), c.name


def test_a_constant_shift_comes_back_as_the_original_page():
    """a decoder output equal to the crop plus a constant per channel: the colour match removes the constant exactly, whatever the ramp"""
    A = PC.page(PC.PAGE_A, 1)
    box, org = (20, 12, 32, 19), (17, 8)
    for shift in ((7, -5, 11), (-7, 5, -11), (32, -32, 0)):
        row = PC.shifted_row(A, org, 16, shift)
        for blend in (PB.Blend(feather=2, grow=2, match_color=True), PB.Blend(feather=0, grow=0, match_color=True, ring=1),
                      PB.Blend(feather=5, grow=1, match_color=True, ring=3)):
            out, mask, stats = PB.paste_chain(A, [(row, box, org, 16)], blend)
            n = stats[0][0]
            assert n > 0 and stats[0][1:] == tuple(-s * n for s in shift)
            assert np.array_equal(out, A), (shift, blend.kwargs())
        hard, _, _ = PB.paste_chain(A, [(row, box, org, 16)], PB.Blend(feather=2, grow=2))
        assert not np.array_equal(hard, A), "without the colour match the shift shows"


def test_pixels_outside_the_union_mask_are_untouched(cases, expected):
    for name, c in cases.items():
        for pg, its, (out, mask, _) in zip(c.pages, c.items, expected[name]):
            assert set(np.unique(mask)) <= {0, 1} and mask.any() and not mask.all()
            assert np.array_equal(out[mask == 0], pg[mask == 0]), name
            grown = np.zeros_like(mask)
            for box, _, _ in its:                                  # every paste rectangle lies inside its grown box
                g = c.blend.grow
                grown[max(box[1] - g, 0):box[3] + g, max(box[0] - g, 0):box[2] + g] = 1
            assert not (mask & ~grown & 1).any(), name


def test_max_shift_clamps(cases, expected):
    c = cases["beyond_max_shift"]
    (out, _, stats), = expected["beyond_max_shift"]
    n = stats[0][0]
    assert n > 0 and stats[0][1:] == (5 * n, -5 * n, 5 * n)
    free = PC.Case("free", c.S, c.pages, c.items, c.rows, PB.Blend(feather=1, grow=1, match_color=True, max_shift=255))
    (out_free, _, stats_free), = free.expected()
    assert all(abs(d) > 25 * n for d in stats_free[0][1:]) and not np.array_equal(out, out_free)
    zero = PC.Case("zero", c.S, c.pages, c.items, c.rows, PB.Blend(feather=1, grow=1, match_color=True, max_shift=0))
    plain = PC.Case("plain", c.S, c.pages, c.items, c.rows, PB.Blend(feather=1, grow=1))
    assert np.array_equal(zero.expected()[0][0], plain.expected()[0][0]), "max_shift = 0 is no correction"


def test_stats_depend_neither_on_the_order_nor_on_the_batch(cases, expected):
    ab, ba = expected["overlap_ab"][0][2], expected["overlap_ba"][0][2]
    assert ab == ba[::-1] and ab[0] != ab[1]
    c = cases["overlap_ab"]
    for b, (box, org, crop) in enumerate(c.items[0]):
        _, _, alone = PB.paste_chain(c.pages[0], [(c.rows[b, 0], box, org, crop)], c.blend)
        assert alone[0] == ab[b]
    assert not np.array_equal(expected["overlap_ab"][0][0], expected["overlap_ba"][0][0]), "the PASTE does depend on the order"


def test_cases_cover_what_they_claim(cases, expected):
    from oracle import prepost as OP
    names = list(cases)
    assert len(names) == 16 and max(c.N for c in cases.values()) == 64
    st = lambda name, b=0, p=0: expected[name][p][2][b]
    assert st("box_fills_crop") == (0, 0, 0, 0)
    assert all(d < 0 for d in st("negative_D")[1:]) and any((2 * d + st("negative_D")[0]) % (2 * st("negative_D")[0]) for d in st("negative_D")[1:])
    assert st("k2_choice_skip", 1) == (0, 0, 0, 0) and st("k2_choice_skip", 0)[0] > 0
    c = cases["rect_empty"]                                        # no paste rectangle, yet a ring: n > 0 and the page is the first item's alone
    (box, org, crop) = c.items[0][1]
    assert box[0] >= org[0] + crop and st("rect_empty", 1)[0] > 0
    alone = PC.Case("alone", c.S, c.pages, [c.items[0][:1]], c.rows[:1], c.blend).expected()[0]
    assert np.array_equal(alone[0], expected["rect_empty"][0][0]) and np.array_equal(alone[1], expected["rect_empty"][0][1])
    c = cases["feather_never_full"]                                # an 8 x 6 rectangle, F = 10: a <= 3
    box = c.items[0][0][0]
    assert min(box[2] - box[0], box[3] - box[1]) < 2 * (c.blend.feather + 1)
    c = cases["grow_past_extent"]                                  # the grown box leaves the crop on two sides
    (box, org, crop), = c.items[0]
    assert box[0] - c.blend.grow < org[0] and box[1] - c.blend.grow < org[1]
    (box, org, crop), = cases["corner_clipped"].items[0]
    assert box[2] == PC.PAGE_A[1] and box[3] == PC.PAGE_A[0] and org[0] + crop > PC.PAGE_A[1] and org[1] + crop > PC.PAGE_A[0]
    assert cases["exact_2x"].S == 2 * cases["exact_2x"].items[0][0][2] and cases["identity"].S == cases["identity"].items[0][0][2]
    a, b = (i[0] for i in cases["overlap_ab"].items[0])
    assert a[0] < b[2] and b[0] < a[2] and a[1] < b[3] and b[1] < a[3]
    assert [p.shape[:2] for p in cases["two_pages"].pages] == [PC.PAGE_A, PC.PAGE_B]
    for c in cases.values():                                       # every item is one the C side accepts
        for pg, its in zip(c.pages, c.items):
            for box, org, crop in its:
                assert 0 <= org[0] < pg.shape[1] and 0 <= org[1] < pg.shape[0] and crop > 0 and box[0] < box[2] and box[1] < box[3]


def test_the_shift_form_of_the_correction_gives_the_same_bytes(cases, expected):
    """floor((2 (G n + D) + n) / (2 n)) = G + floor((2 D + n) / (2 n)): what lets the kernel divide once per item instead of once per pixel"""
    for name, c in cases.items():
        assert all(np.array_equal(w[0], g[0]) for w, g in zip(expected[name], c.expected("shift_form"))), name
    g = np.arange(256, dtype=np.int64).reshape(16, 16, 1).repeat(3, 2)
    for n, D in ((7, (-1785, 1785, -3)), (1, (0, -255, 255)), (1000, (-255000, 1, -1)), (13, (-6, -7, 6))):
        D = np.array(D, dtype=np.int64)
        assert np.array_equal(PB.corrected(g, n, D), PB.corrected(g, n, D, "shift_form"))


@pytest.mark.parametrize("fault", PB.FAULTS)
def test_an_injected_fault_changes_the_bytes_of_a_case(cases, expected, fault):
    hit = [name for name, c in cases.items()
           if any(not np.array_equal(w[0], g[0]) for w, g in zip(expected[name], c.expected(fault)))]
    assert hit, f"no case notices `{fault}`"
    if fault == "trunc_div":
        assert "negative_D" in hit
    if fault == "descending":
        assert "overlap_ab" in hit and "identity" not in hit
    if fault == "stats_from_chain":
        assert set(hit) <= {"overlap_ab", "overlap_ba", "k2_choice_skip", "two_pages", "b64", "rect_empty"}, "a single item has no chain to read from"


def test_paste_blend_checks_its_fields():
    import diffute_amd as D
    from diffute_amd import _cabi, prepost
    assert D.PasteBlend is prepost.PasteBlend and "PasteBlend" in D.__all__
    d = D.PasteBlend()
    assert (d.feather, d.grow, d.match_color, d.ring, d.max_shift) == (0, 0, False, 8, 32)
    b = D.PasteBlend(feather=4, grow=3, match_color=True, ring=2, max_shift=255)
    s = b._struct()
    assert (s.feather, s.grow, s.ring, s.max_shift, s.match_color) == (4, 3, 2, 255, 1) and ctypes.sizeof(_cabi.PasteBlend) == 20
    for bad in (dict(feather=-1), dict(grow=-1), dict(ring=0), dict(max_shift=-1), dict(max_shift=256), dict(feather=_cabi.PASTE_BLEND_MAX + 1),
                dict(grow=_cabi.PASTE_BLEND_MAX + 1), dict(ring=_cabi.PASTE_BLEND_MAX + 1)):
        with pytest.raises(ValueError):
            D.PasteBlend(**bad)
    for bad in (dict(feather=1.5), dict(grow="2"), dict(ring=None), dict(max_shift=True), dict(match_color=1)):
        with pytest.raises(TypeError):
            D.PasteBlend(**bad)
    assert b.grown([(10, 12, 30, 20), (1, 1, 55, 39)]) == [(7, 9, 33, 23), (-2, -2, 58, 42)]
    assert b.grown([(10, 12, 30, 20), (1, 1, 55, 39)], 40, 56) == [(7, 9, 33, 23), (0, 0, 56, 40)]


def test_python_functions_refuse_a_bad_blend_without_a_gpu():
    import diffute_amd as D
    from diffute_amd import prepost
    img = torch.zeros(64, 80, 3, dtype=torch.uint8)
    with pytest.raises(NotImplementedError, match="quads"):
        D.edit_quads(None, None, None, [img], [[[(4, 4), (30, 4), (30, 12), (4, 12)]]], None, 3, blend=D.PasteBlend(feather=1))
    for call in (lambda: D.edit_boxes(None, None, None, img, [(4, 4, 30, 12)], torch.zeros(1, 77, 128), 3, blend="soft"),
                 lambda: D.edit_pages(None, None, None, [img], [[(4, 4, 30, 12)]], torch.zeros(1, 77, 128), 3, blend=dict(feather=1))):
        with pytest.raises(TypeError, match="PasteBlend"):
            call()
    with pytest.raises(TypeError):                                  # a good blend passes the list checks: the host tensor is what is refused
        prepost.postprocess_batch(torch.zeros(1, 3, 16, 16), img, [(4, 4, 30, 12)], [(0, 0)], [32], blend=D.PasteBlend(feather=1))
    with pytest.raises(ValueError):
        prepost.postprocess_pages(torch.zeros(1, 3, 16, 16), [], [], [], [], blend=D.PasteBlend(feather=1))
    with pytest.raises(TypeError):
        prepost.paste_color_stats(torch.zeros(1, 3, 16, 16), img, [(4, 4, 30, 12)], [(0, 0)], [32], D.PasteBlend(match_color=True))


def test_the_new_entries_are_in_the_header_and_in_both_builds():
    from diffute_amd import _cabi
    assert _cabi.PASTE_BLEND_MAX == 1 << 20
    assert [n for n, _ in _cabi.PasteBlend._fields_] == ["feather", "grow", "ring", "max_shift", "match_color"]
    for name in SYMBOLS:
        assert name in _cabi.exported_symbols()
        res, args = _cabi._PROTOS[name]
        assert res is ctypes.c_int and args[-1] is ctypes.c_void_p
    assert _cabi._PROTOS["dmx_select_choices"][1] == [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_float, ctypes.c_void_p, ctypes.c_void_p]
    for elem in ("bf16", "fp16"):
        lib = _cabi.lib(elem)
        for name in SYMBOLS:
            assert callable(getattr(lib, name))


def _tables(lib, S=16):
    from diffute_amd import _cabi
    pt, arr = (_cabi.EditPage * 1)(), (_cabi.EditItem * 1)()
    pt[0].original, pt[0].out, pt[0].union_mask = 64, 128, 0
    pt[0].H, pt[0].W, pt[0].item_lo, pt[0].item_hi = 40, 56, 0, 1
    arr[0].x1, arr[0].y1, arr[0].x2, arr[0].y2 = 20, 12, 32, 19
    arr[0].x_s, arr[0].y_s, arr[0].crop_scale = 17, 8, 16
    _cabi.check(lib.dmx_edit_pages_prepare(pt, 1, arr, 1, S), "prepare", lib)
    return pt, arr


def test_entries_refuse_bad_parameters_before_they_launch():
    """every call below must be refused - the addresses are dummies, so a launch would be visible as a crash on a GPU and is impossible here"""
    from diffute_amd import _cabi
    for elem in ("bf16", "fp16"):
        lib = _cabi.lib(elem)
        pt, arr = _tables(lib)

        def entries(bl, stats=ONE, choice=None, K=1):
            r = ctypes.byref(bl) if bl is not None else None
            return (lambda: lib.dmx_paste_color_stats(ONE, 16, ONE, 40, 56, arr, ONE, 1, r, choice, K, ONE, None),
                    lambda: lib.dmx_paste_color_stats_pages(ONE, 16, pt, ONE, 1, arr, ONE, 1, r, choice, K, ONE, None),
                    lambda: lib.dmx_postprocess_paste_blend(ONE, 16, ONE, ONE, None, 40, 56, arr, ONE, 1, r, stats, choice, K, None),
                    lambda: lib.dmx_postprocess_paste_blend_pages(ONE, 16, pt, ONE, 1, arr, ONE, 1, r, stats, choice, K, None))

        def refused(calls, *words):
            for call in calls:
                assert call() != 0, words
                msg = lib.dmx_last_error().decode()
                assert all(w in msg for w in words), msg
        B = _cabi.PasteBlend
        cap = _cabi.PASTE_BLEND_MAX
        refused(entries(B(-1, 0, 8, 32, 0)), "feather")
        refused(entries(B(cap + 1, 0, 8, 32, 0)), "feather")
        refused(entries(B(0, -1, 8, 32, 0)), "grow")
        refused(entries(B(0, cap + 1, 8, 32, 0)), "grow")
        refused(entries(B(0, 0, 0, 32, 0)), "ring")
        refused(entries(B(0, 0, 8, 256, 0)), "max_shift")
        refused(entries(B(0, 0, 8, -1, 0)), "max_shift")
        refused(entries(B(0, 0, 8, 32, 2)), "match_color")
        refused(entries(None), "blend")
        refused(entries(B(1, 1, 8, 32, 0), K=2), "choice")             # two candidates and no choice table
        refused(entries(B(1, 1, 8, 32, 0), choice=ONE, K=17), "candidates")
        refused(entries(B(1, 1, 8, 32, 0), choice=ONE, K=0), "candidates")
        refused(entries(B(1, 1, 8, 32, 1), stats=None)[2:], "statistics")   # match_color without stats: the two pastes
        arr[0].x_s = 56                                                 # the plain entries' table checks apply unchanged
        refused(entries(B(1, 1, 8, 32, 0)), "item 0", "origin")
        arr[0].x_s = 17
        pt[0].out = pt[0].original
        refused(entries(B(1, 1, 8, 32, 0))[3:], "page 0")
        assert lib.dmx_select_choices(ONE, 0, 2, 0.0, ONE, None) != 0 and "items" in lib.dmx_last_error().decode()
        assert lib.dmx_select_choices(ONE, 65, 2, 0.0, ONE, None) != 0
        assert lib.dmx_select_choices(ONE, 4, 17, 0.0, ONE, None) != 0 and "candidates" in lib.dmx_last_error().decode()
        assert lib.dmx_select_choices(ONE, 4, 2, float("nan"), ONE, None) != 0 and "NaN" in lib.dmx_last_error().decode()
        assert lib.dmx_select_choices(None, 4, 2, 0.0, ONE, None) != 0
