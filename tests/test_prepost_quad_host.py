"""The host half of the quadrilateral regions with oriented crops (csrc/prepost_quad.h, prepost.frame_for / plan_quads, the C-ABI's
host-only dmx_edit_quads_prepare): the prepared integers against the closed form in numpy float64, the Q16 map against the exact affine
map, the properties of the numpy restatement the GPU tests compare against (tests/quad_restatement.py) - invariance under a quarter
turn, the exact-copy identities - with injected faults that must break them, every refusal by index, and the crop plan on hand-computed
cases.  Nothing here needs a GPU."""
import ctypes

import numpy as np
import pytest
import torch

import quad_cases as QC
import quad_restatement as QR

S = QC.S
ONE = ctypes.c_void_p(64)            # a dummy device address: the refusals return before any launch


def _prepared(lib=None, S_=S):
    from diffute_amd import _cabi
    lib = lib or _cabi.lib()
    quads, frames = QC.lists()
    pt, qt = QC.tables(QC.PAGES, quads, frames)
    _cabi.check(lib.dmx_edit_quads_prepare(pt, len(QC.PAGES), qt, QC.N, S_), "edit_quads_prepare", lib)
    return pt, qt, quads, frames


@pytest.fixture(scope="module")
def world():
    """random pages and the cases' prepared integers (from the closed form), computed once and only read afterwards"""
    rs = np.random.RandomState(20251020)
    pages = [rs.randint(0, 256, (h, w, 3), dtype=np.uint8) for h, w in QC.PAGES]
    quads, frames = QC.lists()
    qs = [QR.derive(c, f, S) for cs, fs in zip(quads, frames) for c, f in zip(cs, fs)]
    vae = (rs.standard_normal((QC.N, 3, S, S)) * 0.6).clip(-1.3, 1.3).astype(np.float32)
    for a in pages + [vae]:
        a.setflags(write=False)
    return dict(pages=pages, quads=quads, frames=frames, qs=qs, vae=vae)


def test_cases_cover_what_they_claim():
    names = [it[0] for _, it in QC.FLAT]
    assert QC.N == 9 and [len(i) for i in QC.ITEMS] == [4, 2, 3] and names[0] == "axis_copy" and names[-1] == "larger_than_frame"
    assert sum(w > 256 and w % 256 != 0 for _, w in QC.PAGES) == 2
    quads, frames = QC.lists()
    ang = lambda f: np.degrees(np.arctan2(f[4], f[3]))
    flat_f = [f for fs in frames for f in fs]
    assert [round(float(ang(f))) for f in flat_f] == [0, 7, 30, -15, 90, 4, 180, 3, 10]
    assert flat_f[4][3] == 0 and flat_f[6][4] == 0 and flat_f[6][3] < 0, "exactly 90 and 180 degrees"
    xs = [c[0] for c in quads[0][3]]
    assert min(xs) < 256 < max(xs), "skew_m15_tile_edge lies on both sides of the paste's 256-column tile"
    assert flat_f[5][2] > QC.PAGES[1][0], "overhang: the frame is larger than its page is high"


def test_prepare_fills_the_closed_form(world):
    """every integer dmx_edit_quads_prepare writes equals the closed form of csrc/prepost_quad.h recomputed in numpy float64, on both
    builds and at two sizes; the strips are packed in item order and the pages' blocks are the paged entries' blocks"""
    from diffute_amd import _cabi
    assert ctypes.sizeof(_cabi.EditQuad) == 44 * 4 + 8
    for elem in ("bf16", "fp16"):
        for S_ in (S, 512):
            pt, qt, quads, frames = _prepared(_cabi.lib(elem), S_)
            off = blocks = 0
            for b, (p, (name, c, _)) in enumerate(QC.FLAT):
                f = frames[p][b - pt[p].item_lo]
                want, got = QR.derive(c, f, S_), QR.from_table(qt[b])
                for k in QR.FIELDS:
                    assert got[k] == want[k], f"{name}: {k} = {got[k]}, the closed form gives {want[k]} (S = {S_}, {elem})"
                assert got["page"] == p and got["rect_off"] == off and got["rect_block_lo"] == blocks
                assert got["rect_blocks"] == want["rh"] * ((want["rw"] + 255) // 256)
                off += want["rw"] * want["rh"] * 3; blocks += got["rect_blocks"]
            assert [(pg.block_lo, pg.blocks) for pg in pt] == [(0, 300), (300, 97), (397, 140)]
    q = QR.derive(QC.box_quad(20, 20, 50, 32), (93, 83, 64, 1, 0), 64)
    assert q["fwd"] == [32768, 0, 0, 32768] and q["inv"] == [32768, 0, 0, 32768] and q["rect"] == [32768, 0, 0, 32768] and (q["rw"], q["rh"]) == (31, 13)
    q = QR.derive(QC.ITEMS[1][0][1], QC.ITEMS[1][0][2], 64)          # a quarter turn: the matrix is exact
    assert q["fwd"] == [0, -32768, 32768, 0] and (q["rw"], q["rh"]) == (61, 13)


def test_q16_map_is_the_affine_map_within_the_matrix_rounding(world):
    """X16 / 65536 against cx + s * (cos * p - sin * q) in float64.  The centre term is exact; a Q15 matrix entry is off by at most 1/2, and
    it multiplies the integer 2d + 1 - S: the two terms of a coordinate are off by at most (|2dx + 1 - S| + |2dy + 1 - S|) / 2 units of
    2^-16.  The bound is per pixel; the float64 evaluation of the exact map adds less than 1e-9."""
    for q, f in zip(world["qs"], [f for fs in world["frames"] for f in fs]):
        cx2, cy2, cs, ux, uy = f
        n = np.hypot(ux, uy)
        X16, Y16 = QR.frame_coords(q, S)
        py, px = np.meshgrid(2.0 * np.arange(S) + 1 - S, 2.0 * np.arange(S) + 1 - S, indexing="ij")
        s = cs / S
        X = cx2 / 2 + s * (ux / n * px - uy / n * py) / 2
        Y = cy2 / 2 + s * (uy / n * px + ux / n * py) / 2
        bound = (np.abs(px) + np.abs(py)) / 2 / 65536 + 1e-9
        assert (np.abs(X16 / 65536.0 - X) <= bound).all() and (np.abs(Y16 / 65536.0 - Y) <= bound).all()
        # ... and the inverse map undoes it: U16 of a page point, against the exact inverse, by the same reasoning on 2X - cx2, 2Y - cy2
        Yp, Xp = np.meshgrid(np.arange(0, 60, dtype=np.int64), np.arange(0, 90, dtype=np.int64), indexing="ij")
        U16, V16 = QR.crop_coords(q, S, Xp, Yp)
        qx, qy = 2.0 * Xp - cx2, 2.0 * Yp - cy2
        U = (S - 1) / 2 + (ux / n * qx + uy / n * qy) / s / 2
        V = (S - 1) / 2 + (-uy / n * qx + ux / n * qy) / s / 2
        bound = (np.abs(qx) + np.abs(qy)) / 2 / 65536 + 1e-9
        assert (np.abs(U16 / 65536.0 - U) <= bound).all() and (np.abs(V16 / 65536.0 - V) <= bound).all()


def _turned(world, p, faults=()):
    """page p with its items: (preprocess dicts, strips, paste) of the page as it is and turned by a quarter"""
    H, W = QC.PAGES[p]
    page, tp = world["pages"][p], QR.rot90_page(world["pages"][p])
    lo = sum(len(i) for i in QC.ITEMS[:p])
    res = []
    for pg, cs, fs in ((page, world["quads"][p], world["frames"][p]),
                       (tp, [QR.rot90_corners(c, W) for c in world["quads"][p]], [QR.rot90_frame(f, W) for f in world["frames"][p]])):
        qs = [QR.derive(c, f, S) for c, f in zip(cs, fs)]
        res.append(([QR.preprocess(pg, q, S, faults) for q in qs], [QR.rectify(pg, q, faults) for q in qs],
                    QR.paste_page(pg, qs, world["vae"][lo:lo + len(qs)], S, faults=faults)))
    return res


def _rot90_differences(world, p, faults=()):
    (pre, strips, paste), (tpre, tstrips, tpaste) = _turned(world, p, faults)
    d = sum(int(not np.array_equal(a[k], b[k])) for a, b in zip(pre, tpre) for k in ("image_u8", "masked_u8", "mask"))
    d += sum(int(not np.array_equal(a, b)) for a, b in zip(strips, tstrips))
    return d, int(not np.array_equal(np.rot90(paste["out"]), tpaste["out"])) + int(not np.array_equal(np.rot90(paste["pasted"]), tpaste["pasted"]))


@pytest.mark.parametrize("p", range(len(QC.PAGES)))
def test_restatement_is_invariant_under_a_quarter_turn(world, p):
    """a page turned by np.rot90 with its quads and frames turned along: the crops, masks and strips are THE SAME arrays, the pasted page
    is the turned pasted page - bit for bit (the maps are exact images of each other: csrc/prepost_quad.h)"""
    assert _rot90_differences(world, p) == (0, 0)


def test_exact_copies(world):
    from oracle import prepost as OP
    page = world["pages"][0]
    q = world["qs"][0]                                          # axis_copy: crop_scale = S, centred on a half-pixel
    pre = QR.preprocess(page, q, S)
    assert np.array_equal(pre["image_u8"], page[10:74, 15:79])
    full = OP.generate_mask((QC.PAGES[0][1], QC.PAGES[0][0]), (20, 20, 50, 32))
    assert np.array_equal(pre["mask"], full[10:74, 15:79]), "an axis-aligned quad is generate_mask's inclusive rectangle"
    assert np.array_equal(pre["masked_u8"], page[10:74, 15:79] * (1 - full[10:74, 15:79])[..., None])
    assert np.array_equal(QR.rectify(page, q), page[20:33, 20:51])
    Y, X = np.mgrid[0:150, 0:300]
    assert np.array_equal(QR.inside(q, X, Y), full.astype(bool))
    # the paste of the crop itself puts the page back: every pixel of the quad is on the crop, the weights are 1 and 0
    vae = pre["image"]
    got = QR.paste_page(np.zeros_like(page), [q], [vae], S)
    assert np.array_equal(got["pasted"], full.astype(bool)) and np.array_equal(got["out"][got["pasted"]], page[got["pasted"]])


FAULTS = ("transposed", "flip_v", "drop_half", "exclusive", "reversed", "first_wins", "two_pass", "truncated")


@pytest.mark.parametrize("fault", FAULTS)
def test_an_injected_fault_breaks_a_property(world, fault):
    """each deliberate mistake of tests/quad_restatement.py must show: in the quarter-turn invariance, in an exact-copy identity, or as a
    difference from the clean result on page 0 (whose items overlap)"""
    page, q = world["pages"][0], world["qs"][0]
    broken = []
    if _rot90_differences(world, 0, (fault,)) != (0, 0):
        broken.append("rot90")
    pre = QR.preprocess(page, q, S, (fault,))
    if not (np.array_equal(pre["image_u8"], page[10:74, 15:79]) and np.array_equal(QR.rectify(page, q, (fault,)), page[20:33, 20:51])):
        broken.append("copy")
    Y, X = np.mgrid[0:150, 0:300]
    if not np.array_equal(QR.inside(q, X, Y, (fault,)), (X >= 20) & (X <= 50) & (Y >= 20) & (Y <= 32)):
        broken.append("rectangle")
    clean, bad = QR.paste_page(page, world["qs"][:4], world["vae"][:4], S), QR.paste_page(page, world["qs"][:4], world["vae"][:4], S, faults=(fault,))
    if not np.array_equal(clean["out"], bad["out"]):
        broken.append("clean paste")
    assert broken, f"{fault}: nothing noticed it"
    want = {"two_pass": "rot90", "truncated": "rot90", "drop_half": "copy", "exclusive": "rectangle", "reversed": "rectangle",
            "first_wins": "clean paste", "transposed": "clean paste", "flip_v": "clean paste"}[fault]
    assert want in broken, f"{fault}: expected to break {want}, broke {broken}"


def _refused(lib, pt, P, qt, B, *words, S_=S):
    assert lib.dmx_edit_quads_prepare(pt, P, qt, B, S_) != 0, words
    msg = lib.dmx_last_error().decode()
    assert all(w in msg for w in words), msg


def test_every_refusal_by_index():
    from diffute_amd import _cabi
    lib = _cabi.lib()
    quads, frames = QC.lists()

    def bad(p, j, corners=None, frame=None, sizes=QC.PAGES):
        qs, fs = [list(q) for q in quads], [list(f) for f in frames]
        if corners is not None:
            qs[p][j] = corners
        if frame is not None:
            fs[p][j] = frame
        return QC.tables(sizes, qs, fs)

    good_f = frames[0][1]
    # the quad: counter-clockwise, a bow tie, a dent, no area (a line; a point), a corner outside ITS page but inside the larger page before it
    pt, qt = bad(0, 1, [(20, 20), (20, 32), (50, 32), (50, 20)])
    _refused(lib, pt, 3, qt, QC.N, "item 1", "clockwise")
    for corners, word in (([(20, 20), (50, 32), (50, 20), (20, 32)], "convex"), ([(20, 20), (50, 20), (30, 24), (20, 32)], "convex"),
                          ([(20, 20), (50, 20), (50, 20), (20, 20)], "no area"), ([(20, 20), (20, 20), (20, 20), (20, 20)], "no area")):
        pt, qt = bad(0, 2, corners)
        _refused(lib, pt, 3, qt, QC.N, "item 2", word)
    pt, qt = bad(1, 0, [(100, 10), (140, 10), (140, 30), (100, 30)])          # x = 140: inside the 300-wide page 0, outside the 131-wide page 1
    _refused(lib, pt, 3, qt, QC.N, "item 4", "corner 1", "outside")
    pt, qt = bad(2, 0, [(100, 50), (20, 50), (20, -1), (100, 30)])
    _refused(lib, pt, 3, qt, QC.N, "item 6", "corner 2", "outside")
    # the frame
    for frame, word in (((300, 150, 64, 0, 0), "(0, 0)"), ((300, 150, 0, 1, 0), "crop_scale"), ((300, 150, 65536, 1, 0), "crop_scale"),
                        ((600, 150, 64, 1, 0), "centre"), ((300, 299, 64, 1, 0), "centre"), ((-1, 150, 64, 1, 0), "centre"),
                        ((300, 150, 64, 131071, 0), "131070")):
        pt, qt = bad(0, 3, frame=frame)
        _refused(lib, pt, 3, qt, QC.N, "item 3", word)
    pt, qt = bad(0, 3, frame=(598, 298, 64, -131070, 131070))                  # the limits themselves pass
    _cabi.check(lib.dmx_edit_quads_prepare(pt, 3, qt, QC.N, S), "limits")
    # the page index, the item ranges, the counts, S
    pt, qt = QC.tables(QC.PAGES, quads, frames)
    qt[5].page = 0
    _refused(lib, pt, 3, qt, QC.N, "item 5", "page")
    for change, q in ((lambda pt: setattr(pt[1], "item_lo", 3), 1), (lambda pt: setattr(pt[1], "item_hi", 7), 2), (lambda pt: setattr(pt[2], "item_hi", 8), 2),
                      (lambda pt: setattr(pt[2], "item_hi", 10), 2), (lambda pt: setattr(pt[0], "item_lo", 1), 0), (lambda pt: setattr(pt[1], "item_hi", 4), 1)):
        pt, qt = QC.tables(QC.PAGES, quads, frames)
        change(pt)
        _refused(lib, pt, 3, qt, QC.N, f"page {q}")
    for sizes, q in (([(150, 300), (97, 131), (0, 260)], 2), ([(150, 65536), (97, 131), (70, 260)], 0), ([(150, 300), (65536, 131), (70, 260)], 1)):
        pt, qt = QC.tables(sizes, quads, frames)
        _refused(lib, pt, 3, qt, QC.N, f"page {q}", "size")
    pt, qt = QC.tables(QC.PAGES, quads, frames)
    _refused(lib, pt, 0, qt, QC.N, "pages")
    _refused(lib, pt, 65, qt, QC.N, "pages")
    _refused(lib, pt, 3, qt, 0, "items")
    _refused(lib, pt, 3, qt, 65, "items")
    _refused(lib, pt, 3, qt, QC.N, "S", S_=0)
    _refused(lib, pt, 3, qt, QC.N, "S", S_=65536)
    assert lib.dmx_edit_quads_prepare(None, 3, qt, QC.N, S) != 0 and lib.dmx_edit_quads_prepare(pt, 3, None, QC.N, S) != 0
    # 64 pages of one quad each pass
    pt, qt = QC.tables([(150, 300)] * 64, [[quads[0][1]]] * 64, [[good_f]] * 64)
    _cabi.check(lib.dmx_edit_quads_prepare(pt, 64, qt, 64, S), "64 pages")
    assert qt[63].rect_off == 63 * qt[0].rw * qt[0].rh * 3 and qt[63].page == 63


def test_launch_entries_refuse_a_table_spoiled_after_the_prepare():
    """the three entries check the HOST tables again and return before they launch: callable without a GPU.  Every call below is one
    that must be refused - the addresses are dummies."""
    from diffute_amd import _cabi
    lib = _cabi.lib()

    def entries(pt, qt, S_=S, total=1 << 40):
        """the three calls, unevaluated: only the ones a case expects to be refused are ever made"""
        return (lambda: lib.dmx_preprocess_quads(pt, ONE, 3, qt, ONE, QC.N, S_, ONE, ONE, ONE, ONE, None),
                lambda: lib.dmx_postprocess_paste_quads(ONE, S_, pt, ONE, 3, qt, ONE, QC.N, None),
                lambda: lib.dmx_rectify_quads(pt, ONE, 3, qt, ONE, QC.N, ONE, total, None))

    def spoiled(change, *words, calls=(0, 1, 2)):
        pt, qt, _, _ = _prepared()
        change(pt, qt)
        for call in calls:                                 # one at a time: each call leaves its own message
            assert entries(pt, qt)[call]() != 0, (call, words)
            msg = lib.dmx_last_error().decode()
            assert all(w in msg for w in words), (call, msg)

    def item(b, field, value, index=None):
        def f(pt, qt):
            if index is None:
                setattr(qt[b], field, value)
            else:
                getattr(qt[b], field)[index] = value
        return f
    spoiled(item(4, "x", 131, 1), "item 4", "corner 1")
    spoiled(item(2, "ex", 7, 0), "item 2", "derived")
    spoiled(item(3, "rect_off", 5), "item 3", "derived")
    spoiled(item(7, "rw", 2000), "item 7", "derived")
    spoiled(item(5, "page", 2), "item 5", "page")
    spoiled(item(6, "fwd", 1, 2), "item 6", "derived", calls=(0, 1))       # the rectify entry reads no frame
    spoiled(item(6, "crop_scale", 0), "item 6", "crop_scale", calls=(0, 1))
    spoiled(lambda pt, qt: setattr(pt[1], "W", 300), "page 1", "derived")
    spoiled(lambda pt, qt: setattr(pt[2], "block_lo", 396), "page 2", "derived")
    spoiled(lambda pt, qt: setattr(pt[0], "original", 0), "page 0", "null")
    spoiled(lambda pt, qt: setattr(pt[1], "out", 0), "page 1", calls=(1,))
    spoiled(lambda pt, qt: setattr(pt[1], "out", 64), "page 1", calls=(1,))
    pt, qt, _, _ = _prepared()
    assert entries(pt, qt, S_=100)[0]() != 0, "S must be a multiple of 8"
    assert entries(pt, qt, S_=128)[1]() != 0 and "derived" in lib.dmx_last_error().decode(), "a table prepared for another S"
    need = qt[QC.N - 1].rect_off + qt[QC.N - 1].rw * qt[QC.N - 1].rh * 3
    assert entries(pt, qt, total=need - 1)[2]() != 0 and "bytes" in lib.dmx_last_error().decode()


def test_frame_for_hand_computed():
    from diffute_amd import prepost
    # upright 30 x 12 line in the middle of a 1100 x 1300 page: u = (60, 0); the ladder gives 128; centre (35, 26) -> (70, 52) half-pixels,
    # moved right and down until the 128-pixel box touches the page's corner: 2 * 63.5 = 127
    assert prepost.frame_for(QC.box_quad(20, 20, 50, 32), 1100, 1300) == (127, 127, 128, 60, 0)
    assert prepost.frame_for(QC.box_quad(600, 500, 630, 512), 1100, 1300) == (1230, 1012, 128, 60, 0)
    # at the page's far corner: 2 * (1300 - 64) - 1 and 2 * (1100 - 64) - 1
    assert prepost.frame_for(QC.box_quad(1260, 1080, 1299, 1099), 1100, 1300) == (2471, 2071, 128, 78, 0)
    # a quarter turn, read top to bottom, 60 long and 12 high on the 97 x 131 page: the ladder's 128 is capped by the short side, 97; the
    # box is as high as the page (centred: 96) and fits in x between 96 and 2 * 131 - 1 - 97 = 164
    assert prepost.frame_for([(80, 10), (80, 70), (68, 70), (68, 10)], 97, 131) == (148, 96, 97, 0, 120)
    # a 3-4-5 direction: edges (80, 60), length 100, height 10 -> 128; the box's side is ceil(128 * 7 / 5) = 180 > 150 rows: centred in y
    q = [(100, 20), (180, 80), (174, 88), (94, 28)]
    assert prepost.frame_for(q, 150, 300) == (274, 149, 128, 160, 120)
    assert prepost.plan_quads([[q], [QC.box_quad(20, 20, 50, 32)]], [(150, 300), (1100, 1300)]) == [[(274, 149, 128, 160, 120)], [(127, 127, 128, 60, 0)]]
    with pytest.raises(ValueError):
        prepost.plan_quads([[q]], [(150, 300), (97, 131)])
    with pytest.raises(ValueError):
        prepost.frame_for([(0, 0), (1, 1), (2, 2)], 10, 10)
    # whatever the quad, the planned frame is one the C side accepts
    from diffute_amd import _cabi
    quads, frames = QC.lists()
    pt, qt = QC.tables(QC.PAGES, quads, [[prepost.frame_for(c, *QC.PAGES[p]) for c in cs] for p, cs in enumerate(quads)])
    _cabi.check(_cabi.lib().dmx_edit_quads_prepare(pt, 3, qt, QC.N, S), "planned frames")


def test_quad_functions_check_their_lists_first_and_refuse_host_tensors():
    import diffute_amd as D
    from diffute_amd import prepost
    img = torch.zeros(64, 80, 3, dtype=torch.uint8)
    quad, frame = [QC.box_quad(4, 4, 30, 12)], [(40, 30, 32, 1, 0)]
    calls = {"pre": lambda imgs, q, f: prepost.preprocess_quads(imgs, q, f, size=16),
             "post": lambda imgs, q, f: prepost.postprocess_quads(torch.zeros(1, 3, 16, 16), imgs, q, f),
             "rectify": lambda imgs, q, f: prepost.rectify_quads(imgs, q)}
    for name, fn in calls.items():
        with pytest.raises(ValueError):
            fn([], [], [])
        with pytest.raises(ValueError):
            fn([img] * 65, [quad] * 65, [frame] * 65)
        with pytest.raises(ValueError):
            fn([img] * 2, [quad * 33] * 2, [frame * 33] * 2)
        with pytest.raises(ValueError):
            fn([img] * 2, [quad], [frame] * 2)
        with pytest.raises(ValueError, match="page 1"):
            fn([img] * 2, [quad, []], [frame, []])
        with pytest.raises(ValueError):
            fn([img], [[[(4, 4), (30, 4), (30, 12)]]], [frame])              # three corners
        with pytest.raises(TypeError):
            fn([img], [quad], [frame])                                       # host tensors: no CPU fallback
    with pytest.raises(ValueError, match="page 1"):
        prepost.preprocess_quads([img] * 2, [quad, quad], [frame, frame * 2])
    with pytest.raises(ValueError):
        prepost.preprocess_quads([img], [quad], [[(40, 30, 32, 1)]])
    # edit_quads: the models are never reached
    ctx = torch.zeros(2, 77, 128)

    def run(exc, images=(img, img), quads=(quad, quad), ctx=ctx, **kw):
        with pytest.raises(exc):
            D.edit_quads(None, None, None, list(images), list(quads), ctx, 3, size=64, **kw)
    run(ValueError, batch_size=0)
    run(ValueError, quads=(quad,))
    run(ValueError, ctx=ctx[:1])
    run(ValueError, frames=[frame])
    run(ValueError, frames=[frame, frame * 2])
    run(ValueError, texts=["a", "b"])                                        # both contexts given
    run(TypeError, images=(img, torch.zeros(64, 80, dtype=torch.uint8)))
    run(TypeError)                                                           # every list is fine: the host pages are refused
    assert "edit_quads" in D.__all__ and callable(D.edit_quads)
    for name in ("frame_for", "plan_quads", "preprocess_quads", "postprocess_quads", "rectify_quads"):
        assert callable(getattr(D.prepost, name))
    for name in ("dmx_edit_quads_prepare", "dmx_preprocess_quads", "dmx_postprocess_paste_quads", "dmx_rectify_quads"):
        assert name in _cabi_symbols()


def _cabi_symbols():
    from diffute_amd import _cabi
    return _cabi.exported_symbols()
