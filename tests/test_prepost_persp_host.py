"""The host half of the projective frame for quadrilateral regions (csrc/prepost_persp.h, prepost.persp_frame_for / plan_quads(perspective=True),
the C-ABI's host-only dmx_edit_quads_persp_prepare): every prepared integer against the Python-int restatement, the Q16 maps against the
exact rational homographies in fractions.Fraction, the properties of the numpy restatement the GPU tests compare against
(tests/persp_restatement.py) - no 64-bit wrap, the strip's corners, the mask as a rectangle, invariance under a quarter turn, the
exact-copy and affine cases - with six injected faults that must break them, every refusal by index, and the planner.  Nothing here needs
a GPU."""
import ctypes
from fractions import Fraction

import numpy as np
import pytest
import torch

import persp_cases as PC
import persp_restatement as PR
import quad_restatement as QR

S = PC.S
ONE = ctypes.c_void_p(64)            # a dummy device address: the refusals return before any launch
# csrc/prepost_persp.h: the coefficients' rounding moves a coordinate by < 2^-3 (1 + 2^-18) units of 2^-16, the final rdiv by <= 1/2
BOUND = Fraction(1, 2) + Fraction(1, 8) * (1 + Fraction(1, 1 << 18))


def _prepared(lib=None, S_=S, quads=None, frames=None, sizes=PC.PAGES):
    from diffute_amd import _cabi
    lib = lib or _cabi.lib()
    if quads is None:
        quads, frames = PC.lists()
    pt, qt, xt = PC.tables(sizes, quads, frames)
    B = sum(len(q) for q in quads)
    _cabi.check(lib.dmx_edit_quads_prepare(pt, len(sizes), qt, B, S_), "edit_quads_prepare", lib)
    _cabi.check(lib.dmx_edit_quads_persp_prepare(pt, len(sizes), qt, xt, B, S_), "edit_quads_persp_prepare", lib)
    return pt, qt, xt


@pytest.fixture(scope="module")
def world():
    """random pages, the cases' prepared integers (from the prepare entries) and decoder outputs, computed once and only read afterwards"""
    rs = np.random.RandomState(20261020)
    pages = [rs.randint(0, 256, (h, w, 3), dtype=np.uint8) for h, w in PC.PAGES]
    quads, frames = PC.lists()
    pt, qt, xt = _prepared()
    qs, pms = [QR.from_table(q) for q in qt], [PR.from_table(x) for x in xt]
    vae = (rs.standard_normal((PC.N, 3, S, S)) * 0.6).clip(-1.3, 1.3).astype(np.float32)
    for a in pages + [vae]:
        a.setflags(write=False)
    return dict(pages=pages, quads=quads, frames=frames, qs=qs, pms=pms, vae=vae)


def _ratio(m, g):
    t = m["t"]
    D = [t[6] * p + t[7] * q + t[8] for p, q in ((-g, -g), (g, -g), (g, g), (-g, g))]
    return Fraction(max(D), min(D))


def test_cases_cover_what_they_claim(world):
    names = [it[0] for _, it in PC.FLAT]
    assert PC.N == 9 and [len(i) for i in PC.ITEMS] == [5, 2, 2]
    assert names == ["trap_right", "keystone_down", "general_tile_edge", "axis_copy", "overlap", "rot90_persp", "overhang", "parallelogram", "thin"]
    ratios = {n: float(_ratio(pm["crop"], S - 1)) for n, pm in zip(names, world["pms"])}
    want = dict(trap_right=1.99, keystone_down=2.08, general_tile_edge=1.42, axis_copy=1.0, rot90_persp=2.04, overhang=1.78, parallelogram=1.0, thin=2.0)
    for n, r in want.items():
        assert abs(ratios[n] - r) < 0.006, (n, ratios[n])
    assert max(ratios.values()) <= 2.08, "the cap of 4 leaves no case out"
    xs = [c[0] for c in world["quads"][0][2]]
    assert min(xs) < 256 < max(xs), "general_tile_edge lies on both sides of the paste's 256-column tile"
    Y, X = np.mgrid[0:150, 0:300]
    both = QR.inside(world["qs"][0], X, Y) & QR.inside(world["qs"][4], X, Y)
    assert both.sum() > 50, "overlap overlaps trap_right"
    X16, Y16 = PR.coords(world["pms"][6]["crop"], *PR.crop_grid(S))
    assert (Y16 >> 16).max() >= PC.PAGES[1][0] and (X16 >> 16).min() < 0, "overhang: the window has clamped taps"
    assert world["pms"][3]["crop"]["c16"] == [(46 << 16) + 32768, (41 << 16) + 32768], "axis_copy is centred on a half-pixel"


def test_prepare_fills_what_the_restatement_derives():
    """every integer dmx_edit_quads_persp_prepare writes equals the Python-int host half of the restatement, on both builds and at two
    sizes; the restatement's own acceptance agrees; S = 0 fills the strip maps alone"""
    from diffute_amd import _cabi
    assert ctypes.sizeof(_cabi.PerspMap) == 11 * 8 and ctypes.sizeof(_cabi.QuadPersp) == 6 * 4 + 3 * 88
    for elem in ("bf16", "fp16"):
        for S_ in (S, 512):
            pt, qt, xt = _prepared(_cabi.lib(elem), S_)
            for b, (p, (name, c, cs, ctr)) in enumerate(PC.FLAT):
                rw, rh = qt[b].rw, qt[b].rh
                assert (rw, rh) == PR.strip_size(c)
                want, got = PR.host_maps(c, rw, rh, PC.frame_of(c, cs, ctr), S_), PR.from_table(xt[b])
                assert got == want, f"{name}: the table differs from the restatement (S = {S_}, {elem})"
                PR.accept(want, c, rw, rh, S_)
                assert want["crop"]["t"][8] == want["paste"]["t"][8] == want["strip"]["t"][8] == 1 << PR.Q
    lib = _cabi.lib()
    quads, frames = PC.lists()
    pt, qt, xt = PC.tables(PC.PAGES, quads, [[None] * len(q) for q in quads])
    _cabi.check(lib.dmx_edit_quads_prepare(pt, 3, qt, PC.N, 8), "edit_quads_prepare")
    _cabi.check(lib.dmx_edit_quads_persp_prepare(pt, 3, qt, xt, PC.N, 0), "strips only")
    full = _prepared()[2]
    for b in range(PC.N):
        got = PR.from_table(xt[b])
        assert got["strip"] == PR.from_table(full[b])["strip"] and got["crop"]["t"] == [0] * 9 and got["paste"]["t"] == [0] * 9


def _grids(q, pm):
    """the three maps' evaluation points of one item: name -> (p, q) int64 arrays"""
    H, W = PC.PAGES[q["page"]]
    Y, X = np.mgrid[0:H, 0:W]
    sel = QR.inside(q, X, Y)
    return {"crop": PR.crop_grid(S), "paste": (2 * X[sel].astype(np.int64) - pm["cx2"], 2 * Y[sel].astype(np.int64) - pm["cy2"]),
            "strip": PR.strip_grid(q["rw"], q["rh"])}


def _worst_error(c, q, pm, frame, faults=(), maps=PR.MAP_NAMES):
    """the largest |coordinate - exact coordinate * 2^16| of one item over the points its kernels evaluate, per map, as Fractions.  The
    exact maps are taken about the (cx2, cy2) of the maps under test, so a wrong map cannot hide behind its own centre."""
    rw, rh = q["rw"], q["rh"]
    exact = dict(zip(PR.MAP_NAMES, PR.exact_matrices(c, rw, rh, frame, S, pm["cx2"], pm["cy2"])))
    worst = {}
    for name in maps:
        p, g = (np.asarray(a).reshape(-1) for a in _grids(q, pm)[name])
        A16, B16 = (np.asarray(a).reshape(-1) for a in PR.coords(pm[name], p, g, faults=faults))
        M = exact[name]
        w = Fraction(0)
        for pi, qi, a, b in zip(p.tolist(), g.tolist(), A16.tolist(), B16.tolist()):
            den = M[2][0] * pi + M[2][1] * qi + M[2][2]
            ex = Fraction((M[0][0] * pi + M[0][1] * qi + M[0][2]) << 16, den)
            ey = Fraction((M[1][0] * pi + M[1][1] * qi + M[1][2]) << 16, den)
            w = max(w, abs(a - ex), abs(b - ey))
        worst[name] = w
    return worst


def test_q16_maps_are_the_exact_homographies_within_the_budget(world):
    """Every X16, Y16 of every crop pixel, every U16, V16 of every page pixel inside a quad and every strip coordinate, against the
    exact rational map in fractions.Fraction.

    The bound, from the budget of csrc/prepost_persp.h.  The table's t are the exact coefficients (scaled so that t8 = 2^43) rounded to
    integers: each is off by at most 1/2, so n by at most (gx + gy + 1) / 2 =: e and D by less than e.  With r = n / D the exact ratio's
    magnitude |r| <= (A + e) / (min D - e), the rounded ratio differs from it by (dn - r dD) / D, at most e (1 + |r|) / min D.  The host
    accepts a map only if ((gx + gy + 1)(min D + A)) << 18 <= (min D)^2, which makes e / min D <= 2^-19 and
    2^16 e (1 + |r|) / min D <= 2^15 (gx + gy + 1)(min D + A) / (min D)^2 * (1 + 2^-18) <= 2^-3 (1 + 2^-18).  The centre's rounding
    costs nothing: t2 carries its residual.  The final rdiv adds at most 1/2: BOUND = 1/2 + 1/8 (1 + 2^-18) < 0.6251 units of 2^-16.
    Measured over the nine cases at S = 64: 0.499989 (general_tile_edge's crop; every case but the exact copy lies between 0.476 and 0.49999):
    the coordinates are the correctly rounded exact ones, the coefficients' share stays far below the 1/8 the budget allows."""
    worst = Fraction(0)
    for (p, (name, c, cs, ctr)), q, pm in zip(PC.FLAT, world["qs"], world["pms"]):
        w = _worst_error(c, q, pm, PC.frame_of(c, cs, ctr))
        print(f"{name}: worst error crop {float(w['crop']):.6f} paste {float(w['paste']):.6f} strip {float(w['strip']):.6f} of 2^-16, bound {float(BOUND):.6f}")
        assert max(w.values()) <= BOUND, name
        worst = max(worst, *w.values())
    assert BOUND < 1 and worst <= Fraction(1, 2) + Fraction(1, 1000), float(worst)


def _wraps(world, faults=()):
    """items whose int64 evaluation differs from the same arithmetic in Python ints"""
    bad = 0
    for q, pm in zip(world["qs"], world["pms"]):
        for name, (p, g) in _grids(q, pm).items():
            a = PR.coords(pm[name], p, g, faults=faults)
            b = PR.coords(pm[name], p, g, ints=object, faults=faults)
            bad += int(not all(np.array_equal(np.asarray(x).astype(object), y) for x, y in zip(a, b)))
    return bad


def test_nothing_leaves_64_bits(world):
    """the kernels' half re-run in Python ints gives the same integers, map for map; the budget's terms hold for every table entry"""
    assert _wraps(world) == 0
    for pm in world["pms"]:
        for name in PR.MAP_NAMES:
            assert all(abs(v) < 1 << 62 for v in pm[name]["t"] + pm[name]["c16"])


def _corner_errors(c, q, pm, faults=()):
    rw, rh = q["rw"], q["rh"]
    pts = [(1 - rw, 1 - rh), (rw - 1, 1 - rh), (rw - 1, rh - 1), (1 - rw, rh - 1)]
    X16, Y16 = PR.coords(pm["strip"], [p for p, _ in pts], [g for _, g in pts], faults=faults)
    return max(max(abs(int(a) - (x << 16)), abs(int(b) - (y << 16))) for a, b, (x, y) in zip(X16, Y16, c))


def test_the_strips_corners_are_the_quads_corners(world):
    for (p, (name, c, _, _)), q, pm in zip(PC.FLAT, world["qs"], world["pms"]):
        assert _corner_errors(c, q, pm) <= BOUND, name


def _fills_its_box(mask):
    """the ones fill their own bounding box apart from its outermost ring"""
    rows, cols = np.nonzero(mask.any(1))[0], np.nonzero(mask.any(0))[0]
    r0, r1, c0, c1 = rows[0], rows[-1], cols[0], cols[-1]
    assert r1 - r0 >= 4 and c1 - c0 >= 8
    return bool(mask[r0 + 1:r1, c0 + 1:c1].all())


@pytest.mark.parametrize("b", [0, 1, 2, 5])
def test_the_mask_is_a_rectangle(world, b):
    """what the feature is for: through the projective frame the network sees the quad as an upright rectangle - the text without
    keystone -, through the similarity frame of the same trapezoid it does not"""
    from diffute_amd import prepost
    p, (name, c, cs, ctr) = PC.FLAT[b]
    page = world["pages"][p]
    pre = PR.preprocess(page, world["qs"][b], world["pms"][b], S)
    assert set(np.unique(pre["mask"])) == {0, 1} and _fills_its_box(pre["mask"]), name
    sim = QR.derive(c, prepost.frame_for(c, *PC.PAGES[p]), S)
    assert not _fills_its_box(QR.preprocess(page, sim, S)["mask"]), f"{name}: the similarity frame already shows a rectangle"


def _turned(world, p, faults=()):
    """page p with its items, as it is and turned by a quarter: (crops, strips, paste) each, from the restatement alone.  The frames
    live in strip space and do not turn."""
    H, W = PC.PAGES[p]
    lo = sum(len(i) for i in PC.ITEMS[:p])
    res = []
    for pg, cs in ((world["pages"][p], world["quads"][p]), (QR.rot90_page(world["pages"][p]), [QR.rot90_corners(c, W) for c in world["quads"][p]])):
        qs = [QR.derive(c, (0, 0, 1, 1, 0), 1) for c in cs]
        pms = [PR.host_maps(c, q["rw"], q["rh"], f, S, faults) for c, q, f in zip(cs, qs, world["frames"][p])]
        res.append(([PR.preprocess(pg, q, pm, S, faults=faults) for q, pm in zip(qs, pms)], [PR.rectify(pg, q, pm, faults=faults) for q, pm in zip(qs, pms)],
                    PR.paste_page(pg, qs, pms, world["vae"][lo:lo + len(qs)], S, faults=faults)))
    return res


def _rot90_differences(world, p, faults=()):
    (pre, strips, paste), (tpre, tstrips, tpaste) = _turned(world, p, faults)
    d = sum(int(not np.array_equal(a[k], b[k])) for a, b in zip(pre, tpre) for k in ("image_u8", "masked_u8", "mask"))
    d += sum(int(not np.array_equal(a, b)) for a, b in zip(strips, tstrips))
    return d, int(not np.array_equal(np.rot90(paste["out"]), tpaste["out"])) + int(not np.array_equal(np.rot90(paste["pasted"]), tpaste["pasted"]))


@pytest.mark.parametrize("p", range(len(PC.PAGES)))
def test_restatement_is_invariant_under_a_quarter_turn(world, p):
    """a page turned by np.rot90 with its quads turned along: the crops, masks and strips are THE SAME arrays and the pasted page is the
    turned pasted page, bit for bit - rdiv commutes with negation, on the host and in the two-step division"""
    assert _rot90_differences(world, p) == (0, 0)


def test_degenerate_frames(world):
    page, q, pm = world["pages"][0], world["qs"][3], world["pms"][3]                 # axis_copy: crop_scale = S, centred on a half-pixel
    X16, Y16 = PR.coords(pm["crop"], *PR.crop_grid(S))
    dy, dx = np.mgrid[0:S, 0:S]
    assert np.array_equal(X16, (15 + dx).astype(np.int64) << 16) and np.array_equal(Y16, (10 + dy).astype(np.int64) << 16)
    pre = PR.preprocess(page, q, pm, S)
    assert np.array_equal(pre["image_u8"], page[10:74, 15:79])
    assert np.array_equal(PR.rectify(page, q, pm), page[20:33, 20:51])
    box = np.zeros((150, 300), bool)
    box[20:33, 20:51] = True
    assert np.array_equal(pre["mask"], box[10:74, 15:79].astype(np.uint8))
    got = PR.paste_page(np.zeros_like(page), [q], [pm], [pre["image"]], S)       # the paste of the crop itself puts the page back
    assert np.array_equal(got["pasted"], box) and np.array_equal(got["out"][box], page[box])
    for name in PR.MAP_NAMES:                                                    # parallelogram: affine, the denominator is constant
        t = world["pms"][7][name]["t"]
        assert t[6] == 0 and t[7] == 0 and t[8] == 1 << PR.Q
    assert any(world["pms"][0][n]["t"][6] != 0 for n in PR.MAP_NAMES)


FAULTS = {"floor": "rot90", "unrounded_centre": "accuracy", "u_over_rw": "corners", "transposed_adjugate": "accuracy", "cap_ignored": "cap",
          "one_step": "wrap"}


@pytest.mark.parametrize("fault", sorted(FAULTS))
def test_an_injected_fault_breaks_a_property(world, fault):
    """each deliberate mistake of tests/persp_restatement.py must show in at least one of the checks above - and in the one it is aimed at"""
    f = (fault,)
    p, (name, c, cs, ctr) = PC.FLAT[0]                                           # trap_right
    frame, q = PC.frame_of(c, cs, ctr), world["qs"][0]
    broken = []
    pm = PR.host_maps(c, q["rw"], q["rh"], frame, S, f)
    if max(_worst_error(c, q, pm, frame, f).values()) > BOUND:
        broken.append("accuracy")
    if _corner_errors(c, q, pm, f) > BOUND:
        broken.append("corners")
    if _rot90_differences(world, 1, f) != (0, 0):
        broken.append("rot90")
    if _wraps(world, f):
        broken.append("wrap")
    rw, rh = PR.strip_size(PC.STEEP_QUAD)                                        # refused for the cap alone
    try:
        PR.accept(PR.host_maps(PC.STEEP_QUAD, rw, rh, PC.frame_of(PC.STEEP_QUAD, 512), S, f), PC.STEEP_QUAD, rw, rh, S, f)
        broken.append("cap")
    except PR.Refused:
        pass
    assert FAULTS[fault] in broken, f"{fault}: expected to break {FAULTS[fault]}, broke {broken}"


def _refused(lib, tabs, P, B, *words, S_=S):
    pt, qt, xt = tabs
    assert lib.dmx_edit_quads_persp_prepare(pt, P, qt, xt, B, S_) != 0, words
    msg = lib.dmx_last_error().decode()
    assert all(w in msg for w in words), msg


def test_every_refusal_by_index():
    from diffute_amd import _cabi
    lib = _cabi.lib()
    quads, frames = PC.lists()

    def bad(p, j, corners=None, frame=None):
        qs, fs = [list(q) for q in quads], [list(f) for f in frames]
        if corners is not None:
            qs[p][j] = corners
            fs[p][j] = PC.frame_of(corners, 64)
        if frame is not None:
            fs[p][j] = frame
        pt, qt, xt = PC.tables(PC.PAGES, qs, fs)
        _cabi.check(lib.dmx_edit_quads_prepare(pt, 3, qt, PC.N, S), "edit_quads_prepare")
        return pt, qt, xt

    H = PC.HORIZON_QUAD
    _refused(lib, bad(0, 1, H, PC.frame_of(H, 240)), 3, PC.N, "item 1", "crop window", "horizon")
    _refused(lib, bad(0, 1, H, PC.frame_of(H, 150)), 3, PC.N, "item 1", "crop window", "cap")
    rw, rh = PR.strip_size(H)
    r = _ratio(PR.host_maps(H, rw, rh, PC.frame_of(H, 150), S)["crop"], S - 1)
    assert 4 < r < 8, "a window with the ratio between 4 and infinity"
    _refused(lib, bad(0, 1, H, PC.frame_of(H, 64)), 3, PC.N, "item 1", "strip", "cap")          # the quad's own strip is beyond the cap
    _refused(lib, bad(2, 0, PC.FLAT_STRIP_QUAD), 3, PC.N, "item 7", "thinner than 2")
    assert PR.strip_size(PC.FLAT_STRIP_QUAD)[1] == 1
    pt, qt, xt = PC.tables(PC.PAGES, quads, [frames[0], [frames[1][0], None], frames[2]])
    _cabi.check(lib.dmx_edit_quads_prepare(pt, 3, qt, PC.N, S), "edit_quads_prepare")
    _refused(lib, (pt, qt, xt), 3, PC.N, "item 6", "no projective frame")
    for frame, word in (((10, 10, -1), "crop_scale"), ((10, 10, 65536), "crop_scale"), (((1 << 20) + 1, 10, 64), "centre"), ((10, -(1 << 20) - 1, 64), "centre")):
        _refused(lib, bad(1, 0, frame=frame), 3, PC.N, "item 5", word)
    # a window so small that the quad's far corners leave the paste map's budget; a window the page -> crop map turns inside out
    _refused(lib, bad(0, 0, frame=(-4000, 34, 8)), 3, PC.N, "item 0")
    # what the quad prepare refuses is refused here too: tables it did not prepare, a spoiled quad, the counts, S
    pt, qt, xt = PC.tables(PC.PAGES, quads, frames)
    _refused(lib, (pt, qt, xt), 3, PC.N, "derived")
    pt, qt, xt = bad(0, 0)
    qt[4].x[1] = 300
    _refused(lib, (pt, qt, xt), 3, PC.N, "item 4", "corner 1")
    pt, qt, xt = bad(0, 0)
    _refused(lib, (pt, qt, xt), 0, PC.N, "pages")
    _refused(lib, (pt, qt, xt), 3, 65, "items")
    _refused(lib, (pt, qt, xt), 3, PC.N, "S", S_=-1)
    _refused(lib, (pt, qt, xt), 3, PC.N, "S", S_=65536)
    assert lib.dmx_edit_quads_persp_prepare(pt, 3, qt, None, PC.N, S) != 0 and "null" in lib.dmx_last_error().decode()
    # a geometry whose exact arithmetic would leave 126 bits is refused, not computed wrongly
    big = [(0, 0), (65000, 100), (65000, 60000), (10, 65000)]
    pt, qt, xt = PC.tables([(65535, 65535)], [[big]], [[PC.frame_of(big, 65535)]])
    _cabi.check(lib.dmx_edit_quads_prepare(pt, 1, qt, 1, 512), "edit_quads_prepare")
    _refused(lib, (pt, qt, xt), 1, 1, "item 0", S_=512)
    # the benchmark's scale passes: a 700-pixel keystoned line on a 1100 x 1300 page at S = 512
    line = [(100, 500), (800, 520), (800, 568), (100, 580)]
    pt, qt, xt = PC.tables([(1100, 1300)], [[line]], [[PC.frame_of(line, 1024)]])
    _cabi.check(lib.dmx_edit_quads_prepare(pt, 1, qt, 1, 512), "edit_quads_prepare")
    _cabi.check(lib.dmx_edit_quads_persp_prepare(pt, 1, qt, xt, 1, 512), "the benchmark's scale")
    want = PR.host_maps(line, qt[0].rw, qt[0].rh, PC.frame_of(line, 1024), 512)
    assert PR.from_table(xt[0]) == want
    t = want["crop"]["t"]
    assert abs(t[0]) * 511 + abs(t[1]) * 511 + abs(t[2]) < 1 << 53


def test_launch_entries_refuse_a_table_spoiled_after_the_prepare():
    """the three entries check the HOST tables again and return before they launch: callable without a GPU.  Every call below is one
    that must be refused - the addresses are dummies."""
    from diffute_amd import _cabi
    lib = _cabi.lib()

    def entries(pt, qt, xt, S_=S, total=1 << 40):
        return (lambda: lib.dmx_preprocess_quads_persp(pt, ONE, 3, qt, ONE, xt, ONE, PC.N, S_, ONE, ONE, ONE, ONE, None),
                lambda: lib.dmx_postprocess_paste_quads_persp(ONE, S_, pt, ONE, 3, qt, ONE, xt, ONE, PC.N, None),
                lambda: lib.dmx_rectify_quads_persp(pt, ONE, 3, qt, ONE, xt, ONE, PC.N, ONE, total, None))

    def spoiled(change, *words, calls=(0, 1, 2)):
        pt, qt, xt = _prepared()
        change(pt, qt, xt)
        for call in calls:                                 # one at a time: each call leaves its own message
            assert entries(pt, qt, xt)[call]() != 0, (call, words)
            msg = lib.dmx_last_error().decode()
            assert all(w in msg for w in words), (call, msg)

    def coef(b, name, k, v):
        def f(pt, qt, xt):
            getattr(xt[b], name).t[k] = v
        return f
    spoiled(coef(2, "crop", 0, 1), "item 2", "derived", calls=(0, 1))
    spoiled(coef(5, "paste", 8, 1 << 40), "item 5", "derived", calls=(0, 1))
    spoiled(coef(7, "strip", 6, 12345), "item 7", "derived")
    spoiled(lambda pt, qt, xt: setattr(xt[1], "cx2", 0), "item 1", "derived", calls=(0, 1))
    spoiled(lambda pt, qt, xt: setattr(xt[8], "crop_scale", 0), "item 8", "no projective frame", calls=(0, 1))
    spoiled(lambda pt, qt, xt: setattr(xt[4], "crop_scale", 99), "item 4", "derived", calls=(0, 1))
    spoiled(lambda pt, qt, xt: qt[4].x.__setitem__(1, 300), "item 4", "corner 1")
    spoiled(lambda pt, qt, xt: setattr(qt[3], "rw", 2000), "item 3", "derived")
    spoiled(lambda pt, qt, xt: setattr(pt[1], "W", 300), "page 1", "derived")
    spoiled(lambda pt, qt, xt: setattr(pt[0], "original", 0), "page 0", "null")
    spoiled(lambda pt, qt, xt: setattr(pt[1], "out", 0), "page 1", calls=(1,))
    pt, qt, xt = _prepared()
    assert entries(pt, qt, xt, S_=100)[0]() != 0, "S must be a multiple of 8"
    assert entries(pt, qt, xt, S_=128)[1]() != 0 and "derived" in lib.dmx_last_error().decode(), "a table prepared for another S"
    need = qt[PC.N - 1].rect_off + qt[PC.N - 1].rw * qt[PC.N - 1].rh * 3
    assert entries(pt, qt, xt, total=need - 1)[2]() != 0 and "bytes" in lib.dmx_last_error().decode()
    for call in range(3):
        assert (entries(pt, qt, None)[call])() != 0


def test_the_planner_steps_down_the_ladder():
    from diffute_amd import prepost
    # an upright 30 x 12 box in the middle of a 1100 x 1300 page: strip 31 x 13, the ladder's 128, centred on the strip
    assert prepost.persp_frame_for(PC.box_quad(600, 500, 630, 512), 1100, 1300) == (30, 12, 128)
    assert prepost.strip_size(PC.box_quad(600, 500, 630, 512)) == (31, 13)
    for _, (name, c, _, _) in PC.FLAT:
        assert prepost.strip_size(c) == PR.strip_size(c), name
    # strongly foreshortened: left edge 120, right edge 45.  The strip is 301 x 83, 6 * 83 = 498 < 512 -> the ladder's 512, over which the
    # denominator changes by more than 4x; the next rung that is longer than the strip, 384, is accepted
    steep = PC.STEEP_QUAD
    assert prepost.strip_size(steep) == (301, 83)
    assert prepost.crop_scale_for((0, 0, 301, 83), 1100, 1300) == 512
    assert "cap" in prepost.persp_frame_accepted(steep, 1100, 1300, (300, 82, 512))
    assert prepost.persp_frame_accepted(steep, 1100, 1300, (300, 82, 384)) is None
    assert prepost.persp_frame_for(steep, 1100, 1300) == (300, 82, 384)
    assert prepost.plan_quads([[steep], [PC.box_quad(600, 500, 630, 512)]], [(1100, 1300)] * 2, perspective=True) == [[(300, 82, 384)], [(30, 12, 128)]]
    assert prepost.plan_quads([[steep]], [(1100, 1300)]) == [[prepost.frame_for(steep, 1100, 1300)]], "perspective=False plans what it always planned"
    # nothing fits: the quad's own strip is beyond the cap, whatever the window
    with pytest.raises(ValueError, match=r"\(20, 10\)|\[20, 10\]"):
        prepost.persp_frame_for(PC.HORIZON_QUAD, 150, 300, size=S)
    with pytest.raises(ValueError):
        prepost.plan_quads([[steep]], [(1100, 1300), (97, 131)], perspective=True)
    # whatever the case, the planned frame is one the C side accepts - and the same on every call
    for p, (name, c, _, _) in PC.FLAT:
        f = prepost.persp_frame_for(c, *PC.PAGES[p], size=S)
        assert f[:2] == (PR.strip_size(c)[0] - 1, PR.strip_size(c)[1] - 1) and prepost.persp_frame_accepted(c, *PC.PAGES[p], f, S) is None, name
        assert f == prepost.persp_frame_for(c, *PC.PAGES[p], size=S)


def test_quad_functions_check_projective_frames_first_and_refuse_host_tensors():
    import diffute_amd as D
    from diffute_amd import prepost, _cabi
    img = torch.zeros(64, 80, 3, dtype=torch.uint8)
    quad, frame = [PC.box_quad(4, 4, 30, 12)], [(26, 8, 32)]
    calls = {"pre": lambda imgs, q, f: prepost.preprocess_quads(imgs, q, f, size=16, perspective=True),
             "post": lambda imgs, q, f: prepost.postprocess_quads(torch.zeros(1, 3, 16, 16), imgs, q, f, perspective=True),
             "rectify": lambda imgs, q, f: prepost.rectify_quads(imgs, q, perspective=True)}
    for name, fn in calls.items():
        with pytest.raises(ValueError):
            fn([], [], [])
        with pytest.raises(ValueError, match="page 1"):
            fn([img] * 2, [quad, []], [frame, []])
        with pytest.raises(TypeError):
            fn([img], [quad], [frame])                                       # host tensors: no CPU fallback
    for fn in (calls["pre"], calls["post"]):
        with pytest.raises(ValueError, match="projective"):
            fn([img], [quad], [[(40, 30, 32, 1, 0)]])                         # a similarity frame where a projective one is expected
        with pytest.raises(ValueError, match="page 0: quad 1"):
            fn([img], [quad * 2], [[frame[0], None]])                         # an item whose projective frame is missing
    with pytest.raises(ValueError):
        prepost.preprocess_quads([img], [quad], [frame])                      # ... and the other way round
    ctx = torch.zeros(2, 77, 128)

    def run(exc, images=(img, img), quads=(quad, quad), ctx=ctx, **kw):
        with pytest.raises(exc):
            D.edit_quads(None, None, None, list(images), list(quads), ctx, 3, size=64, perspective=True, **kw)
    run(ValueError, batch_size=0)
    run(ValueError, frames=[frame])
    run(ValueError, texts=["a", "b"])
    run(TypeError)                                                           # every list is fine and the frames are planned: the host pages are refused
    run(TypeError, frames=[frame, frame])
    for name in ("persp_frame_for", "persp_frame_accepted", "strip_size"):
        assert callable(getattr(prepost, name))
    for name in ("dmx_edit_quads_persp_prepare", "dmx_preprocess_quads_persp", "dmx_postprocess_paste_quads_persp", "dmx_rectify_quads_persp"):
        assert name in _cabi.exported_symbols()
