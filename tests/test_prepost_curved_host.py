"""The host half of curved text regions (csrc/prepost_curved.h, prepost.strip_size_curved / curved_frame_for / plan_curved, the C-ABI's
host-only dmx_edit_curved_prepare): every prepared integer against the restatement (tests/curved_restatement.py), every coordinate of every
piece against the exact affine map in fractions.Fraction, the agreement of neighbouring pieces on shared edges and diagonals, the n = 2 and
the subdivided parallelogram against dmx_edit_quads_persp_prepare, the restatement's invariance under a quarter turn, six injected faults
that must break these comparisons, every refusal by index, and the planner.  Nothing here needs a GPU."""
import ctypes
from fractions import Fraction

import numpy as np
import pytest

import curved_cases as CC
import curved_restatement as CR
import persp_restatement as PR
import quad_restatement as QR

S = CC.S
BOUND = CR.BOUND


def _prepared(lib=None, S_=S, polygons=None, frames=None, sizes=CC.PAGES):
    from diffute_amd import _cabi
    lib = lib or _cabi.lib()
    if polygons is None:
        polygons, frames = CC.lists()
    pt, ct, xt = CC.tables(sizes, polygons, frames)
    _cabi.check(lib.dmx_edit_curved_prepare(pt, len(sizes), ct, xt, sum(len(q) for q in polygons), S_), "edit_curved_prepare", lib)
    return pt, ct, xt


@pytest.fixture(scope="module")
def world():
    """random pages, the cases' prepared integers (from the prepare entry) and decoder outputs, computed once and only read afterwards"""
    rs = np.random.RandomState(20261021)
    pages = [rs.randint(0, 256, (h, w, 3), dtype=np.uint8) for h, w in CC.PAGES]
    polygons, frames = CC.lists()
    pt, ct, xt = _prepared()
    items = [CR.from_table(c, xt) for c in ct]
    vae = (rs.standard_normal((CC.N, 3, S, S)) * 0.6).clip(-1.3, 1.3).astype(np.float32)
    for a in pages + [vae]:
        a.setflags(write=False)
    return dict(pages=pages, polygons=polygons, frames=frames, items=items, vae=vae)


def _paste(world, p, faults=()):
    mine = [b for b, it in enumerate(world["items"]) if it["page"] == p]
    return CR.paste_page(world["pages"][p], [world["items"][b] for b in mine], [world["vae"][b] for b in mine], S, faults)


def test_cases_cover_what_they_claim(world):
    names = [it[0] for _, it in CC.FLAT]
    assert names == ["arc90", "overlap", "s_bend", "border", "arc270", "downwards", "two_rows", "one_column", "overhang"]
    assert sorted({len(it[1]) // 2 for _, it in CC.FLAT}) == [2, 3, 4, 7, 17] and CC.N == 9 and CC.CELLS == 36
    it = dict(zip(names, world["items"]))
    assert it["two_rows"]["rh"] == 2 and it["one_column"]["c"][1:3] == [40, 41], "a region two rows high, a cell one column long"
    assert it["border"]["bx1"] == 0 and it["border"]["by1"] == 0
    Y, X = np.mgrid[0:160, 0:200]
    both = CR.inside(it["arc90"], X, Y) & CR.inside(it["overlap"], X, Y)
    assert both.sum() > 100 and (_paste(world, 0)["hit"][both] == 1).all(), "overlap lies over arc90 and, the later one, decides"
    X16, Y16, piece = CR.crop_coords(it["overhang"], S)
    assert (Y16 >> 16).max() >= 100 and (X16 >> 16).max() >= 180, "overhang: the window has clamped taps"
    for name in ("arc90", "arc270", "s_bend"):
        assert len(np.unique(CR.crop_coords(it[name], S)[2])) == 2 * (it[name]["n"] - 1), f"{name}: every piece is seen in the crop"
    t0, t1 = it["downwards"]["y"][0], it["downwards"]["y"][2]
    assert t1 - t0 == 90 and abs(it["downwards"]["x"][2] - it["downwards"]["x"][0]) < 3, "downwards is read top to bottom"
    a = it["arc270"]
    ang = lambda k: np.degrees(np.arctan2(a["y"][k] - 60, a["x"][k] - 75)) % 360
    assert abs((ang(16) - ang(0)) % 360 - 270) < 2, "arc270 spans 270 degrees"


def test_prepare_fills_what_the_restatement_derives():
    """every integer dmx_edit_curved_prepare writes equals the restatement's host half, on both builds and at three sizes; the
    restatement's own acceptance agrees; the offsets are the running sums; S = 0 fills the strip maps alone"""
    from diffute_amd import _cabi
    assert ctypes.sizeof(_cabi.EditCurved) == 100 * 4 + 8 and ctypes.sizeof(_cabi.CurvedPiece) == 2 * 4 + 3 * 88
    for elem in ("bf16", "fp16"):
        for S_ in (32, S, 512):
            pt, ct, xt = _prepared(_cabi.lib(elem), S_)
            pieces = rect_off = rect_blocks = 0
            for b, (p, (name, pts, cs, ctr)) in enumerate(CC.FLAT):
                got, want = CR.from_table(ct[b], xt), CR.host_item(pts, CC.frame_of(pts, cs, ctr), S_)
                for k in CR.ITEM_FIELDS:
                    assert got[k] == want[k], f"{name}: {k} differs from the restatement (S = {S_}, {elem})"
                assert got["pieces"] == want["pieces"], f"{name}: a piece's maps differ from the restatement (S = {S_}, {elem})"
                CR.check_cells(pts, *CC.PAGES[p])
                CR.accept(want, S_)
                assert all(m[k]["t"][6:] == [0, 0, 1 << PR.Q] for m in got["pieces"] for k in PR.MAP_NAMES), "an affine map: t6 = t7 = 0, D = 2^43"
                assert (got["page"], got["piece_lo"], got["piece_count"]) == (p, pieces, len(pts) - 2)
                assert (got["rect_off"], got["rect_block_lo"], got["rect_blocks"]) == (rect_off, rect_blocks, got["rh"] * ((got["rw"] + 255) // 256))
                pieces, rect_off, rect_blocks = pieces + len(pts) - 2, rect_off + got["rw"] * got["rh"] * 3, rect_blocks + got["rect_blocks"]
            assert [(g.block_lo, g.blocks) for g in pt] == [(0, 160), (160, 120), (280, 100)]
    lib = _cabi.lib()
    polygons, _ = CC.lists()
    pt, ct, xt = CC.tables(CC.PAGES, polygons, [[None] * len(q) for q in polygons])
    _cabi.check(lib.dmx_edit_curved_prepare(pt, 3, ct, xt, CC.N, 0), "strips only")
    full = _prepared()
    for b in range(CC.N):
        got, ref = CR.from_table(ct[b], xt), CR.from_table(full[1][b], full[2])
        assert [m["strip"] for m in got["pieces"]] == [m["strip"] for m in ref["pieces"]]
        assert all(m["crop"]["t"] == [0] * 9 and m["paste"]["t"] == [0] * 9 for m in got["pieces"])


def _points_of(item, page_size):
    """per map name: (p, q, piece) - the grid points the kernels evaluate, and the piece each takes"""
    H, W = page_size
    Y, X = np.mgrid[0:H, 0:W]
    pc = CR.page_pieces(item, X, Y)
    sel = pc >= 0
    out = {}
    px, py = PR.crop_grid(S)
    out["crop"] = (px.reshape(-1), py.reshape(-1), CR.crop_coords(item, S)[2].reshape(-1))
    sx, sy = PR.strip_grid(item["rw"], item["rh"])
    out["strip"] = (sx.reshape(-1), sy.reshape(-1), CR.strip_coords(item)[2].reshape(-1))
    out["paste"] = (X[sel].astype(np.int64), Y[sel].astype(np.int64), pc[sel])
    return out


def _worst_error(points, item, frame, faults=(), maps=PR.MAP_NAMES, page_size=None):
    """the largest |coordinate - exact coordinate * 2^16| over the points the kernels evaluate, per map, as Fractions; the exact map of a
    piece is taken about the (cx2, cy2) of the piece under test"""
    worst = {}
    pts = _points_of(item, page_size)
    for name in maps:
        p, q, piece = pts[name]
        w = Fraction(0)
        for g in np.unique(piece):
            m = item["pieces"][int(g)]
            exact = CR.exact_matrices(CR.piece_matrix(points, item["c"], item["rh"], int(g)), item["rw"], item["rh"], frame, S, m["cx2"], m["cy2"])[name]
            sel = piece == g
            gp, gq = (p[sel], q[sel]) if name != "paste" else (2 * p[sel] - m["cx2"], 2 * q[sel] - m["cy2"])
            A16, B16 = (np.asarray(a).reshape(-1) for a in PR.coords(m[name], gp, gq, faults=faults))
            for a16, b16, u, v in zip(A16.tolist(), B16.tolist(), gp.tolist(), gq.tolist()):
                ex, ey = CR.exact_point(exact, u, v)
                w = max(w, abs(a16 - ex * 65536), abs(b16 - ey * 65536))
        worst[name] = w
    return worst


def test_every_coordinate_is_within_the_bound_of_the_exact_map(world):
    """all three maps of every piece, at every point its kernel evaluates it: within 0.6251 units of 2^-16 of the exact affine map"""
    seen = Fraction(0)
    for b, (p, (name, pts, cs, ctr)) in enumerate(CC.FLAT):
        worst = _worst_error(pts, world["items"][b], CC.frame_of(pts, cs, ctr), page_size=CC.PAGES[p])
        for k, w in worst.items():
            assert w <= BOUND, f"{name}: {k}: {float(w):.4f} units beyond the bound"
            seen = max(seen, w)
    assert seen > Fraction(1, 2) - Fraction(1, 100), "the final rounding alone comes close to 1 / 2 somewhere"


def _seam_points(item):
    """strip grid points on lines two pieces share: (piece a, piece b, p, q) - the columns c_k between two cells, all rows; the diagonal's
    lattice points of every cell"""
    rw, rh, c, M = item["rw"], item["rh"], item["c"], item["n"] - 1
    h = rh - 1
    out = []
    for k in range(1, M):
        out += [(2 * k - 1, 2 * k, 2 * c[k] + 1 - rw, 2 * j + 1 - rh) for j in range(rh)]
    for k in range(M):
        w = c[k + 1] - c[k]
        out += [(2 * k, 2 * k + 1, 2 * i + 1 - rw, 2 * j + 1 - rh) for i in range(c[k], c[k + 1] + 1) for j in range(rh) if (i - c[k]) * h + j * w == w * h]
    return out


def _worst_seam(item, faults=()):
    worst = 0
    for a, b, p, q in _seam_points(item):
        (xa, ya), (xb, yb) = (PR.coords(item["pieces"][g]["strip"], [p], [q], faults=faults) for g in (a, b))
        worst = max(worst, abs(int(xa[0]) - int(xb[0])), abs(int(ya[0]) - int(yb[0])))
    for k, cell in enumerate(item["cells"]):                 # the paste maps at the cell's corners: 0 and 3 lie on the edge to cell k - 1,
        share = [(0, 2 * k - 1, 2 * k), (3, 2 * k - 1, 2 * k), (1, 2 * k, 2 * k + 1), (3, 2 * k, 2 * k + 1)]     # 1 and 3 on the diagonal
        for corner, a, b in share:
            if a < 0:
                continue
            X, Y = cell["x"][corner], cell["y"][corner]
            uv = []
            for g in (a, b):
                m = item["pieces"][g]
                u, v = PR.coords(m["paste"], [2 * X - m["cx2"]], [2 * Y - m["cy2"]], faults=faults)
                uv.append((int(u[0]), int(v[0])))
            worst = max(worst, abs(uv[0][0] - uv[1][0]), abs(uv[0][1] - uv[1][1]))
    return worst


def test_neighbouring_pieces_agree_on_the_lines_they_share(world):
    """on a shared cell edge and on a diagonal the two pieces' exact maps are the same map, so their Q16 coordinates differ by at most
    twice the bound: the paste does not tear"""
    n_pts = 0
    for b, (p, (name, _, _, _)) in enumerate(CC.FLAT):
        n_pts += len(_seam_points(world["items"][b]))
        assert _worst_seam(world["items"][b]) <= 2 * BOUND, f"{name}: two pieces disagree on a line they share"
    assert n_pts > 500


def test_a_parallelogram_is_the_projective_quad_piece_for_piece():
    """n = 2 on a parallelogram: both pieces hold the maps dmx_edit_quads_persp_prepare fills for the same quad and frame; the same
    parallelogram cut at whole-number cell lengths holds them in every piece (relative is scale-invariant: exact)"""
    import persp_cases as PC
    from diffute_amd import _cabi
    lib = _cabi.lib()
    for S_ in (32, S, 512):
        for quad, page in ((CC.PARA, CC.PARA_PAGE), (CC.FLAT[8][1][1], CC.PAGES[2]), (CC.box(20, 30, 70, 44), CC.PAGES[0])):
            rw, rh = CC.strip_size(quad)
            frame = (rw - 1 + 6, rh - 1 - 4, 90)
            pt, qt, xt = PC.tables([page], [[quad]], [[frame]])
            _cabi.check(lib.dmx_edit_quads_prepare(pt, 1, qt, 1, max(S_, 8)), "edit_quads_prepare")
            _cabi.check(lib.dmx_edit_quads_persp_prepare(pt, 1, qt, xt, 1, S_), "edit_quads_persp_prepare")
            want = PR.from_table(xt[0])
            assert (qt[0].rw, qt[0].rh) == (rw, rh), "the strip of a parallelogram is the quad's strip"
            polys = [quad] + ([CC.PARA_CUT] if quad is CC.PARA else [])
            for poly in polys:
                _, ct, yt = _prepared(lib, S_, [[poly]], [[frame]], [page])
                got = CR.from_table(ct[0], yt)
                assert (got["rw"], got["rh"]) == (rw, rh)
                for g, m in enumerate(got["pieces"]):
                    assert {k: m[k] for k in ("cx2", "cy2") + PR.MAP_NAMES} == {k: want[k] for k in ("cx2", "cy2") + PR.MAP_NAMES}, f"piece {g} of {len(poly)} points"
    assert CR.strip(CC.PARA_CUT)[2] == [0, 30, 60, 100]


def _turned(world, b):
    p = world["items"][b]["page"]
    H, W = CC.PAGES[p]
    pts = CC.FLAT[b][1][1]
    return QR.rot90_page(world["pages"][p]), QR.rot90_corners(pts, W)


def _quarter_turn_holds(world, b, faults=()):
    """crop and strip of the turned page with the turned polygon equal the upright ones, bit for bit"""
    _, (name, pts, cs, ctr) = CC.FLAT[b]
    frame = CC.frame_of(pts, cs, ctr)
    page = world["pages"][world["items"][b]["page"]]
    tpage, tpts = _turned(world, b)
    a, t = CR.host_item(pts, frame, S, faults), CR.host_item(tpts, frame, S, faults)
    pa, pt_ = CR.preprocess(page, a, S, faults), CR.preprocess(tpage, t, S, faults)
    return all(np.array_equal(pa[k], pt_[k]) for k in pa) and np.array_equal(CR.rectify(page, a, faults), CR.rectify(tpage, t, faults))


def test_the_restatement_is_invariant_under_a_quarter_turn(world):
    for b in range(CC.N):
        assert _quarter_turn_holds(world, b), CC.FLAT[b][1][0]
    for p, (H, W) in enumerate(CC.PAGES):                      # the pasted turned page is the turned pasted page
        mine = [b for b in range(CC.N) if world["items"][b]["page"] == p]
        titems = [CR.host_item(QR.rot90_corners(CC.FLAT[b][1][1], W), world["frames"][p][i], S) for i, b in enumerate(mine)]
        got = CR.paste_page(QR.rot90_page(world["pages"][p]), titems, [world["vae"][b] for b in mine], S)
        want = _paste(world, p)
        assert np.array_equal(got["out"], np.rot90(want["out"])) and np.array_equal(got["union"], np.rot90(want["union"])), f"page {p}"


def test_six_injected_faults_break_the_comparisons(world):
    """each deliberate mistake of tests/curved_restatement.py is seen by one of the comparisons above"""
    names = [it[0] for _, it in CC.FLAT]
    b90, b270, bs = names.index("arc90"), names.index("arc270"), names.index("s_bend")

    def table_differs(b, fault):
        _, (name, pts, cs, ctr) = CC.FLAT[b]
        bad, good = CR.host_item(pts, CC.frame_of(pts, cs, ctr), S, (fault,)), world["items"][b]
        return any(bad[k] != good[k] for k in CR.ITEM_FIELDS) or bad["pieces"] != good["pieces"]
    # a floor instead of ties-away: the table differs, and the quarter turn no longer holds
    assert table_differs(b90, "floor") and not all(_quarter_turn_holds(world, b, ("floor",)) for b in (b90, bs))
    # the other diagonal: other maps in the table, other bytes in crop and paste
    assert table_differs(bs, "other_diagonal")
    page0 = world["pages"][0]
    assert not np.array_equal(CR.rectify(page0, world["items"][bs], ("other_diagonal",)), CR.rectify(page0, world["items"][bs]))
    # a cell picked by bounding boxes: the bent cells' boxes overlap, and the paste takes another piece
    assert not np.array_equal(_paste(world, 1, ("bbox_cell",))["piece"], _paste(world, 1)["piece"])
    assert not np.array_equal(_paste(world, 1, ("bbox_cell",))["out"], _paste(world, 1)["out"])
    # one homography per cell: the table differs, and two cells disagree BETWEEN the ends of the edge they share
    _, (name, pts, cs, ctr) = CC.FLAT[bs]
    hom = CR.host_item(pts, CC.frame_of(pts, cs, ctr), S, ("homography",))
    assert table_differs(bs, "homography") and _worst_seam(hom) > 1000 * 2 * BOUND
    # rh from the summed vectors: around three quarters of a circle they cancel
    assert CR.strip(CC.FLAT[b270][1][1], ("rh_summed",))[1] != world["items"][b270]["rh"] == 21
    # a predicate that leaves a cell out: a smaller mask, a smaller paste
    item = world["items"][b90]
    full, less = CR.preprocess(page0, item, S), CR.preprocess(page0, item, S, ("cell_left_out",))
    assert less["mask"].sum() < full["mask"].sum() and np.array_equal(less["image"], full["image"])
    assert _paste(world, 0, ("cell_left_out",))["union"].sum() < _paste(world, 0)["union"].sum()


def test_every_refusal_is_made_by_index():
    from diffute_amd import _cabi
    lib = _cabi.lib()
    polygons, frames = CC.lists()

    def refused(polys, frs, S_=S, sizes=CC.PAGES, B=None):
        pt, ct, xt = CC.tables(sizes, polys, frs)
        rc = lib.dmx_edit_curved_prepare(pt, len(sizes), ct, xt, sum(len(q) for q in polys) if B is None else B, S_)
        return lib.dmx_last_error().decode() if rc != 0 else None

    def swap(p, j, pts, frame=(20, 10, 64)):
        qs, fs = [list(q) for q in polygons], [list(f) for f in frames]
        qs[p][j], fs[p][j] = pts, frame
        return qs, fs
    assert refused(polygons, frames) is None
    for (p, j, pts), words in [((0, 2, CC.ODD), ("item 2", "5 points")), ((1, 1, CC.CONCAVE), ("item 5", "cell 0", "turns the wrong way")),
                               ((0, 1, CC.COUNTER), ("item 1", "cell 0")), ((2, 0, CC.FLAT_STRIP), ("item 6", "thinner than 2")),
                               ((0, 3, CC.OUTSIDE), ("item 3", "cell 0", "point 1 (200, 20)", "200x160")),
                               ((0, 0, CC.FAN), ("item 0", "cell 0", "piece 1", "page -> crop"))]:
        why = refused(*swap(p, j, pts))
        assert why is not None and all(w in why for w in words), (words, why)
    bent = list(polygons[1][0])
    bent[5] = (75, 60)                                         # top point 5 of arc270 pulled to the centre: cell 4 is no longer convex
    why = refused(*swap(1, 0, bent, frames[1][0]))
    assert "item 4" in why and "cell 4" in why
    one = [(10 + 3 * k, 10) for k in range(18)] + [(10 + 3 * k, 30) for k in reversed(range(18))]
    assert "18 point pairs" in refused(*swap(0, 0, one)) and "item 0" in refused(*swap(0, 0, one))
    assert "1 point pairs" in refused(*swap(2, 2, [(10, 10), (10, 30)]))
    for frame, word in (((20, 10, 0), "no frame"), ((20, 10, 65536), "crop_scale outside"), ((1 << 21, 10, 64), "beyond +-2^20")):
        why = refused(*swap(2, 1, polygons[2][1], frame))
        assert "item 7" in why and word in why, why
    assert refused(*swap(2, 1, polygons[2][1], (20, 10, 0)), S_=0) is None, "the strips read no frame"
    # a window so far from its line that the page -> crop numerators leave the budget
    why = refused(*swap(2, 2, polygons[2][2], (1 << 20, 1 << 20, 1)), S_=512)
    assert why is not None and "item 8" in why and "piece" in why, why
    # the tables' own limits: items, cells, pages, page index
    many = [[CC.box(2 + 3 * k, 2, 4 + 3 * k, 8) for k in range(65)]]
    assert "65 items" in refused(many, [[(2, 6, 8)] * 65], sizes=[(20, 220)])
    ring = CC.arc(75, 60, 30, 50, 135, 405, 17)
    why = refused([[ring] * 33], [[frames[1][0]] * 33], sizes=[CC.PAGES[1]])
    assert "item 32" in why and "more than 512 cells" in why
    pt, ct, xt = CC.tables(CC.PAGES, polygons, frames)
    ct[5].page = 2
    assert lib.dmx_edit_curved_prepare(pt, 3, ct, xt, CC.N, S) == -1 and "item 5: page index 2" in lib.dmx_last_error().decode()
    pt, ct, xt = CC.tables(CC.PAGES, polygons, frames)
    pt[1].item_lo = 5
    assert lib.dmx_edit_curved_prepare(pt, 3, ct, xt, CC.N, S) == -1 and "page 1" in lib.dmx_last_error().decode()


def test_the_planner_gives_the_hand_computed_cases():
    from diffute_amd import prepost
    # an upright 100 x 20 rectangle in four cells: rw = 101, rh = 21; 6 * 21 = 126 < 128 -> crop_scale max(128, 101) = 128
    rect = [(10, 40), (35, 40), (60, 40), (85, 40), (110, 40), (110, 60), (85, 60), (60, 60), (35, 60), (10, 60)]
    assert prepost.strip_size_curved(rect) == (101, 21) and prepost.curved_frame_for(rect, 300, 400, S) == (100, 20, 128)
    assert prepost.curved_frame_for(rect, 90, 400, S) == (100, 20, 90), "no larger than the page's short side"
    # 3-4-5 cells, the bottom 10 below the top: |u_k| / 2 = 50 each, every segment T_k B_k is 10 long
    bent = [(10, 50), (50, 20), (90, 50), (90, 60), (50, 30), (10, 60)]
    assert prepost.strip_size_curved(bent) == (101, 11) and prepost.curved_frame_for(bent, 200, 200, S) == (100, 10, 128)
    # a trapezoid: u = (200, 11), |u| / 2 = 100.15; its sides are 10 and 21 long, their mean 15.5 goes to the even 16
    assert prepost.strip_size_curved([(10, 10), (110, 10), (110, 31), (10, 20)]) == (101, 17)
    assert prepost.strip_size_curved(CC.PARA) == prepost.strip_size(CC.PARA) == (101, 16)
    for _, (name, pts, _, _) in CC.FLAT:
        assert prepost.strip_size_curved(pts) == CC.strip_size(pts), name
    polygons, _ = CC.lists()
    frames = prepost.plan_curved(polygons, CC.PAGES, S)
    assert frames == prepost.plan_curved(polygons, CC.PAGES, S), "deterministic"
    assert frames[1] == [(188, 20, 120), (90, 14, 120)] and frames[2][0] == (60, 1, 100)
    with pytest.raises(ValueError, match="odd point count"):
        prepost.curved_frame_for(CC.ODD, 160, 200, S)
    with pytest.raises(ValueError, match="cell 0 turns the wrong way"):
        prepost.curved_frame_for(CC.COUNTER, 160, 200, S)
    with pytest.raises(ValueError, match="thinner than 2"):
        prepost.plan_curved([[CC.FLAT_STRIP]], [(160, 200)], S)
    with pytest.raises(ValueError, match="lengths must agree"):
        prepost.plan_curved(polygons, CC.PAGES[:2], S)
    assert prepost.curved_frame_accepted(rect, 300, 400, (100, 20, 128), S) is None
    assert "item 0" in prepost.curved_frame_accepted(rect, 300, 400, (100, 20, 0), S)


def test_the_strip_of_an_arc_on_a_radial_ramp_is_straight():
    """the restatement's strip of the M = 6 arc on a page whose value is a linear ramp in r: every row is flat within the bound derived
    in tests/curved_cases.ramp_bound (3.79 levels; the restatement measures 3) - and the same band as ONE quad, through the projective
    strip, exceeds it in every row (its sagitta is 23.4 pixels), so the bound can fail"""
    page = CC.ramp_page()
    bound = CC.ramp_bound(CC.RAMP_M)
    assert 3.7 < bound < 3.8
    item = CR.host_item(CC.RAMP_ARC, (0, 0, 0), 0)
    spread = CC.row_spread(CR.rectify(page, item))
    assert len(spread) == 21 and spread.max() <= bound, f"the strip is bent: a row spreads over {spread.max()} levels"
    assert spread.max() == 3, "the figure DESIGN.md states"
    q = QR.derive(CC.RAMP_QUAD, (0, 0, 1, 1, 0), 1)
    pm = PR.host_maps(CC.RAMP_QUAD, q["rw"], q["rh"], (q["rw"] - 1, q["rh"] - 1, 64), 64)
    bent = CC.row_spread(PR.rectify(page, q, pm))
    assert bent.min() > bound and bent.min() > 30, "one quad leaves the arc's bend in the strip"
