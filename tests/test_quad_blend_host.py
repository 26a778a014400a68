"""The feathered, colour-matched paste for quads without a GPU: the exact edge steps of csrc/prepost_quad_blend.h (through the host-only
entries dmx_test_quad_edge_steps / _threshold of both builds) against Python ints at magnitudes no small page reaches; the integer
restatement (tests/quad_blend_restatement.py) against the box blend's restatement, against the plain quad paste and against its own
invariants - union mask, quarter turn, uniform pages, statistics that depend on nothing but their item -; seven injected faults, each of
which must change some case; the checks of QuadBlend and every refusal of the Python functions and of the C entries (dummy addresses:
nothing is launched)."""
import ctypes
import random
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import paste_blend_restatement as PB
import persp_cases as PC
import quad_blend_cases as BC
import quad_blend_restatement as QB
import quad_cases as QC
import quad_restatement as QR

S, PAGES, M = BC.S, BC.PAGES, QB.M


@pytest.fixture(scope="module")
def cases():
    return {c.name: c for c in BC.cases()}


@pytest.fixture(scope="module")
def expected(cases):
    """the restatement's pages, masks and statistics: computed once, only read afterwards"""
    exp = {name: c.expected() for name, c in cases.items()}
    for pages in exp.values():
        for out, mask, _ in pages:
            out.setflags(write=False); mask.setflags(write=False)
    return exp


# ---------------------------------------------------------------------------------------------------------------- the exact edge steps
def _edge_inputs():
    """(ex, ey, E, M): |E| up to 2^33, L2 up to 2 * 65535^2 (just below 2^33), ties j^2 L2 == E^2, both signs, a zero-length edge"""
    rnd = random.Random(20261021)
    out = []
    edges = [(3, 4), (-3, 4), (65535, 0), (0, -65535), (65535, 65535), (-65535, 65535), (1, 0), (0, 1), (1, 1), (120, 17), (-7, -24), (20, 21), (0, 0),
             (46341, 0), (32768, 32767)]
    for ex, ey in edges:
        L2 = ex * ex + ey * ey
        root = int(round(L2 ** 0.5))
        for j in (0, 1, 2, 5, 1024, 1025, 2047, 2048, 2049, 2050, 2051, 2052, 4000):
            for e in (j * root, j * root + 1, j * root - 1):                          # ties where root^2 == L2, their neighbours
                out += [(ex, ey, e, M), (ex, ey, -e, M)]
        for E in (0, 1, -1, (1 << 31) - 1, -(1 << 31) + 1, 1 << 31, -(1 << 31), (1 << 31) + 1, (1 << 33), -(1 << 33), (1 << 33) - 1, (1 << 32) + 12345):
            out += [(ex, ey, E, M), (ex, ey, E, 1), (ex, ey, E, 7)]
        for _ in range(200):
            mag = rnd.choice((8, 12, 20, 28, 31, 33))
            out.append((ex, ey, rnd.randint(-(1 << mag), 1 << mag), rnd.choice((M, M, 1, 100))))
    for _ in range(3000):
        ex, ey = rnd.randint(-65535, 65535), rnd.randint(-65535, 65535)
        L2 = ex * ex + ey * ey
        j = rnd.randint(-M - 3, M + 3)
        near = int(j * L2 ** 0.5) + rnd.randint(-2, 2)                                # around a step boundary
        out += [(ex, ey, max(min(near, 1 << 33), -(1 << 33)), M), (ex, ey, rnd.randint(-(1 << 33), 1 << 33), M)]
    return out


@pytest.mark.parametrize("elem", ["bf16", "fp16"])
def test_edge_steps_and_thresholds_are_the_python_ints(elem):
    from diffute_amd import _cabi
    lib = _cabi.lib(elem)
    inputs = _edge_inputs()
    assert any(abs(E) >= 1 << 33 for _, _, E, _ in inputs) and any(ex * ex + ey * ey > (1 << 33) - (1 << 18) for ex, ey, _, _ in inputs)
    ties = 0
    for ex, ey, E, m in inputs:
        want = QB.edge_steps_int(ex, ey, E, m)
        assert lib.dmx_test_quad_edge_steps(ex, ey, E, m) == want, (ex, ey, E, m)
        L2 = ex * ex + ey * ey
        ties += int(L2 > 0 and E != 0 and abs(want) < m and want * want * L2 == E * E)
    assert ties > 100, "the inputs hold exact ties j^2 L2 == E^2"
    assert QB.edge_steps_int(3, 4, -51) == -11 and QB.edge_steps_int(3, 4, -50) == -10 and QB.edge_steps_int(3, 4, 49) == 9 and QB.edge_steps_int(0, 0, -9) == M
    rnd = random.Random(5)
    for ex, ey in [(3, 4), (65535, 65535), (1, 0), (0, -1), (120, 17), (65535, 1)] + [(rnd.randint(-65535, 65535), rnd.randint(1, 65535)) for _ in range(300)]:
        for j in (-M, -2049, -1025, -9, -1, 0, 1, 2, 10, 1024, 1025, M, rnd.randint(-M, M)):
            thr = lib.dmx_test_quad_edge_threshold(ex, ey, j)
            assert thr == QB.edge_threshold_int(ex, ey, j), (ex, ey, j)
            assert QB.edge_steps_int(ex, ey, thr) >= j > QB.edge_steps_int(ex, ey, thr - 1) or j == -M, "the threshold is the least E with s >= j"
    lo = -(1 << 63)
    assert lib.dmx_test_quad_edge_steps(65536, 0, 1, M) == lo and lib.dmx_test_quad_edge_steps(1, 0, (1 << 33) + 1, M) == lo
    assert lib.dmx_test_quad_edge_steps(1, 0, 1, 0) == lo and lib.dmx_test_quad_edge_steps(1, 0, 1, M + 1) == lo
    assert lib.dmx_test_quad_edge_threshold(0, 0, 1) == lo and lib.dmx_test_quad_edge_threshold(1, 0, M + 1) == lo


def test_the_array_form_of_the_edge_steps_is_the_python_int_form():
    rnd = random.Random(3)
    for ex, ey in [(3, 4), (120, 17), (-99, 14), (1, 1), (299, 0)]:
        E = np.array([rnd.randint(-(1 << 22), 1 << 22) for _ in range(500)] + [5 * j for j in range(-30, 30)], dtype=np.int64)
        assert QB.edge_steps(ex * ex + ey * ey, E).tolist() == [QB.edge_steps_int(ex, ey, int(e)) for e in E]


# ---------------------------------------------------------------------------------------------------------------- equalities
@pytest.mark.parametrize("blend", [dict(feather=0, grow=0), dict(feather=4, grow=0), dict(feather=9, grow=0), dict(feather=3, grow=5), dict(feather=2, grow=2)])
def test_an_axis_aligned_quad_has_the_weights_of_the_box_blend(blend):
    """the weight map a on a 64 x 80 page against the box blend's restatement on the rectangle (x1, y1, x2 + 1, y2 + 1): a white patch over a
    black page shows the weight in its bytes, floor((2 * 255 a + F) / (2 F)), and F <= 10 < 255 keeps distinct weights distinct"""
    h, w, (x1, y1, x2, y2) = 64, 80, (12, 20, 51, 33)
    bl, F = QB.Blend(**blend), blend["feather"] + 1
    byte = [(2 * 255 * a + F) // (2 * F) for a in range(F + 1)]
    assert len(set(byte)) == F + 1
    page = np.zeros((h, w, 3), np.uint8)
    box = page.copy()
    PB.paste_one(box, page, np.ones((3, 16, 16), np.float32), (x1, y1, x2 + 1, y2 + 1), (0, 0), 128, PB.Blend(**blend))
    q = QR.derive(QC.box_quad(x1, y1, x2, y2), (2 * x1, 2 * y1, 1, 1, 0), 1)
    Y, X = np.mgrid[0:h, 0:w]
    cover, a = QB.weights(q, X, Y, bl)
    assert cover.sum() == (x2 - x1 + 1 + 2 * bl.grow) * (y2 - y1 + 1 + 2 * bl.grow) and a[cover].min() == 1 and a.max() == min(F, 6 + bl.grow + 1)
    assert np.array_equal(box[:, :, 0], np.where(cover, np.array(byte)[np.clip(a, 0, F)], 0))
    assert np.array_equal(QB.depth(q, X, Y), np.minimum(np.minimum(X - x1, x2 - X), np.minimum(Y - y1, y2 - Y))), "m is the distance on the rectangle"


def test_everything_off_is_the_plain_quad_paste_where_every_quad_lies_on_its_crop():
    for c in BC.on_crop_cases():
        flat = [n for ns in c.names for n in ns]
        assert set(flat) == set(BC.ON_CROP) - ({"degenerate_corner"} if c.persp else set())
        for p, page in enumerate(c.pages):
            items = c.page_items(p)
            assert QB.covered_off_crop(page, items, S) == 0, "the premise: no covered pixel off its quad's crop"
            out, mask, stats = QB.paste_page(page, items, S, c.blend)
            plain = QB.plain_paste_page(page, items, S)
            assert stats is None and np.array_equal(out, plain["out"]) and np.array_equal(mask, plain["union"]), f"{c.name}: page {p}"
            assert (out != page).any()


def test_off_the_crop_an_earlier_item_shows_through_where_the_plain_paste_resets(cases):
    """the stated deviation, on the full geometry with everything off: the pages differ from the plain paste exactly at pixels whose LAST
    covering quad has them off its crop while an earlier one has them on its crop"""
    seen = 0
    for persp in (False, True):
        c = BC.Case("x", persp, QB.Blend(), False)
        for p, page in enumerate(c.pages):
            items = c.page_items(p)
            out, mask, _ = QB.paste_page(page, items, S, c.blend)
            plain = QB.plain_paste_page(page, items, S)
            assert np.array_equal(mask, plain["union"])
            X, Y = QB._grid(page)
            earlier = np.zeros(mask.shape, bool)
            for b, (q, pm, _) in enumerate(items):
                earlier |= QR.inside(q, X, Y) & QB.on_crop(q, pm, S, X, Y)[0] & (plain["hit"] > b)
            differ = (out != plain["out"]).any(axis=2)
            assert not (differ & ~(earlier & ~plain["pasted"])).any()
            seen += int(differ.sum())
            assert np.array_equal(QB.paste_page(page, items, S, c.blend, "last_decides")[0], plain["out"]), "with the plain rule put back: the plain paste"
    assert seen > 0, "under_the_end under the end of upside_down: the deviation shows in the cases"


# ---------------------------------------------------------------------------------------------------------------- invariants
def test_union_mask_and_untouched_pixels(cases, expected):
    for name, c in cases.items():
        for p, (out, mask, stats) in enumerate(expected[name]):
            page = c.pages[p]
            assert np.array_equal(out[mask == 0], page[mask == 0]), f"{name}: out == original wherever the mask is 0"
            X, Y = QB._grid(page)
            inside = np.zeros(mask.shape, bool)
            boxes = np.zeros(mask.shape, bool)
            for q, _, _ in c.page_items(p):
                inside |= QR.inside(q, X, Y)
                g = c.blend.grow
                boxes |= (X >= q["bx1"] - g) & (X <= q["bx2"] + g) & (Y >= q["by1"] - g) & (Y <= q["by2"] + g)
            assert (mask[inside] == 1).all() and (mask[~boxes] == 0).all()
            if c.blend.grow == 0:
                assert np.array_equal(mask.astype(bool), inside), "m >= 0 is the plain coverage"
            else:
                assert mask.sum() > inside.sum()
    lp = expected["sim-feather_grow_match"][0][1]
    assert lp[149, 0:8].any() or lp[140:150, 0].any(), "leaves_page: the grown region reaches the page's border"


def test_every_matching_item_has_a_ring(cases, expected):
    for name, c in cases.items():
        if not c.blend.match_color:
            continue
        flat = [s for _, _, stats in expected[name] for s in stats]
        assert len(flat) == c.N
        for b, st in enumerate(flat):
            if c.choice is not None and c.choice[b] < 0:
                assert st == (0, 0, 0, 0)
            else:
                assert st[0] > 0, f"{name}: item {b} has an empty ring"
                assert all(abs(d) <= c.blend.max_shift * st[0] for d in st[1:])
        assert any(abs(d) == c.blend.max_shift * st[0] for st in flat for d in st[1:] if st[0]), "some shift reaches the clamp"
        assert any(0 < abs(d) < c.blend.max_shift * st[0] for st in flat for d in st[1:] if st[0]), "some shift stays below it"


@pytest.mark.parametrize("name", ["sim-feather_grow_match", "persp-feather_grow_match", "sim-choice_k3", "persp-grow_lt_feather"])
def test_a_quarter_turn_turns_pages_masks_and_statistics(cases, expected, name):
    c = cases[name]
    tp, tq, tf = BC.rot90_case(c)
    titems = BC.prepared(c.persp, tq, tf, [(w, h) for h, w in PAGES])
    lo = 0
    for p in range(len(PAGES)):
        n = len(c.quads[p])
        items = [titems[b] + (c.row(b),) for b in range(lo, lo + n)]
        out, mask, stats = QB.paste_page(tp[p], items, S, c.blend)
        want = expected[name][p]
        assert np.array_equal(out, np.rot90(want[0])) and np.array_equal(mask, np.rot90(want[1])) and stats == want[2], f"{name}: page {p}"
        lo += n


@pytest.mark.parametrize("persp", [False, True])
def test_a_uniform_page_under_a_uniform_patch_comes_back_as_it_was(persp):
    """page value 140, decoder output 0.2 -> G = 153: the constant between them, 13, is within max_shift, so the matched patch IS the
    page, whatever feather and grow; beyond max_shift (4) it is not"""
    c = BC.Case("u", persp, QB.Blend(feather=3, grow=4, match_color=True, ring=5, max_shift=13), False)
    row = np.full((3, S, S), 0.2, np.float32)
    for p, (h, w) in enumerate(PAGES):
        page = np.full((h, w, 3), 140, np.uint8)
        items = [it[:2] + (row,) for it in c.page_items(p)]
        g = QB.generated(row, S, np.array([1 << 20]), np.array([1 << 20]))
        assert abs(140 - int(g[0, 0])) == 13
        out, mask, stats = QB.paste_page(page, items, S, c.blend)
        assert np.array_equal(out, page) and mask.any() and all(st[0] > 0 and st[1] == -13 * st[0] for st in stats)
        out4, _, _ = QB.paste_page(page, items, S, QB.Blend(feather=3, grow=4, match_color=True, ring=5, max_shift=4))
        assert (out4 != page).any()


def test_statistics_depend_on_their_item_alone(cases, expected):
    for name in ("sim-feather_grow_match", "persp-match_only", "sim-choice_k3"):
        c = cases[name]
        for p, page in enumerate(c.pages):
            items, want = c.page_items(p), expected[name][p][2]
            for b, it in enumerate(items):
                alone = (0, 0, 0, 0) if it[2] is None else QB.color_stats(page, it[0], it[1], it[2], S, c.blend)
                assert alone == want[b], f"{name}: page {p} item {b} alone"
            back = QB.paste_page(page, items[::-1], S, c.blend)[2]
            assert back[::-1] == want, "the order of the table does not change an item's numbers"


# ---------------------------------------------------------------------------------------------------------------- injected faults
@pytest.mark.parametrize("fault", QB.FAULTS)
def test_every_injected_fault_changes_some_case(cases, expected, fault):
    assert len(QB.FAULTS) >= 6
    changed = []
    for name, c in cases.items():
        got = c.expected(fault)
        for p, ((out, mask, stats), (wout, wmask, wstats)) in enumerate(zip(got, expected[name])):
            if not (np.array_equal(out, wout) and np.array_equal(mask, wmask) and stats == wstats):
                changed.append((name, p))
    assert changed, f"the fault {fault} changes no case: the cases do not see it"


# ---------------------------------------------------------------------------------------------------------------- checks and refusals
def test_quad_blend_checks_its_arguments():
    import diffute_amd as D
    from diffute_amd import _cabi, prepost
    assert D.QuadBlend is prepost.QuadBlend and not issubclass(D.QuadBlend, D.PasteBlend) and _cabi.QUAD_BLEND_MAX == 1024
    b = D.QuadBlend()
    assert (b.feather, b.grow, b.match_color, b.ring, b.max_shift) == (0, 0, False, 8, 32)
    b = D.QuadBlend(feather=np.int64(3), grow=2, match_color=np.bool_(True), ring=1024, max_shift=0)
    assert (b.feather, b.grow, b.match_color, b.ring, b.max_shift) == (3, 2, True, 1024, 0) and "feather=3" in repr(b) and repr(b).startswith("QuadBlend(")
    for bad in (dict(feather=-1), dict(grow=-1), dict(ring=0), dict(max_shift=256), dict(max_shift=-1), dict(feather=1025), dict(grow=1025), dict(ring=1025)):
        with pytest.raises(ValueError):
            D.QuadBlend(**bad)
    D.QuadBlend(feather=1024, grow=1024, ring=1024)
    for bad in (dict(feather=1.5), dict(grow="2"), dict(ring=None), dict(max_shift=True), dict(match_color=1)):
        with pytest.raises(TypeError):
            D.QuadBlend(**bad)
    quads = [QC.box_quad(10, 12, 30, 20), [(5, 1), (55, 9), (53, 39), (1, 30)], [5, 1, 55, 9, 53, 39, 1, 30]]
    assert b.grown(quads) == [(8, 10, 33, 23), (-1, -1, 58, 42), (-1, -1, 58, 42)]
    assert b.grown(quads, 40, 56) == [(8, 10, 33, 23), (0, 0, 56, 40), (0, 0, 56, 40)]
    s = b._struct()
    assert (s.feather, s.grow, s.ring, s.max_shift, s.match_color) == (3, 2, 1024, 0, 1)


def test_python_functions_refuse_without_a_gpu():
    import diffute_amd as D
    from diffute_amd import prepost
    img = torch.zeros(64, 80, 3, dtype=torch.uint8)
    quad = [(4, 4), (30, 4), (30, 12), (4, 12)]
    frame = prepost.frame_for(quad, 64, 80)
    vae, sc = torch.zeros(1, 3, 16, 16), torch.zeros(1, 1)
    for fn in (lambda bl: prepost.postprocess_quads(vae, [img], [[quad]], [[frame]], blend=bl),
               lambda bl: prepost.postprocess_select_quads(vae[None], sc, [img], [[quad]], [[frame]], blend=bl),
               lambda bl: prepost.paste_color_stats_quads(vae, [img], [[quad]], [[frame]], bl)):
        with pytest.raises(NotImplementedError, match="QuadBlend"):
            fn(D.PasteBlend(feather=1))
        for bad in ("soft", dict(feather=1), 3):
            with pytest.raises(TypeError, match="QuadBlend"):
                fn(bad)
        with pytest.raises(TypeError):                              # a good blend passes: the host tensors are what is refused
            fn(D.QuadBlend(feather=1, match_color=True))
    with pytest.raises(TypeError, match="QuadBlend"):
        prepost.paste_color_stats_quads(vae, [img], [[quad]], [[frame]], None)
    with pytest.raises(ValueError):
        prepost.postprocess_quads(vae, [], [], [], blend=D.QuadBlend(feather=1))
    with pytest.raises(ValueError):
        prepost.postprocess_quads(vae, [img], [[quad, quad]], [[frame]], blend=D.QuadBlend(feather=1))


def _ocr(image_size=32, vocab=300, positions=64):
    return SimpleNamespace(encoder=SimpleNamespace(config=SimpleNamespace(image_size=image_size)),
                           decoder=SimpleNamespace(config=SimpleNamespace(vocab_size=vocab, max_position_embeddings=positions)))


def test_the_quad_edits_take_none_or_a_quad_blend(monkeypatch):
    """None or a QuadBlend passes the blend check (the next check refuses cache_interval = 0), a PasteBlend raises NotImplementedError that
    names quads and QuadBlend, anything else TypeError; no prepost stage is reached"""
    import diffute_amd as D
    from diffute_amd import pipeline, prepost

    def reached(*a, **kw):
        raise AssertionError("a prepost stage was reached before the arguments were checked")
    for name in ("preprocess_quads", "readback_pixel_values_quads", "postprocess_select_quads", "postprocess_quads", "plan_quads"):
        monkeypatch.setattr(prepost, name, reached)
    assert pipeline.prepost is prepost
    imgs = [torch.zeros(64, 80, 3, dtype=torch.uint8)]
    quads = [[[(4, 4), (30, 4), (30, 12), (4, 12)]]]
    ctx = torch.zeros(1, 77, 128)
    labels = torch.full((1, 5), 7, dtype=torch.int64)
    proc = D.TrOCRProcessor(size=32)
    plain = lambda bl: D.edit_quads(None, None, None, imgs, quads, ctx, 3, size=S, cache_interval=0, blend=bl)
    verified = lambda bl: D.edit_quads_verified(None, None, None, _ocr(), proc, imgs, quads, ctx, labels, 3, size=S, cache_interval=0, blend=bl)
    for call in (plain, verified):
        for ok in (None, D.QuadBlend(), D.QuadBlend(feather=4, grow=2, match_color=True)):
            with pytest.raises(ValueError, match="cache_interval"):
                call(ok)
        with pytest.raises(NotImplementedError, match="quads") as e:
            call(D.PasteBlend(feather=1))
        assert "QuadBlend" in str(e.value)
        for bad in ("soft", dict(feather=1), 1):
            with pytest.raises(TypeError, match="QuadBlend"):
                call(bad)


@pytest.mark.parametrize("elem", ["bf16", "fp16"])
def test_the_c_entries_refuse_and_launch_nothing(elem):
    """all four entries through dummy addresses: every call below is refused by a host-side check, so nothing is launched"""
    from diffute_amd import _cabi
    lib = _cabi.lib(elem)
    for name in ("dmx_paste_color_stats_quads", "dmx_paste_color_stats_quads_persp", "dmx_postprocess_paste_blend_quads",
                 "dmx_postprocess_paste_blend_quads_persp", "dmx_test_quad_edge_steps", "dmx_test_quad_edge_threshold", "dmx_select_choices"):
        assert name in _cabi.exported_symbols() and getattr(lib, name)
    P, addr = len(PAGES), ctypes.c_void_p(4096)
    _, quads, frames = BC.geometry(False)
    _, pquads, pframes = BC.geometry(True)
    pt, qt = QC.tables(PAGES, quads, frames)
    ppt, pqt, pxt = PC.tables(PAGES, pquads, pframes)
    B, PB_ = len(qt), len(pqt)
    assert lib.dmx_edit_quads_prepare(pt, P, qt, B, S) == 0 and lib.dmx_edit_quads_prepare(ppt, P, pqt, PB_, S) == 0
    assert lib.dmx_edit_quads_persp_prepare(ppt, P, pqt, pxt, PB_, S) == 0
    Bl = _cabi.PasteBlend

    def all_four(bl, stats=addr, ch=None, K=1, vae=addr, sim=(pt, qt), per=(ppt, pqt, pxt), s=S, only=range(4)):
        r = ctypes.byref(bl) if bl is not None else None
        calls = [lambda: lib.dmx_paste_color_stats_quads(vae, s, sim[0], addr, P, sim[1], addr, B, r, ch, K, addr, None),
                 lambda: lib.dmx_paste_color_stats_quads_persp(vae, s, per[0], addr, P, per[1], addr, per[2], addr, PB_, r, ch, K, addr, None),
                 lambda: lib.dmx_postprocess_paste_blend_quads(vae, s, sim[0], addr, P, sim[1], addr, B, r, stats, ch, K, None),
                 lambda: lib.dmx_postprocess_paste_blend_quads_persp(vae, s, per[0], addr, P, per[1], addr, per[2], addr, PB_, r, stats, ch, K, None)]
        return [calls[i]() for i in only]
    bad = (Bl(-1, 0, 8, 32, 0), Bl(0, -1, 8, 32, 0), Bl(0, 0, 0, 32, 0), Bl(0, 0, -1, 32, 0), Bl(0, 0, 8, 256, 1), Bl(0, 0, 8, -1, 1), Bl(1025, 0, 8, 32, 0),
           Bl(0, 1025, 8, 32, 0), Bl(0, 0, 1025, 32, 0), Bl(1, 1, 8, 32, 2), Bl(1, 1, 8, 32, -1))
    for bl in bad:
        assert all_four(bl) == [-1] * 4, "a bad blend was accepted"
    assert "1024" in lib.dmx_last_error().decode() or "match_color" in lib.dmx_last_error().decode()
    good = Bl(3, 4, 5, 12, 1)
    assert all_four(None) == [-1] * 4, "null blend"
    assert all_four(good, K=2) == [-1] * 4, "K = 2 without a choice table"
    assert all_four(good, ch=addr, K=17) == [-1] * 4 and all_four(good, ch=addr, K=0) == [-1] * 4
    assert all_four(good, stats=None, only=(2, 3)) == [-1] * 2 and "match_color without" in lib.dmx_last_error().decode()
    assert all_four(good, vae=None) == [-1] * 4, "null decoder outputs"
    assert all_four(good, s=0) == [-1] * 4 and all_four(good, s=65536) == [-1] * 4
    # whatever the plain quad entries refuse, named by page or item index
    saved = qt[2].x[1]
    qt[2].x[1] = 100000
    assert all_four(good, only=(0, 2)) == [-1] * 2 and "item 2" in lib.dmx_last_error().decode()
    qt[2].x[1] = saved
    qt[3].bx2 += 1                                                    # a derived field that does not belong to the quad
    assert all_four(good, only=(0, 2)) == [-1] * 2 and "item 3" in lib.dmx_last_error().decode()
    qt[3].bx2 -= 1
    pt[1].out = 0
    assert all_four(good, only=(2,)) == [-1] and "page 1" in lib.dmx_last_error().decode()
    pt[1].out = 128
    pxt[4].crop_scale += 1                                            # the prepared projective table no longer belongs to its frame
    assert all_four(good, only=(1, 3)) == [-1] * 2 and "item 4" in lib.dmx_last_error().decode()
    pxt[4].crop_scale -= 1
    ppt[0].original = 0
    assert all_four(good, only=(1, 3)) == [-1] * 2 and "page 0" in lib.dmx_last_error().decode()
