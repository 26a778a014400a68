"""The feathered, colour-matched paste for quads on the GPU (csrc/prepost_quad_blend.hip through prepost.postprocess_quads /
postprocess_select_quads with blend=QuadBlend(...), prepost.paste_color_stats_quads and dmx_select_choices), on both builds and in both
frames, bit for bit against the integer restatement (tests/quad_blend_restatement.py) over the cases of tests/quad_blend_cases.py:
thirteen quads on pages of 150 x 300, 97 x 131 and 70 x 260 at S = 64, every case in one launch per stage.  The pastes write into views of
one sentinel-filled slab with guard bands between and around the pages."""
import ctypes

import numpy as np
import pytest
import torch

import quad_blend_cases as BC
import quad_blend_restatement as QB
import readback_restatement as RB

pytestmark = pytest.mark.gpu

S, PAGES, K = BC.S, BC.PAGES, BC.K
GUARD = 4096
THRESHOLD = -2.0
NAMES = [f"{kind}-{b}" for kind in ("sim", "persp") for b in list(BC.BLENDS) + ["choice_k3"]]
MATCHING = [n for n in NAMES if "match" in n or "choice" in n or "grow_lt" in n]


@pytest.fixture(scope="module")
def cases():
    cs = {c.name: c for c in BC.cases()}
    assert list(cs) == NAMES and [n for n, c in cs.items() if c.blend.match_color] == MATCHING
    return cs


@pytest.fixture(scope="module")
def expected(cases):
    """the restatement's pages, masks and statistics: computed once, only read afterwards"""
    exp = {name: c.expected() for name, c in cases.items()}
    for pages in exp.values():
        for out, mask, _ in pages:
            out.setflags(write=False); mask.setflags(write=False)
    return exp


@pytest.fixture(params=["bf16", "fp16"])
def build(request, monkeypatch, cuda):
    """route every prepost call of the test through one build of the library"""
    from diffute_amd import _cabi
    real = _cabi.lib
    real(request.param)
    monkeypatch.setattr(_cabi, "lib", lambda elem=None: real(request.param))
    return request.param


def _blend(c):
    import diffute_amd as D
    return D.QuadBlend(**c.blend.kwargs())


def _slab(sizes, fill, cuda):
    """guard | page 0 | guard | page 1 | ... | guard -> (buffer, the pages as views, the guards' slices)"""
    buf = torch.full((sum(h * w * 3 for h, w in sizes) + GUARD * (len(sizes) + 1),), fill, dtype=torch.uint8, device=cuda)
    views, guards, off = [], [], 0
    for h, w in sizes:
        guards.append(slice(off, off + GUARD)); off += GUARD
        views.append(buf[off:off + h * w * 3].view(h, w, 3)); off += h * w * 3
    guards.append(slice(off, off + GUARD))
    return buf, views, guards


def _scores(c):
    """a score table whose choice, at THRESHOLD, is c.choice: the chosen candidate scores 0, the others -1, a skipped quad -5 throughout"""
    sc = np.full((c.N, K), -1.0, dtype=np.float32)
    for b, k in enumerate(c.choice):
        if k < 0:
            sc[b] = -5.0
        else:
            sc[b, k] = 0.0
    assert RB.select(sc, THRESHOLD).tolist() == list(c.choice)
    return sc


def _device(c, cuda, pages=None):
    imgs = [torch.from_numpy(np.ascontiguousarray(p).copy()).to(cuda) for p in (c.pages if pages is None else pages)]
    rows = torch.from_numpy(c.rows.copy()).to(cuda)
    return imgs, (rows if c.choice is not None else rows[:, 0].contiguous())


def _paste(c, imgs, vae, cuda, out=None, quads=None, frames=None):
    """the blended paste of a case -> (pages, masks)"""
    from diffute_amd import prepost
    quads, frames = (c.quads if quads is None else quads), (c.frames if frames is None else frames)
    if c.choice is None:
        return prepost.postprocess_quads(vae, imgs, quads, frames, return_mask=True, out=out, perspective=c.persp, blend=_blend(c))
    got, choice, masks = prepost.postprocess_select_quads(vae, torch.from_numpy(_scores(c)).to(cuda), imgs, quads, frames, threshold=THRESHOLD,
                                                          return_mask=True, out=out, perspective=c.persp, blend=_blend(c))
    assert choice.dtype == torch.int32 and choice.cpu().tolist() == list(c.choice)
    return got, masks


def _stats(c, imgs, vae, cuda, quads=None, frames=None):
    from diffute_amd import prepost
    choice = None if c.choice is None else torch.tensor(c.choice, dtype=torch.int32, device=cuda)
    return prepost.paste_color_stats_quads(vae, imgs, c.quads if quads is None else quads, c.frames if frames is None else frames, _blend(c),
                                           choice=choice, perspective=c.persp)


@pytest.mark.parametrize("name", NAMES)
def test_blended_quad_paste_is_the_restatement(cuda, build, cases, expected, name):
    """pages and union masks of every case, one launch per stage, into a guarded slab under two fills: every output element is written,
    no guard byte is; the K = 3 cases choose on the device (dmx_select_choices) and skip a quad"""
    import diffute_amd as D
    c, exp = cases[name], expected[name]
    imgs, vae = _device(c, cuda)
    for fill in (0, 255):                                  # a byte nobody wrote shows under one fill or the other
        buf, views, guards = _slab(PAGES, fill, cuda)
        got, masks = _paste(c, imgs, vae, cuda, views)
        D.synchronize()
        assert all(g.data_ptr() == v.data_ptr() for g, v in zip(got, views))
        assert all(bool((buf[g] == fill).all()) for g in guards), "a guard band was written"
        for p, (want, want_mask, _) in enumerate(exp):
            host, mask = got[p].cpu().numpy(), masks[p].cpu().numpy()
            assert mask.dtype == np.uint8 and np.array_equal(mask, want_mask), f"{name}: union mask of page {p}"
            bad = np.argwhere((host != want).any(axis=2))
            assert bad.size == 0, f"{name}: page {p} differs from the restatement at {len(bad)} pixels, the first (y, x) = {bad[0].tolist()}"
            assert np.array_equal(host[mask == 0], c.pages[p][mask == 0]), "out == original wherever the mask is 0"
    again, masks2 = _paste(c, imgs, vae, cuda)               # pages of its own, a second run: the same bytes
    assert all(torch.equal(a, b) for a, b in zip(again, got)) and all(torch.equal(a, b) for a, b in zip(masks2, masks))


@pytest.mark.parametrize("name", MATCHING)
def test_quad_color_stats_are_the_restatement(cuda, build, cases, expected, name):
    """n and the clamped D of every item in one launch, behind a guard; then items ALONE in a table of one - the same four numbers"""
    import diffute_amd as D
    from diffute_amd import prepost
    c = cases[name]
    want = np.array([s for _, _, stats in expected[name] for s in stats], dtype=np.int64)
    imgs, vae = _device(c, cuda)
    got = _stats(c, imgs, vae, cuda)
    D.synchronize()
    assert got.dtype == torch.int64 and got.shape == (c.N, 4)
    assert np.array_equal(got.cpu().numpy(), want), f"{name}: stats differ from the restatement"
    b = 0
    for p in range(len(PAGES)):
        for j in range(len(c.quads[p])):
            if b % 3 == 0:
                ch = None if c.choice is None else torch.tensor(c.choice[b:b + 1], dtype=torch.int32, device=cuda)
                alone = prepost.paste_color_stats_quads(vae[b:b + 1], [imgs[p]], [[c.quads[p][j]]], [[c.frames[p][j]]], _blend(c), choice=ch,
                                                        perspective=c.persp)
                assert torch.equal(alone[0], got[b]), f"{name}: item {b} alone against item {b} in the batch"
            b += 1


@pytest.mark.parametrize("name", ["sim-feather_grow_match", "persp-grow_lt_feather"])
def test_a_quad_alone_is_pasted_as_the_restatement_pastes_it_alone(cuda, build, cases, name):
    """a table of one: the overlapped skew_7 alone on its page, against the restatement of that one item"""
    import diffute_amd as D
    from diffute_amd import prepost
    c = cases[name]
    imgs, vae = _device(c, cuda)
    out, mask = prepost.postprocess_quads(vae[1:2], [imgs[0]], [[c.quads[0][1]]], [[c.frames[0][1]]], return_mask=True, perspective=c.persp,
                                          blend=_blend(c))
    D.synchronize()
    want, want_mask, _ = QB.paste_page(c.pages[0], [c.items[1] + (c.rows[1, 0],)], S, c.blend)
    assert np.array_equal(out[0].cpu().numpy(), want) and np.array_equal(mask[0].cpu().numpy(), want_mask)


@pytest.mark.parametrize("name", ["sim-feather_grow_match", "persp-feather_grow_match", "sim-choice_k3", "persp-feather_wide"])
def test_a_quarter_turn_on_the_device(cuda, build, cases, name):
    """np.rot90 of every page with its quads (and similarity frames) turned along: statistics, pages and masks of the turned input are
    the turned outputs, bit for bit"""
    import diffute_amd as D
    c = cases[name]
    imgs, vae = _device(c, cuda)
    tp, tq, tf = BC.rot90_case(c)
    timgs, _ = _device(c, cuda, tp)
    got, masks = _paste(c, imgs, vae, cuda)
    tgot, tmasks = _paste(c, timgs, vae, cuda, quads=tq, frames=tf)
    same_stats = not c.blend.match_color or torch.equal(_stats(c, imgs, vae, cuda), _stats(c, timgs, vae, cuda, quads=tq, frames=tf))
    D.synchronize()
    assert same_stats, f"{name}: the statistics changed under the turn"
    for p in range(len(PAGES)):
        assert np.array_equal(np.rot90(got[p].cpu().numpy()), tgot[p].cpu().numpy()), f"{name}: page {p}: the pasted turned page is not the turned pasted page"
        assert np.array_equal(np.rot90(masks[p].cpu().numpy()), tmasks[p].cpu().numpy())


def test_everything_off_is_the_existing_quad_paste(cuda, build):
    """QuadBlend() against blend=None on the quads that lie on their crops (asserted first, on the CPU): the same pages and masks from the
    paste and, with K = 1, from the select paste"""
    import diffute_amd as D
    from diffute_amd import prepost
    for c in BC.on_crop_cases():
        assert all(QB.covered_off_crop(c.pages[p], c.page_items(p), S) == 0 for p in range(len(PAGES))), "the premise: every quad on its crop"
        imgs, vae = _device(c, cuda)
        plain, pmask = prepost.postprocess_quads(vae, imgs, c.quads, c.frames, return_mask=True, perspective=c.persp)
        off, omask = prepost.postprocess_quads(vae, imgs, c.quads, c.frames, return_mask=True, perspective=c.persp, blend=D.QuadBlend())
        sc = torch.zeros(c.N, 1, device=cuda)
        sel, ch, _ = prepost.postprocess_select_quads(vae[:, None].contiguous(), sc, imgs, c.quads, c.frames, return_mask=True, perspective=c.persp)
        bsel, bch, bmask = prepost.postprocess_select_quads(vae[:, None].contiguous(), sc, imgs, c.quads, c.frames, return_mask=True, perspective=c.persp,
                                                            blend=D.QuadBlend())
        D.synchronize()
        for p in range(len(PAGES)):
            assert torch.equal(plain[p], off[p]) and torch.equal(pmask[p], omask[p]), f"{c.name}: page {p}"
            assert torch.equal(sel[p], bsel[p]) and torch.equal(sel[p], plain[p]) and torch.equal(bmask[p], pmask[p])
            assert not torch.equal(plain[p], imgs[p])
        assert torch.equal(ch, bch)


@pytest.mark.parametrize("persp", [False, True])
def test_a_choice_table_is_clamped_and_a_skipped_quad_is_transparent(cuda, build, cases, persp):
    """the entries themselves with a choice table written by hand: an entry of 7 at K = 3 reads candidate 2, -1 skips - statistics, pages
    and masks against the restatement of the clamped table"""
    import diffute_amd as D
    from diffute_amd import _cabi, prepost
    c = cases[("persp" if persp else "sim") + "-choice_k3"]
    table = list(c.choice)
    table[1], table[4], table[0] = 7, -3, 2
    exp = c.expected(table=table)
    imgs, vae = _device(c, cuda)
    out, union = prepost._page_outputs(imgs, cuda, None, True)
    qx = prepost._check_quads(imgs, c.quads, c.frames, c.persp)
    t = prepost._upload_quads(qx, S, out, union)
    choice = torch.tensor(table, dtype=torch.int32, device=cuda)
    stats = torch.full((c.N + 1, 4), 77, dtype=torch.int64, device=cuda)
    bs = _blend(c)._struct()
    prepost._call_quads("paste_color_stats_quads", t, (_cabi.ptr(vae), S), ctypes.byref(bs), _cabi.ptr(choice), K, _cabi.ptr(stats))
    prepost._call_quads("postprocess_paste_blend_quads", t, (_cabi.ptr(vae), S), ctypes.byref(bs), _cabi.ptr(stats), _cabi.ptr(choice), K)
    D.synchronize()
    assert stats[c.N].tolist() == [77] * 4, "written past stats[B]"
    assert np.array_equal(stats[:c.N].cpu().numpy(), np.array([s for _, _, st in exp for s in st], dtype=np.int64))
    for p, (want, want_mask, _) in enumerate(exp):
        assert np.array_equal(out[p].cpu().numpy(), want) and np.array_equal(union[p].cpu().numpy(), want_mask), f"page {p}"


def test_one_table_upload_per_call(cuda, build, cases, monkeypatch):
    from diffute_amd import prepost
    calls = []
    real = prepost._upload_quads_extra
    monkeypatch.setattr(prepost, "_upload_quads_extra", lambda *a, **kw: (calls.append(1), real(*a, **kw))[1])
    c = cases["sim-feather_grow_match"]
    imgs, vae = _device(c, cuda)
    _paste(c, imgs, vae, cuda)
    assert len(calls) == 1, "[stats ->] paste: one table upload"
    c = cases["persp-choice_k3"]
    imgs, vae = _device(c, cuda)
    _paste(c, imgs, vae, cuda)
    assert len(calls) == 2, "choose -> stats -> paste: one table upload"


def test_bad_parameters_are_refused_and_nothing_is_launched(cuda, build, cases):
    """the entries themselves, with real addresses and good tables: a bad blend, a missing stats or choice table, a spoiled host table -
    an error, and the sentinel-filled outputs keep their sentinel"""
    import diffute_amd as D
    from diffute_amd import _cabi, prepost
    lib, st = _cabi.lib(), _cabi.current_stream()
    Bl = _cabi.PasteBlend
    for name in ("sim-feather_grow_match", "persp-feather_grow_match"):
        c = cases[name]
        imgs, vae = _device(c, cuda)
        buf, views, guards = _slab(PAGES, 0x5A, cuda)
        stats = torch.full((c.N, 4), 0x5A5A, dtype=torch.int64, device=cuda)
        choice = torch.full((c.N,), 77, dtype=torch.int32, device=cuda)
        qx = prepost._check_quads(imgs, c.quads, c.frames, c.persp)
        t = prepost._upload_quads(qx, S, views, None)
        base = t.dbuf.data_ptr()
        tables = (t.pages, base + t.off, len(PAGES), t.host, base) + ((t.persp, base + t.xoff) if c.persp else ())
        sfx = "_persp" if c.persp else ""

        def both(bl, stats_in=stats, ch=None, k=1, only=(0, 1)):
            r = ctypes.byref(bl)
            calls = [lambda: getattr(lib, "dmx_paste_color_stats_quads" + sfx)(_cabi.ptr(vae), S, *tables, c.N, r, _cabi.ptr(ch), k, _cabi.ptr(stats), st),
                     lambda: getattr(lib, "dmx_postprocess_paste_blend_quads" + sfx)(_cabi.ptr(vae), S, *tables, c.N, r, _cabi.ptr(stats_in), _cabi.ptr(ch), k,
                                                                                  st)]
            return [calls[i]() for i in only]
        for bl in (Bl(-1, 0, 8, 32, 0), Bl(0, -1, 8, 32, 0), Bl(0, 0, 0, 32, 0), Bl(0, 0, 8, 256, 1), Bl(1025, 0, 8, 32, 0), Bl(0, 1025, 8, 32, 0),
                   Bl(0, 0, 1025, 32, 0), Bl(1, 1, 8, 32, 2)):
            assert both(bl) == [-1, -1], "a bad blend was accepted"
        good = Bl(3, 4, 5, 12, 1)
        assert both(good, k=2) == [-1, -1], "K = 2 without a choice table"
        assert both(good, ch=choice, k=17) == [-1, -1]
        assert both(good, stats_in=None, only=(1,)) == [-1], "match_color without stats (the stats entry itself would run)"
        t.host[2].x[0] += 1                                # a corner moved under its derived fields
        assert both(good) == [-1, -1] and "item 2" in lib.dmx_last_error().decode()
        t.host[2].x[0] -= 1
        t.pages[1].W = 300                                 # another tile count: the blocks no longer belong to the table
        assert both(good) == [-1, -1] and "page 1" in lib.dmx_last_error().decode()
        for bad in (D.PasteBlend(feather=1), "soft"):
            with pytest.raises((NotImplementedError, TypeError)):
                prepost.postprocess_quads(vae, imgs, c.quads, c.frames, out=views, perspective=c.persp, blend=bad)
        _cabi.synchronize()
        assert bool((buf == 0x5A).all()) and bool((stats == 0x5A5A).all()) and bool((choice == 77).all()), "refused, yet something was written"
