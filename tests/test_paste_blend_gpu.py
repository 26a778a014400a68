"""The feathered, colour-matched paste on the GPU (csrc/prepost_blend.hip through prepost.postprocess_batch / _pages / _select_batch /
_select_pages with blend=PasteBlend(...), prepost.paste_color_stats / _pages and dmx_select_choices), on both builds, bit for bit against
the integer restatement (tests/paste_blend_restatement.py) over the cases of tests/paste_blend_cases.py.  Pages of 40 x 56 and 33 x 47 at
S = 16 / 32; the paged pastes write into views of one sentinel-filled slab with guard bands between and around the pages."""
import ctypes

import numpy as np
import pytest
import torch

import paste_blend_cases as PC
import readback_restatement as RB

pytestmark = pytest.mark.gpu

GUARD = 4096
NAMES = [c.name for c in PC.cases()]
MATCHING = [c.name for c in PC.cases() if c.blend.match_color]
THRESHOLD = -2.0


@pytest.fixture(scope="module")
def cases():
    return {c.name: c for c in PC.cases()}


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
    return D.PasteBlend(**c.blend.kwargs())


def _slab(c, fill, cuda):
    """guard | page 0 | guard | page 1 | ... | guard -> (buffer, the pages as views, the guards' slices)"""
    sizes = [p.shape[:2] for p in c.pages]
    buf = torch.full((sum(h * w * 3 for h, w in sizes) + GUARD * (len(sizes) + 1),), fill, dtype=torch.uint8, device=cuda)
    views, guards, off = [], [], 0
    for h, w in sizes:
        guards.append(slice(off, off + GUARD)); off += GUARD
        views.append(buf[off:off + h * w * 3].view(h, w, 3)); off += h * w * 3
    guards.append(slice(off, off + GUARD))
    return buf, views, guards


def _scores(c):
    """a score table whose choice, at THRESHOLD, is c.choice: the chosen candidate scores 0, the others -1, a skipped box -5 throughout"""
    sc = np.full((c.N, c.K), -1.0, dtype=np.float32)
    for b, k in enumerate(c.choice):
        if k < 0:
            sc[b] = -5.0
        else:
            sc[b, k] = 0.0
    assert RB.select(sc, THRESHOLD).tolist() == list(c.choice)
    return sc


def _device(c, cuda):
    imgs = [torch.from_numpy(p.copy()).to(cuda) for p in c.pages]
    rows = torch.from_numpy(c.rows.copy()).to(cuda)
    return imgs, (rows if c.choice is not None else rows[:, 0].contiguous())


def _paste_pages(c, imgs, vae, cuda, out=None):
    """the paged blended paste of a case -> (pages, masks)"""
    from diffute_amd import prepost
    if c.choice is None:
        return prepost.postprocess_pages(vae, imgs, *c.lists(), return_mask=True, out=out, blend=_blend(c))
    got, choice, masks = prepost.postprocess_select_pages(vae, torch.from_numpy(_scores(c)).to(cuda), imgs, *c.lists(), threshold=THRESHOLD,
                                                          return_mask=True, out=out, blend=_blend(c))
    assert choice.dtype == torch.int32 and choice.cpu().tolist() == list(c.choice)
    return got, masks


@pytest.mark.parametrize("name", NAMES)
def test_blended_paste_is_the_restatement(cuda, build, cases, expected, name):
    import diffute_amd as D
    from diffute_amd import prepost
    c, exp = cases[name], expected[name]
    imgs, vae = _device(c, cuda)
    for fill in (0, 255):                                  # a byte nobody wrote shows under one fill or the other
        buf, views, guards = _slab(c, fill, cuda)
        got, masks = _paste_pages(c, imgs, vae, cuda, views)
        D.synchronize()
        assert all(g.data_ptr() == v.data_ptr() for g, v in zip(got, views))
        assert all(bool((buf[g] == fill).all()) for g in guards), "a guard band was written"
        for p, (want, want_mask, _) in enumerate(exp):
            host, mask = got[p].cpu().numpy(), masks[p].cpu().numpy()
            assert np.array_equal(mask, want_mask), f"{name}: union mask of page {p}"
            bad = np.argwhere((host != want).any(axis=2))
            assert bad.size == 0, f"{name}: page {p} differs from the restatement at {len(bad)} pixels, the first (y, x) = {bad[0].tolist()}"
            assert np.array_equal(host[mask == 0], c.pages[p][mask == 0]), "out == original wherever the mask is 0"
    again, masks2 = _paste_pages(c, imgs, vae, cuda)         # pages of its own, a second run: the same bytes
    assert all(torch.equal(a, b) for a, b in zip(again, got)) and all(torch.equal(a, b) for a, b in zip(masks2, masks))
    if len(c.pages) == 1:                                  # the one-page entry
        one = [l[0] for l in c.lists()]
        if c.choice is None:
            out, mask = prepost.postprocess_batch(vae, imgs[0], *one, return_mask=True, blend=_blend(c))
        else:
            out, choice, mask = prepost.postprocess_select_batch(vae, torch.from_numpy(_scores(c)).to(cuda), imgs[0], *one, threshold=THRESHOLD,
                                                                 return_mask=True, blend=_blend(c))
            assert choice.cpu().tolist() == list(c.choice)
        D.synchronize()
        assert torch.equal(out, got[0]) and torch.equal(mask, masks[0]), f"{name}: the one-page entry differs from the paged one"


@pytest.mark.parametrize("name", MATCHING)
def test_color_stats_are_the_restatement(cuda, build, cases, expected, name):
    """n and the clamped D of every item, from the paged entry and (one page) from the one-page entry; then every item ALONE in a table
    of one - the same four numbers"""
    import diffute_amd as D
    from diffute_amd import prepost
    c = cases[name]
    want = np.array([s for _, _, stats in expected[name] for s in stats], dtype=np.int64)
    imgs, vae = _device(c, cuda)
    choice = None if c.choice is None else torch.tensor(c.choice, dtype=torch.int32, device=cuda)
    got = prepost.paste_color_stats_pages(vae, imgs, *c.lists(), _blend(c), choice=choice)
    D.synchronize()
    assert got.dtype == torch.int64 and got.shape == (c.N, 4)
    assert np.array_equal(got.cpu().numpy(), want), f"{name}: stats differ from the restatement"
    if len(c.pages) == 1:
        one = prepost.paste_color_stats(vae, imgs[0], *[l[0] for l in c.lists()], _blend(c), choice=choice)
        assert torch.equal(one, got)
    boxes, origins, crops = c.lists()
    b = 0
    for p in range(len(c.pages)):
        for j in range(len(boxes[p])):
            if b % 9 == 0 or c.N <= 3:                     # (b64: every ninth item)
                ch = None if choice is None else choice[b:b + 1].contiguous()
                alone = prepost.paste_color_stats(vae[b:b + 1], imgs[p], [boxes[p][j]], [origins[p][j]], [crops[p][j]], _blend(c), choice=ch)
                assert torch.equal(alone[0], got[b]), f"{name}: item {b} alone against item {b} in the batch"
            b += 1


@pytest.mark.parametrize("name", [n for n in NAMES if n != "k2_choice_skip"])
def test_everything_off_is_the_existing_paste(cuda, build, cases, name):
    """PasteBlend() over the geometry of every case against blend=None: the same page from both entries (the masks differ by definition:
    inclusive boxes there, paste rectangles here)"""
    import diffute_amd as D
    from diffute_amd import prepost
    c = cases[name]
    imgs, vae = _device(c, cuda)
    plain = prepost.postprocess_pages(vae, imgs, *c.lists())
    off, masks = prepost.postprocess_pages(vae, imgs, *c.lists(), return_mask=True, blend=D.PasteBlend())
    D.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(plain, off)), name
    for p, (img, got, mask) in enumerate(zip(imgs, off, masks)):
        assert torch.equal(got[mask == 0], img[mask == 0])
    if len(c.pages) == 1:
        one = [l[0] for l in c.lists()]
        assert torch.equal(prepost.postprocess_batch(vae, imgs[0], *one, blend=D.PasteBlend()), prepost.postprocess_batch(vae, imgs[0], *one))


def test_everything_off_with_a_choice_is_the_existing_select_paste(cuda, build, cases):
    import diffute_amd as D
    from diffute_amd import prepost
    c = cases["k2_choice_skip"]
    imgs, vae = _device(c, cuda)
    sc = torch.from_numpy(_scores(c)).to(cuda)
    one = [l[0] for l in c.lists()]
    a, ac = prepost.postprocess_select_batch(vae, sc, imgs[0], *one, threshold=THRESHOLD)
    b, bc = prepost.postprocess_select_batch(vae, sc, imgs[0], *one, threshold=THRESHOLD, blend=D.PasteBlend())
    pa, pac = prepost.postprocess_select_pages(vae, sc, imgs, *c.lists(), threshold=THRESHOLD)
    pb, pbc = prepost.postprocess_select_pages(vae, sc, imgs, *c.lists(), threshold=THRESHOLD, blend=D.PasteBlend())
    D.synchronize()
    assert torch.equal(a, b) and torch.equal(ac, bc) and torch.equal(pa[0], pb[0]) and torch.equal(pac, pbc) and torch.equal(a, pa[0])


def test_select_choices_is_the_choice_of_the_select_paste(cuda, build, cases):
    """dmx_select_choices alone against the choice postprocess_select_batch writes: ties, NaNs, a row of NaNs, infinities, thresholds;
    B = 64 with K = 16 fills the score table"""
    from diffute_amd import _cabi, prepost
    nan, inf = float("nan"), float("inf")
    c = cases["k2_choice_skip"]
    imgs, _ = _device(c, cuda)
    one = [l[0] for l in c.lists()]
    lib = _cabi.lib()
    tables = [[[-1.0, -0.5, -2.0], [-0.5, -0.5, -0.5], [nan, -3.0, nan]], [[nan, nan, nan], [-inf, -5.0, -inf], [inf, 1.0, inf]],
              [[-2.0, -1.0, -1.0], [0.0, -0.0, -1.0], [-inf, nan, -inf]]]
    vae = torch.zeros(3, 3, 3, 16, 16, device=cuda)
    for table in tables:
        for thr in (None, -1.0, inf):
            sc = torch.tensor(table, dtype=torch.float32, device=cuda)
            _, want = prepost.postprocess_select_batch(vae, sc, imgs[0], *one, threshold=thr)
            got = torch.full((3 + 2,), 77, dtype=torch.int32, device=cuda)
            _cabi.check(lib.dmx_select_choices(_cabi.ptr(sc), 3, 3, float("-inf") if thr is None else thr, _cabi.ptr(got), _cabi.current_stream()),
                        "select_choices", lib)
            _cabi.synchronize()
            assert got[:3].cpu().tolist() == want.cpu().tolist() == RB.select(np.array(table, np.float32), -np.inf if thr is None else thr).tolist()
            assert got[3:].cpu().tolist() == [77, 77], "written past choice[B]"
    rng = np.random.RandomState(9)
    big = rng.randn(64, 16).astype(np.float32)
    big[rng.rand(64, 16) < 0.2] = nan
    big[5] = nan
    got = torch.empty(64, dtype=torch.int32, device=cuda)
    _cabi.check(lib.dmx_select_choices(_cabi.ptr(torch.from_numpy(big).to(cuda)), 64, 16, 1.5, _cabi.ptr(got), _cabi.current_stream()), "select_choices", lib)
    _cabi.synchronize()
    assert got.cpu().tolist() == RB.select(big, 1.5).tolist()


def test_bad_parameters_are_refused_and_nothing_is_launched(cuda, build, cases):
    """the entries themselves, with real addresses and good tables: a bad blend, a missing stats or choice table - an error, and the
    sentinel-filled outputs keep their sentinel"""
    from diffute_amd import _cabi, prepost
    c = cases["two_pages"]
    imgs, vae = _device(c, cuda)
    boxes, origins, crops = c.lists()
    flat = lambda ll: [x for l in ll for x in l]
    buf, views, guards = _slab(c, 0x5A, cuda)
    stats = torch.full((c.N, 4), 0x5A5A, dtype=torch.int64, device=cuda)
    choice = torch.full((c.N,), 77, dtype=torch.int32, device=cuda)
    host, pages, stage, dbuf, offs = prepost._upload_pages(imgs, flat(boxes), flat(origins), flat(crops), [len(b) for b in boxes], c.S, cuda, views, None)
    one_host, _, one_stage, one_dbuf, _ = prepost._upload(prepost._one_page(imgs[0], boxes[0], origins[0], crops[0]), c.S)
    lib, base, st = _cabi.lib(), dbuf.data_ptr(), _cabi.current_stream()
    h, w = imgs[0].shape[:2]
    one_out = views[0]
    B = _cabi.PasteBlend

    def all_four(bl, stats_in=stats, ch=None, K=1, only=range(4)):
        r = ctypes.byref(bl)
        calls = [lambda: lib.dmx_paste_color_stats_pages(_cabi.ptr(vae), c.S, pages, base + offs[0], 2, host, base, c.N, r, _cabi.ptr(ch), K, _cabi.ptr(stats), st),
                 lambda: lib.dmx_paste_color_stats(_cabi.ptr(vae), c.S, _cabi.ptr(imgs[0]), h, w, one_host, one_dbuf.data_ptr(), 2, r, _cabi.ptr(ch), K,
                                          _cabi.ptr(stats), st),
                 lambda: lib.dmx_postprocess_paste_blend_pages(_cabi.ptr(vae), c.S, pages, base + offs[0], 2, host, base, c.N, r, _cabi.ptr(stats_in),
                                                      _cabi.ptr(ch), K, st),
                 lambda: lib.dmx_postprocess_paste_blend(_cabi.ptr(vae), c.S, _cabi.ptr(imgs[0]), _cabi.ptr(one_out), None, h, w, one_host, one_dbuf.data_ptr(), 2,
                                                r, _cabi.ptr(stats_in), _cabi.ptr(ch), K, st)]
        return [calls[i]() for i in only]
    for bl in (B(-1, 0, 8, 32, 0), B(0, -1, 8, 32, 0), B(0, 0, 0, 32, 0), B(0, 0, 8, 256, 1), B(_cabi.PASTE_BLEND_MAX + 1, 0, 8, 32, 0), B(1, 1, 8, 32, 2)):
        assert all(rc == -1 for rc in all_four(bl)), "a bad blend was accepted"
    assert all(rc == -1 for rc in all_four(B(1, 1, 8, 32, 1), K=2)), "K = 2 without a choice table"
    assert all(rc == -1 for rc in all_four(B(1, 1, 8, 32, 1), ch=choice, K=17))
    assert all(rc == -1 for rc in all_four(B(1, 1, 8, 32, 1), stats_in=None, only=(2, 3))), "match_color without stats"
    host[2].y_s = 33                                       # the first row below page 1: the plain entries' table checks apply unchanged
    assert all_four(B(1, 1, 8, 32, 0), only=(0, 2)) == [-1, -1] and "item 2" in lib.dmx_last_error().decode()
    assert lib.dmx_select_choices(_cabi.ptr(vae), c.N, 17, 0.0, _cabi.ptr(choice), st) == -1
    assert lib.dmx_select_choices(_cabi.ptr(vae), 65, 2, 0.0, _cabi.ptr(choice), st) == -1
    assert lib.dmx_select_choices(_cabi.ptr(vae), c.N, 2, float("nan"), _cabi.ptr(choice), st) == -1
    _cabi.synchronize()
    assert bool((buf == 0x5A).all()) and bool((stats == 0x5A5A).all()) and bool((choice == 77).all()), "refused, yet something was written"
