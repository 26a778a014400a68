"""Quadrilateral regions in perspective on the GPU (csrc/prepost_quad.hip through prepost.preprocess_quads / postprocess_quads /
rectify_quads with perspective=True, and pipeline.edit_quads(perspective=True)) against the numpy restatement of csrc/prepost_persp.h
(tests/persp_restatement.py, fed with the integers the prepare entries filled) - bit exact, on both builds.  The cases are
tests/persp_cases.py: nine quads on three pages in one launch at S = 64 - trapezoids narrowing to the right and upwards, a general quad
across the paste's 256-column tile, an exact copy, two overlapping quads, a line read top to bottom, a window overhanging its page, a
parallelogram, a quad four pixels thin.  The paste writes into views of one sentinel-filled slab with guard bands."""
import numpy as np
import pytest
import torch

import persp_cases as PC
import persp_restatement as PR
import quad_cases as QC
import quad_restatement as QR
from test_models_gpu import TINY_UNET, TINY_VAE

pytestmark = pytest.mark.gpu

S, N, PAGES = PC.S, PC.N, PC.PAGES
GUARD = 4096


@pytest.fixture(scope="module")
def ref():
    """pages, decoder outputs, the prepared integers and the restatement's results, computed once and only read afterwards"""
    from diffute_amd import _cabi
    rs = np.random.RandomState(20261020)
    pages = [rs.randint(0, 256, (h, w, 3), dtype=np.uint8) for h, w in PAGES]
    vae = (rs.standard_normal((N, 3, S, S)) * 0.6).clip(-1.3, 1.3).astype(np.float32)      # some values leave [-1, 1]
    quads, frames = PC.lists()
    pt, qt, xt = PC.tables(PAGES, quads, frames)
    _cabi.check(_cabi.lib().dmx_edit_quads_prepare(pt, len(PAGES), qt, N, S), "edit_quads_prepare")
    _cabi.check(_cabi.lib().dmx_edit_quads_persp_prepare(pt, len(PAGES), qt, xt, N, S), "edit_quads_persp_prepare")
    qs, pms = [QR.from_table(q) for q in qt], [PR.from_table(x) for x in xt]
    pre = [PR.preprocess(pages[q["page"]], q, pm, S) for q, pm in zip(qs, pms)]
    strips = [PR.rectify(pages[q["page"]], q, pm) for q, pm in zip(qs, pms)]
    pastes = []
    for p in range(len(PAGES)):
        mine = [b for b, q in enumerate(qs) if q["page"] == p]
        pastes.append(PR.paste_page(pages[p], [qs[b] for b in mine], [pms[b] for b in mine], [vae[b] for b in mine], S))
    for a in pages + [vae] + strips + [v for d in pre + pastes for v in d.values()]:
        a.setflags(write=False)
    return dict(pages=pages, vae=vae, quads=quads, frames=frames, qs=qs, pms=pms, pre=pre, strips=strips, pastes=pastes)


@pytest.fixture(params=["bf16", "fp16"])
def build(request, monkeypatch, cuda):
    """route every prepost call of the test through one build of the library"""
    from diffute_amd import _cabi
    real = _cabi.lib
    real(request.param)
    monkeypatch.setattr(_cabi, "lib", lambda elem=None: real(request.param))
    return request.param


def _dev(arrays, cuda):
    return [torch.from_numpy(np.ascontiguousarray(a).copy()).to(cuda) for a in arrays]


def _slab(fill, cuda, sizes=PAGES):
    """one sentinel-filled uint8 buffer: guard | page 0 | guard | page 1 | ... | guard -> (buffer, the pages as views, the guards' slices)"""
    n = sum(h * w * 3 for h, w in sizes) + GUARD * (len(sizes) + 1)
    buf = torch.full((n,), fill, dtype=torch.uint8, device=cuda)
    views, guards, off = [], [], 0
    for h, w in sizes:
        guards.append(slice(off, off + GUARD)); off += GUARD
        views.append(buf[off:off + h * w * 3].view(h, w, 3)); off += h * w * 3
    guards.append(slice(off, off + GUARD))
    return buf, views, guards


def test_reference_covers_what_the_cases_claim(ref):
    """the restatement's own results show the cases do what their names say (no GPU work)"""
    hit0 = ref["pastes"][0]["hit"]
    Y, X = np.mgrid[0:PAGES[0][0], 0:PAGES[0][1]]
    both = QR.inside(ref["qs"][0], X, Y) & QR.inside(ref["qs"][4], X, Y)
    assert both.sum() > 50 and (hit0[both] == 4).all(), "trap_right and overlap overlap, and the later one decides there"
    assert all(p["pasted"].sum() > 0 for p in ref["pastes"]) and all(0 < d["mask"].sum() < S * S for d in ref["pre"])
    assert (ref["pastes"][2]["hit"] == 1).sum() > 300, "thin has pixels of its own"
    pasted_all = all(np.array_equal(p["pasted"], p["hit"] >= 0) for p in ref["pastes"])
    assert pasted_all, "every window covers its quad: what is masked is pasted"


def test_preprocess_quads_rows(cuda, build, ref):
    import diffute_amd as D
    imgs = _dev(ref["pages"], cuda)
    got = D.prepost.preprocess_quads(imgs, ref["quads"], ref["frames"], size=S, perspective=True)
    D.synchronize()
    assert sorted(got) == ["image", "mask", "mask_latent", "masked_image"]
    assert got["image"].shape == (N, 3, S, S) and got["masked_image"].shape == (N, 3, S, S) and got["image"].dtype == torch.float32
    assert got["mask"].shape == (N, 1, S, S) and got["mask"].dtype == torch.uint8 and got["mask_latent"].shape == (N, 1, S // 8, S // 8)
    host = {k: v.cpu().numpy() for k, v in got.items()}
    for b, (p, (name, _, _, _)) in enumerate(PC.FLAT):
        want = ref["pre"][b]
        for k in ("image", "masked_image"):
            assert np.array_equal(host[k][b].view(np.uint32), want[k].view(np.uint32)), f"{name}: {k} of row {b} (page {p}) differs from the restatement"
        for k in ("mask", "mask_latent"):
            assert np.array_equal(host[k][b, 0], want[k]), f"{name}: {k} of row {b} (page {p}) differs from the restatement"
    assert torch.equal(got["image"][3], (imgs[0][10:74, 15:79].permute(2, 0, 1).float() - 127.5) * (1.0 / 127.5)), "axis_copy is the page slice"


def test_postprocess_quads_pages_and_union_masks(cuda, build, ref):
    import diffute_amd as D
    imgs, vae = _dev(ref["pages"], cuda), torch.from_numpy(ref["vae"].copy()).to(cuda)
    for fill in (0, 255):                                  # a byte nobody wrote shows under one fill or the other
        buf, views, guards = _slab(fill, cuda)
        got, unions = D.prepost.postprocess_quads(vae, imgs, ref["quads"], ref["frames"], return_mask=True, out=views, perspective=True)
        D.synchronize()
        assert all(g.data_ptr() == v.data_ptr() for g, v in zip(got, views))
        assert all(bool((buf[g] == fill).all()) for g in guards), "a guard band between the pages was written"
        for p, want in enumerate(ref["pastes"]):
            host = got[p].cpu().numpy()
            assert host.shape == PAGES[p] + (3,) and got[p].dtype == torch.uint8
            assert np.array_equal(host, want["out"]), f"page {p} differs from the restatement"
            assert np.array_equal(unions[p].cpu().numpy(), want["union"]), f"union mask of page {p} differs from the OR of the quads"
            outside = want["union"] == 0
            assert outside.sum() > 1000 and np.array_equal(host[outside], ref["pages"][p][outside]), "pixels outside every quad must be untouched"
            assert (host[want["pasted"]] != ref["pages"][p][want["pasted"]]).any()
    plain = D.prepost.postprocess_quads(vae, imgs, ref["quads"], ref["frames"], perspective=True)     # pages of its own, no mask: the same bytes
    assert all(torch.equal(a, b) for a, b in zip(plain, got))


def test_rectify_quads_strips(cuda, build, ref):
    import diffute_amd as D
    imgs = _dev(ref["pages"], cuda)
    got = D.prepost.rectify_quads(imgs, ref["quads"], perspective=True)
    D.synchronize()
    assert len(got) == N and all(t.dtype == torch.uint8 and t.is_cuda and t.is_contiguous() for t in got)
    base = got[0].data_ptr()
    for b, (t, want, q) in enumerate(zip(got, ref["strips"], ref["qs"])):
        assert t.data_ptr() - base == q["rect_off"], "the strips are views of one buffer, packed in item order"
        assert tuple(t.shape) == (q["rh"], q["rw"], 3) and np.array_equal(t.cpu().numpy(), want), f"{PC.FLAT[b][1][0]}: strip {b} differs from the restatement"
    assert torch.equal(got[3], imgs[0][20:33, 20:51]), "an axis-aligned quad is the page slice, both corners included"
    flat = D.prepost.rectify_quads(imgs, ref["quads"])
    assert [tuple(t.shape) for t in flat] == [tuple(t.shape) for t in got] and not torch.equal(flat[0], got[0]), "the similarity strip keeps the keystone"


def test_a_quarter_turn_of_pages_and_quads(cuda, build, ref):
    """np.rot90 of every page with its quads turned along (the frames live in strip space and stay), in one launch each: the crops,
    masks and strips are identical and the pasted page is the turned pasted page, bit for bit - the crop coordinates of a page pixel
    are the same integers, so the fp32 paste is the same arithmetic"""
    import diffute_amd as D
    P = D.prepost
    imgs, vae = _dev(ref["pages"], cuda), torch.from_numpy(ref["vae"].copy()).to(cuda)
    timgs = _dev([QR.rot90_page(p) for p in ref["pages"]], cuda)
    tquads = [[QR.rot90_corners(c, w) for c in cs] for cs, (h, w) in zip(ref["quads"], PAGES)]
    a = P.preprocess_quads(imgs, ref["quads"], ref["frames"], size=S, perspective=True)
    b = P.preprocess_quads(timgs, tquads, ref["frames"], size=S, perspective=True)
    assert all(torch.equal(a[k], b[k]) for k in a), "the crops of the turned pages differ"
    sa, sb = P.rectify_quads(imgs, ref["quads"], perspective=True), P.rectify_quads(timgs, tquads, perspective=True)
    assert all(torch.equal(x, y) for x, y in zip(sa, sb)), "the strips of the turned pages differ"
    pa, ua = P.postprocess_quads(vae, imgs, ref["quads"], ref["frames"], return_mask=True, perspective=True)
    pb, ub = P.postprocess_quads(vae, timgs, tquads, ref["frames"], return_mask=True, perspective=True)
    D.synchronize()
    for p in range(len(PAGES)):
        assert np.array_equal(np.rot90(ua[p].cpu().numpy()), ub[p].cpu().numpy())
        assert np.array_equal(np.rot90(pa[p].cpu().numpy()), pb[p].cpu().numpy()), f"page {p}: the pasted turned page is not the turned pasted page"


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
    """perspective=True: the two prepares and one launch of the projective entry; perspective=False: the quad entries, and what they
    return today - the restatement of csrc/prepost_quad.h, bit for bit"""
    import diffute_amd as D
    from diffute_amd import _cabi
    names = []
    rec = _Recorder(_cabi.lib(), names)
    monkeypatch.setattr(_cabi, "lib", lambda elem=None: rec)
    imgs, vae = _dev(ref["pages"], cuda), torch.from_numpy(ref["vae"].copy()).to(cuda)
    Q, F = ref["quads"], ref["frames"]
    calls = [("dmx_preprocess_quads_persp", lambda: D.prepost.preprocess_quads(imgs, Q, F, size=S, perspective=True)),
             ("dmx_postprocess_paste_quads_persp", lambda: D.prepost.postprocess_quads(vae, imgs, Q, F, return_mask=True, perspective=True)),
             ("dmx_rectify_quads_persp", lambda: D.prepost.rectify_quads(imgs, Q, perspective=True)),
             ("dmx_preprocess_quads_persp", lambda: D.prepost.preprocess_quads(imgs[:1], Q[:1], F[:1], size=S, perspective=True))]      # one page is P = 1
    for entry, fn in calls:
        del names[:]
        fn()
        assert names == ["dmx_edit_quads_prepare", "dmx_edit_quads_persp_prepare", entry], entry
    del names[:]
    planned = D.prepost.preprocess_quads(imgs, Q, None, size=S, perspective=True)                 # frames None: planned on the host, then the same three
    assert names[-3:] == ["dmx_edit_quads_prepare", "dmx_edit_quads_persp_prepare", "dmx_preprocess_quads_persp"]
    assert set(names[:-3]) <= {"dmx_edit_quads_prepare", "dmx_edit_quads_persp_prepare", "dmx_last_error"} and planned["image"].shape == (N, 3, S, S)
    # the similarity path, asked for by name: the old entries, the old bytes
    sq, sf = QC.lists()
    sim_f = [[f for f in fs] for fs in sf]
    simgs = imgs
    old = [("dmx_preprocess_quads", lambda: D.prepost.preprocess_quads(simgs, sq, sim_f, size=S, perspective=False)),
           ("dmx_postprocess_paste_quads", lambda: D.prepost.postprocess_quads(vae, simgs, sq, sim_f, perspective=False)),
           ("dmx_rectify_quads", lambda: D.prepost.rectify_quads(simgs, sq, perspective=False))]
    res = []
    for entry, fn in old:
        del names[:]
        res.append(fn())
        assert names == ["dmx_edit_quads_prepare", entry], entry
    D.synchronize()
    pt, qt = QC.tables(PAGES, sq, sim_f)
    _cabi.check(rec.dmx_edit_quads_prepare(pt, 3, qt, QC.N, S), "edit_quads_prepare")
    qs = [QR.from_table(q) for q in qt]
    for b, q in enumerate(qs):
        want = QR.preprocess(ref["pages"][q["page"]], q, S)
        assert np.array_equal(res[0]["image"][b].cpu().numpy().view(np.uint32), want["image"].view(np.uint32)) and np.array_equal(res[0]["mask"][b, 0].cpu().numpy(), want["mask"])
        assert np.array_equal(res[2][b].cpu().numpy(), QR.rectify(ref["pages"][q["page"]], q))
    for p in range(3):
        mine = [b for b, q in enumerate(qs) if q["page"] == p]
        want = QR.paste_page(ref["pages"][p], [qs[b] for b in mine], [ref["vae"][b] for b in mine], S)
        assert np.array_equal(res[1][p].cpu().numpy(), want["out"])


def test_refusals_launch_nothing(cuda, ref):
    """a window the horizon crosses, a window beyond the cap, a strip one pixel high, a missing frame and a host table spoiled after the
    prepare: an error naming the item, and the sentinel-filled outputs stay as they were"""
    from diffute_amd import _cabi, prepost
    imgs, vae = _dev(ref["pages"], cuda), torch.from_numpy(ref["vae"].copy()).to(cuda)
    buf, views, guards = _slab(0x5A, cuda)
    quads, frames = ref["quads"], ref["frames"]

    def swap(p, j, corners, frame):
        qs, fs = [list(q) for q in quads], [list(f) for f in frames]
        qs[p][j], fs[p][j] = corners, frame
        return qs, fs
    H = PC.HORIZON_QUAD
    cases = [(swap(0, 1, H, PC.frame_of(H, 240)), "item 1"), (swap(0, 2, H, PC.frame_of(H, 150)), "item 2"),
             (swap(2, 0, PC.FLAT_STRIP_QUAD, PC.frame_of(PC.FLAT_STRIP_QUAD, 64)), "item 7"), (swap(1, 1, quads[1][1], (58, 13, 0)), "item 6")]
    for (q, f), word in cases:
        with pytest.raises(RuntimeError, match=word):
            prepost.postprocess_quads(vae, imgs, q, f, out=views, perspective=True)
        with pytest.raises(RuntimeError, match=word):
            prepost.preprocess_quads(imgs, q, f, size=S, perspective=True)
    for (q, f), word in cases[:3:2]:                       # the strips read no window: the horizon quad's own strip and the flat one
        with pytest.raises(RuntimeError, match=word):
            prepost.rectify_quads(imgs, q, perspective=True)
    with pytest.raises(ValueError, match="page 1: quad 1"):
        prepost.preprocess_quads(imgs, quads, [frames[0], [frames[1][0], None], frames[2]], size=S, perspective=True)
    # the launch entries themselves, with real addresses and good device tables: only the host tables are spoiled
    lib = _cabi.lib()
    qx = prepost._check_quads(imgs, quads, frames, True)
    strips = torch.full((1 << 16,), 0x5A, dtype=torch.uint8, device=cuda)
    pre_out = [torch.full((N * 3 * S * S,), 3.0, device=cuda), torch.full((N * 3 * S * S,), 3.0, device=cuda),
               torch.full((N * S * S,), 0x5A, dtype=torch.uint8, device=cuda), torch.full((N * 64,), 3.0, device=cuda)]
    for spoil in ("map", "quad", "page"):
        host, pages, persp, stage, dbuf, off, xoff = prepost._upload_quads(qx, S, views, None)
        if spoil == "map":
            persp[6].strip.t[0] += 1
            persp[6].crop.t[6] += 1
        elif spoil == "quad":
            host[6].x[0] = 131                                 # the first column right of page 1
        else:
            pages[1].W = 300                                   # another tile count: the blocks no longer belong to the table
        base, word = dbuf.data_ptr(), ("page 1" if spoil == "page" else "item 6")
        assert lib.dmx_postprocess_paste_quads_persp(_cabi.ptr(vae), S, pages, base + off, 3, host, base, persp, base + xoff, N, _cabi.current_stream()) == -1
        assert word in lib.dmx_last_error().decode()
        assert lib.dmx_preprocess_quads_persp(pages, base + off, 3, host, base, persp, base + xoff, N, S, *(_cabi.ptr(t) for t in pre_out),
                                              _cabi.current_stream()) == -1
        assert word in lib.dmx_last_error().decode()
        assert lib.dmx_rectify_quads_persp(pages, base + off, 3, host, base, persp, base + xoff, N, _cabi.ptr(strips), strips.numel(),
                                           _cabi.current_stream()) == -1
        assert word in lib.dmx_last_error().decode()
    _cabi.synchronize()
    assert bool((buf == 0x5A).all()) and bool((strips == 0x5A).all()) and bool((pre_out[2] == 0x5A).all()), "refused, yet something was written"
    assert all(bool((t == 3.0).all()) for t in (pre_out[0], pre_out[1], pre_out[3]))


# ---- pipeline.edit_quads(perspective=True) on the tiny models: S = 128, two pages with 2 + 1 trapezoids, batch_size=2 (the first chunk
# spans both pages, the last has one row)
ES, ESTEPS, EBS = 128, 2, 2
EPAGES = [(320, 384), (384, 200)]
EQUADS = [[[(60, 80), (220, 92), (220, 124), (60, 140)], [(200, 220), (330, 216), (334, 252), (196, 244)]],
          [[(120, 60), (124, 200), (96, 196), (84, 64)]]]        # the last one is read top to bottom
EN = 3


def test_edit_quads_in_perspective_is_the_manual_chain(cuda):
    import diffute_amd as D
    from diffute_amd.init import normal
    unet = D.UNet2DConditionModel(**TINY_UNET).cuda().requires_grad_(False)
    vae = D.AutoencoderKL(**TINY_VAE).cuda().requires_grad_(False)
    rs = np.random.RandomState(12)
    imgs = [torch.from_numpy(rs.randint(0, 256, (h, w, 3), dtype=np.uint8)).to(cuda) for h, w in EPAGES]
    ctx = normal(2, 13, EN * 77 * 128, cuda).reshape(EN, 77, 128)
    enc_noise = normal(4, 71, EN * 4 * 16 * 16, cuda).reshape(EN, 4, 16, 16)
    frames = D.prepost.plan_quads(EQUADS, EPAGES, perspective=True, size=ES)
    assert all(len(f) == 3 for fs in frames for f in fs)
    kw = dict(batch_size=EBS, enc_noise=enc_noise, size=ES)
    out, image_vae, pre = D.edit_quads(unet, vae, D.DDIMScheduler(), imgs, EQUADS, ctx, ESTEPS, return_intermediate=True, perspective=True, **kw)   # frames planned
    want_pre = D.prepost.preprocess_quads(imgs, EQUADS, frames, size=ES, perspective=True)
    assert sorted(pre) == sorted(want_pre) and all(torch.equal(pre[k], want_pre[k]) for k in pre)
    init = torch.randn((1, 4, ES // 8, ES // 8), generator=torch.manual_seed(0), dtype=torch.float32).to(cuda)
    chunks = []
    for lo in range(0, EN, EBS):
        hi = min(EN, lo + EBS)
        chunks.append(D.edit_latents(unet, vae, D.DDIMScheduler(), want_pre["image"][lo:hi], want_pre["masked_image"][lo:hi], want_pre["mask"][lo:hi],
                                     ctx[lo:hi], ESTEPS, init_latents=init.expand(hi - lo, -1, -1, -1).contiguous(), enc_noise=enc_noise[lo:hi]).clone())
    want_vae = torch.cat(chunks, 0)
    assert image_vae.shape == (EN, 3, ES, ES) and torch.equal(image_vae, want_vae), "image_vae differs from edit_latents over the chunks"
    want = D.prepost.postprocess_quads(want_vae, imgs, EQUADS, frames, perspective=True)
    D.synchronize()
    for p, (h, w) in enumerate(EPAGES):
        assert out[p].shape == (h, w, 3) and out[p].dtype == torch.uint8 and torch.equal(out[p], want[p]), f"page {p}"
        Y, X = np.mgrid[0:h, 0:w]
        covered = np.zeros((h, w), bool)
        for c in EQUADS[p]:
            covered |= QR.inside(QR.derive(c, (0, 0, 1, 1, 0), 1), X, Y)
        covered = torch.from_numpy(covered).to(cuda)
        assert torch.equal(out[p][~covered], imgs[p][~covered]), "pixels outside all quads must be untouched"
        assert (out[p][covered] != imgs[p][covered]).any() and int(covered.sum()) > 1000
    given = D.edit_quads(unet, vae, D.DDIMScheduler(), imgs, EQUADS, ctx, ESTEPS, frames=frames, perspective=True, **kw)
    assert isinstance(given, list) and all(torch.equal(a, b) for a, b in zip(given, out))
    # perspective=False is the call without the argument - the similarity frames, another result
    a = D.edit_quads(unet, vae, D.DDIMScheduler(), imgs, EQUADS, ctx, 1, perspective=False, **kw)
    b = D.edit_quads(unet, vae, D.DDIMScheduler(), imgs, EQUADS, ctx, 1, **kw)
    D.synchronize()
    assert all(torch.equal(x, y) for x, y in zip(a, b)) and not all(torch.equal(x, y) for x, y in zip(a, out))
