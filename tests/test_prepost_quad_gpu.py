"""Quadrilateral regions with oriented crops on the GPU (csrc/prepost_quad.hip through prepost.preprocess_quads / postprocess_quads /
rectify_quads) against the numpy restatement of csrc/prepost_quad.h (tests/quad_restatement.py, fed with the integers the prepare entry
filled) - bit exact, on both builds.  The cases are tests/quad_cases.py: nine quads on three pages in one launch at S = 64 - axis-aligned,
skews of 7, 30 and -15 degrees, exactly 90 and 180 degrees, a frame overhanging its page, a quad larger than its frame, two overlapping
quads, a quad one pixel thin; two pages cross the paste's 256-column tile.  The paste writes into views of one sentinel-filled slab with
guard bands.  A quarter turn of everything and a round trip over a linear ramp check the geometry without the restatement."""
import math

import numpy as np
import pytest
import torch

import quad_cases as QC
import quad_restatement as QR

pytestmark = pytest.mark.gpu

S, N, PAGES = QC.S, QC.N, QC.PAGES
GUARD = 4096


@pytest.fixture(scope="module")
def ref():
    """pages, decoder outputs, the prepared integers and the restatement's results, computed once and only read afterwards"""
    from diffute_amd import _cabi
    rs = np.random.RandomState(20251020)
    pages = [rs.randint(0, 256, (h, w, 3), dtype=np.uint8) for h, w in PAGES]
    vae = (rs.standard_normal((N, 3, S, S)) * 0.6).clip(-1.3, 1.3).astype(np.float32)      # some values leave [-1, 1]
    quads, frames = QC.lists()
    pt, qt = QC.tables(PAGES, quads, frames)
    _cabi.check(_cabi.lib().dmx_edit_quads_prepare(pt, len(PAGES), qt, N, S), "edit_quads_prepare")
    qs = [QR.from_table(q) for q in qt]
    pre = [QR.preprocess(pages[q["page"]], q, S) for q in qs]
    strips = [QR.rectify(pages[q["page"]], q) for q in qs]
    pastes = []
    for p in range(len(PAGES)):
        mine = [b for b, q in enumerate(qs) if q["page"] == p]
        pastes.append(QR.paste_page(pages[p], [qs[b] for b in mine], [vae[b] for b in mine], S))
    for a in pages + [vae] + strips + [v for d in pre + pastes for v in d.values()]:
        a.setflags(write=False)
    return dict(pages=pages, vae=vae, quads=quads, frames=frames, qs=qs, pre=pre, strips=strips, pastes=pastes)


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
    names = [it[0] for _, it in QC.FLAT]
    hit0 = ref["pastes"][0]["hit"]
    Y, X = np.mgrid[0:PAGES[0][0], 0:PAGES[0][1]]
    both = QR.inside(ref["qs"][1], X, Y) & QR.inside(ref["qs"][2], X, Y)
    assert both.sum() > 50 and (hit0[both] == 2).all(), "skew_7 and skew_30_overlap overlap, and the later one decides there"
    last = ref["pastes"][2]
    mine = last["hit"] == 2
    assert names[8] == "larger_than_frame" and (mine & last["pasted"]).sum() > 500 and (mine & ~last["pasted"]).sum() > 500, "partly unpasted"
    X16, Y16 = QR.frame_coords(ref["qs"][5], S)
    assert names[5] == "overhang" and (Y16 >> 16).max() >= PAGES[1][0] and (X16 >> 16).min() < 0, "the overhanging frame has clamped taps"
    assert names[7] == "thin" and 100 < (last["hit"] == 1).sum() < 260, "about two pixels per column"
    assert all(p["pasted"].sum() > 0 and p["clamped"].sum() >= 0 for p in ref["pastes"])
    assert all(0 < d["mask"].sum() < S * S for d in ref["pre"])


def test_preprocess_quads_rows(cuda, build, ref):
    import diffute_amd as D
    imgs = _dev(ref["pages"], cuda)
    got = D.prepost.preprocess_quads(imgs, ref["quads"], ref["frames"], size=S)
    D.synchronize()
    assert sorted(got) == ["image", "mask", "mask_latent", "masked_image"]
    assert got["image"].shape == (N, 3, S, S) and got["masked_image"].shape == (N, 3, S, S) and got["image"].dtype == torch.float32
    assert got["mask"].shape == (N, 1, S, S) and got["mask"].dtype == torch.uint8 and got["mask_latent"].shape == (N, 1, S // 8, S // 8)
    host = {k: v.cpu().numpy() for k, v in got.items()}
    for b, (p, (name, _, _)) in enumerate(QC.FLAT):
        want = ref["pre"][b]
        for k in ("image", "masked_image"):
            assert np.array_equal(host[k][b].view(np.uint32), want[k].view(np.uint32)), f"{name}: {k} of row {b} (page {p}) differs from the restatement"
        for k in ("mask", "mask_latent"):
            assert np.array_equal(host[k][b, 0], want[k]), f"{name}: {k} of row {b} (page {p}) differs from the restatement"
    assert torch.equal(got["image"][0], (imgs[0][10:74, 15:79].permute(2, 0, 1).float() - 127.5) * (1.0 / 127.5)), "axis_copy is the page slice"


def test_postprocess_quads_pages_and_union_masks(cuda, build, ref):
    import diffute_amd as D
    imgs, vae = _dev(ref["pages"], cuda), torch.from_numpy(ref["vae"].copy()).to(cuda)
    for fill in (0, 255):                                  # a byte nobody wrote shows under one fill or the other
        buf, views, guards = _slab(fill, cuda)
        got, unions = D.prepost.postprocess_quads(vae, imgs, ref["quads"], ref["frames"], return_mask=True, out=views)
        D.synchronize()
        assert all(g.data_ptr() == v.data_ptr() for g, v in zip(got, views))
        assert all(bool((buf[g] == fill).all()) for g in guards), "a guard band between the pages was written"
        for p, want in enumerate(ref["pastes"]):
            host = got[p].cpu().numpy()
            assert host.shape == PAGES[p] + (3,) and got[p].dtype == torch.uint8
            assert np.array_equal(host, want["out"]), f"page {p} differs from the restatement"
            assert np.array_equal(unions[p].cpu().numpy(), want["union"]), f"union mask of page {p} differs from the OR of the quads"
            outside = want["union"] == 0
            assert np.array_equal(host[outside], ref["pages"][p][outside]), "pixels outside every quad must be untouched"
            assert (host[want["pasted"]] != ref["pages"][p][want["pasted"]]).any()
    plain = D.prepost.postprocess_quads(vae, imgs, ref["quads"], ref["frames"])               # pages of its own, no mask: the same bytes
    assert all(torch.equal(a, b) for a, b in zip(plain, got))


def test_rectify_quads_strips(cuda, build, ref):
    import diffute_amd as D
    imgs = _dev(ref["pages"], cuda)
    got = D.prepost.rectify_quads(imgs, ref["quads"])
    D.synchronize()
    assert len(got) == N and all(t.dtype == torch.uint8 and t.is_cuda and t.is_contiguous() for t in got)
    base = got[0].data_ptr()
    for b, (t, want, q) in enumerate(zip(got, ref["strips"], ref["qs"])):
        assert t.data_ptr() - base == q["rect_off"], "the strips are views of one buffer, packed in item order"
        assert tuple(t.shape) == (q["rh"], q["rw"], 3) and np.array_equal(t.cpu().numpy(), want), f"{QC.FLAT[b][1][0]}: strip {b} differs from the restatement"
    assert torch.equal(got[0], imgs[0][20:33, 20:51]), "an axis-aligned quad is the page slice, both corners included"
    assert torch.equal(got[4], imgs[1][10:71, 68:81].flip(1).transpose(0, 1)), "a quarter turn is the slice turned, no resampling"
    assert torch.equal(got[6], imgs[2][30:51, 20:101].flip(0).flip(1)), "upside-down text is the slice turned by a half"


def test_a_quarter_turn_of_pages_quads_and_frames(cuda, build, ref):
    """np.rot90 of every page with its quads and frames turned along, in one launch each: the crops, masks and strips are identical; the
    pasted page is the turned pasted page - the same pixels pasted; values at most one level apart, and only where the float64 restatement
    lies within the fp32 error of a half-integer: at most 9 fp32 roundings (3 in post_src per tap side, 3 per pass) of values below
    295, each 295 * 2^-24."""
    import diffute_amd as D
    P = D.prepost
    imgs, vae = _dev(ref["pages"], cuda), torch.from_numpy(ref["vae"].copy()).to(cuda)
    timgs = _dev([QR.rot90_page(p) for p in ref["pages"]], cuda)
    tquads = [[QR.rot90_corners(c, w) for c in cs] for cs, (h, w) in zip(ref["quads"], PAGES)]
    tframes = [[QR.rot90_frame(f, w) for f in fs] for fs, (h, w) in zip(ref["frames"], PAGES)]
    a, b = P.preprocess_quads(imgs, ref["quads"], ref["frames"], size=S), P.preprocess_quads(timgs, tquads, tframes, size=S)
    assert all(torch.equal(a[k], b[k]) for k in a), "the crops of the turned pages differ"
    sa, sb = P.rectify_quads(imgs, ref["quads"]), P.rectify_quads(timgs, tquads)
    assert all(torch.equal(x, y) for x, y in zip(sa, sb)), "the strips of the turned pages differ"
    (pa, ua), (pb, ub) = P.postprocess_quads(vae, imgs, ref["quads"], ref["frames"], return_mask=True), P.postprocess_quads(vae, timgs, tquads, tframes,
                                                                                                                        return_mask=True)
    D.synchronize()
    bound = 9 * 295 * 2.0 ** -24
    for p in range(len(PAGES)):
        x, y = np.rot90(pa[p].cpu().numpy()).astype(np.int64), pb[p].cpu().numpy().astype(np.int64)
        assert np.array_equal(np.rot90(ua[p].cpu().numpy()), ub[p].cpu().numpy())
        pasted = np.rot90(ref["pastes"][p]["pasted"])
        assert np.array_equal(x[~pasted], y[~pasted]) and np.array_equal(y[~pasted], QR.rot90_page(ref["pages"][p])[~pasted]), "the same pixels are pasted"
        d = np.abs(x - y)
        assert d.max() <= 1
        if d.any():
            mine = [i for i, q in enumerate(ref["qs"]) if q["page"] == p]
            v64 = np.rot90(QR.paste_page(ref["pages"][p], [ref["qs"][i] for i in mine], [ref["vae"][i] for i in mine], S, dtype=np.float64)["value"])
            frac = np.abs(v64 - np.floor(v64) - 0.5)
            assert (frac[d > 0] <= bound).all(), "a pasted value changed under the turn away from a rounding tie"


# ---- the round trip: a linear ramp cropped, fed back as the decoder output and pasted onto a BLANK page must reproduce the ramp
RAMP = (64, 80)
RT_QUADS = [[QC.tilted(40, 32, 30, 8, 20), [(60, 44), (20, 44), (20, 32), (60, 32)]], [[(45, 12), (45, 52), (35, 52), (35, 12)]]]
RT_FRAMES = [[(80, 64, 40, 56, 20), (2 * 8 + S - 1, S - 1, S, -80, 0)], [(80, 64, 48, 0, 80)]]


def _ramp():
    y, x = np.mgrid[0:RAMP[0], 0:RAMP[1]]
    return np.stack([3 * x, 3 * y + 20, 250 - 3 * x], -1)


def test_round_trip_over_a_linear_ramp(cuda, build):
    """Geometry without the restatement.  The page is an integer linear ramp with |slope| = 3 along x (channels 0, 2) or y (channel 1),
    inside 0 .. 255.  Cropping a linear page is exact up to ONE byte rounding (<= 1/2: bilinear interpolation reproduces a linear
    function, the frames lie inside the page so no tap is clamped); the paste interpolates those bytes (a convex combination: the 1/2
    stays 1/2) and rounds once more (<= 1/2).  The two maps are each off by at most (|p| + |q|) / 2 * 2^-16 of their own pixels from the
    matrix rounding (tests/test_prepost_quad_host.py), with |p|, |q| <= S going out and <= 2 * 80, 2 * 64 coming back (crop_scale <= S:
    a crop pixel is at most a page pixel), times the slope 3; the fp32 arithmetic adds less than 1e-3.  A map off by one crop pixel
    moves the sample by crop_scale / S >= 40 / 64 page pixels, so one of the channels changes by at least 3 * 0.625 / sqrt(2) - above
    the bound."""
    import diffute_amd as D
    ramp = _ramp()
    assert ramp.min() >= 0 and ramp.max() <= 255
    bound = 0.5 + 0.5 + 3 * (S + (2 * RAMP[1] + 2 * RAMP[0]) / 2) / 65536 + 1e-3
    assert all(f[2] <= S and 3 * (f[2] / S) / math.sqrt(2) > bound for fs in RT_FRAMES for f in fs)
    page = torch.from_numpy(ramp.astype(np.uint8)).to(cuda)
    imgs, blank = [page, page.clone()], [torch.full_like(page, 7), torch.full_like(page, 7)]
    for (cx2, cy2, cs, ux, uy) in (f for fs in RT_FRAMES for f in fs):                        # the frames' boxes lie inside the page
        e = cs * (abs(ux) + abs(uy)) / math.hypot(ux, uy) / 2
        assert cx2 / 2 - e >= -0.5 and cx2 / 2 + e <= RAMP[1] - 0.5 and cy2 / 2 - e >= -0.5 and cy2 / 2 + e <= RAMP[0] - 0.5
    pre = D.prepost.preprocess_quads(imgs, RT_QUADS, RT_FRAMES, size=S)
    out = D.prepost.postprocess_quads(pre["image"], blank, RT_QUADS, RT_FRAMES)
    D.synchronize()
    Y, X = np.mgrid[0:RAMP[0], 0:RAMP[1]].astype(np.float64)
    for p in range(2):
        got = out[p].cpu().numpy().astype(np.float64)
        later = np.zeros(RAMP, bool)
        for c, (cx2, cy2, cs, ux, uy) in reversed(list(zip(RT_QUADS[p], RT_FRAMES[p]))):
            inside = np.ones(RAMP, bool)
            for k in range(4):
                (x0, y0), (x1, y1) = c[k], c[(k + 1) % 4]
                inside &= (x1 - x0) * (Y - y0) - (y1 - y0) * (X - x0) >= 0
            n, s = math.hypot(ux, uy), cs / S
            U = (S - 1) / 2 + (ux * (X - cx2 / 2) + uy * (Y - cy2 / 2)) / n / s
            V = (S - 1) / 2 + (-uy * (X - cx2 / 2) + ux * (Y - cy2 / 2)) / n / s
            sel = inside & ~later & (U >= 0.01) & (U <= S - 1.01) & (V >= 0.01) & (V <= S - 1.01)       # pasted, and no tap clamped
            assert sel.sum() >= 100
            err = np.abs(got[sel] - ramp[sel])
            print(f"round trip page {p} crop_scale {cs}: {int(sel.sum())} pixels, max error {err.max():.0f} levels, bound {bound:.4f}")
            assert err.max() <= bound, "a pasted pixel does not reproduce the page it was cropped from"
            later |= inside
        assert (got[~later] == 7).all(), "outside the quads the blank page is untouched"


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
    """one prepare and one launch per call, nothing else"""
    import diffute_amd as D
    from diffute_amd import _cabi
    names = []
    rec = _Recorder(_cabi.lib(), names)
    monkeypatch.setattr(_cabi, "lib", lambda elem=None: rec)
    imgs, vae = _dev(ref["pages"], cuda), torch.from_numpy(ref["vae"].copy()).to(cuda)
    calls = [("dmx_preprocess_quads", lambda: D.prepost.preprocess_quads(imgs, ref["quads"], ref["frames"], size=S)),
             ("dmx_postprocess_paste_quads", lambda: D.prepost.postprocess_quads(vae, imgs, ref["quads"], ref["frames"], return_mask=True)),
             ("dmx_rectify_quads", lambda: D.prepost.rectify_quads(imgs, ref["quads"])),
             ("dmx_preprocess_quads", lambda: D.prepost.preprocess_quads(imgs[:1], ref["quads"][:1], ref["frames"][:1], size=S))]      # one page is P = 1
    for entry, fn in calls:
        del names[:]
        fn()
        assert names == ["dmx_edit_quads_prepare", entry], entry
    D.synchronize()


def test_refusals_launch_nothing(cuda, ref):
    """a bad quad, a bad frame, a bad output list and a host table spoiled after the prepare: an error, and the sentinel-filled outputs
    stay as they were"""
    from diffute_amd import _cabi, prepost
    imgs, vae = _dev(ref["pages"], cuda), torch.from_numpy(ref["vae"].copy()).to(cuda)
    buf, views, guards = _slab(0x5A, cuda)
    quads, frames = ref["quads"], ref["frames"]
    bad_q = [list(q) for q in quads]
    bad_q[1][0] = [(100, 10), (140, 10), (140, 30), (100, 30)]        # x = 140: inside the 300-wide page 0, outside its own 131-wide page
    bad_f = [list(f) for f in frames]
    bad_f[2][1] = (100, 20, 0, 1, 0)
    ccw = [list(q) for q in quads]
    ccw[0][2] = list(reversed(quads[0][2]))
    for q, f, word in ((bad_q, frames, "item 4"), (quads, bad_f, "item 7"), (ccw, frames, "item 2")):
        with pytest.raises(RuntimeError, match=word):
            prepost.postprocess_quads(vae, imgs, q, f, out=views)
        with pytest.raises(RuntimeError, match=word):
            prepost.preprocess_quads(imgs, q, f, size=S)
    for q, word in ((bad_q, "item 4"), (ccw, "item 2")):
        with pytest.raises(RuntimeError, match=word):
            prepost.rectify_quads(imgs, q)
    for out in (views[:2], views[:2] + [imgs[2]], [v.to(torch.int8) for v in views]):
        with pytest.raises(ValueError):
            prepost.postprocess_quads(vae, imgs, quads, frames, out=out)
    with pytest.raises(TypeError):
        prepost.postprocess_quads(ref_vae_host(ref), imgs, quads, frames, out=views)
    # the launch entries themselves, with real addresses and good device tables: only the host tables are spoiled
    lib = _cabi.lib()
    qx = prepost._check_quads(imgs, quads, frames)
    strips = torch.full((1 << 16,), 0x5A, dtype=torch.uint8, device=cuda)
    pre_out = [torch.full((N * 3 * S * S,), 3.0, device=cuda), torch.full((N * 3 * S * S,), 3.0, device=cuda),
               torch.full((N * S * S,), 0x5A, dtype=torch.uint8, device=cuda), torch.full((N * 64,), 3.0, device=cuda)]
    for spoil in ("item", "page"):
        host, pages, _, stage, dbuf, off, _ = prepost._upload_quads(qx, S, views, None)
        if spoil == "item":
            host[6].x[0] = 260                                 # the first column right of page 2
        else:
            pages[1].W = 300                                   # another tile count: the blocks no longer belong to the table
        base, word = dbuf.data_ptr(), ("item 6" if spoil == "item" else "page 1")
        assert lib.dmx_postprocess_paste_quads(_cabi.ptr(vae), S, pages, base + off, 3, host, base, N, _cabi.current_stream()) == -1
        assert word in lib.dmx_last_error().decode()
        assert lib.dmx_preprocess_quads(pages, base + off, 3, host, base, N, S, *(_cabi.ptr(t) for t in pre_out), _cabi.current_stream()) == -1
        assert word in lib.dmx_last_error().decode()
        assert lib.dmx_rectify_quads(pages, base + off, 3, host, base, N, _cabi.ptr(strips), strips.numel(), _cabi.current_stream()) == -1
        assert word in lib.dmx_last_error().decode()
    _cabi.synchronize()
    assert bool((buf == 0x5A).all()) and bool((strips == 0x5A).all()) and bool((pre_out[2] == 0x5A).all()), "refused, yet something was written"
    assert all(bool((t == 3.0).all()) for t in (pre_out[0], pre_out[1], pre_out[3]))


def ref_vae_host(ref):
    return torch.from_numpy(ref["vae"].copy())
