"""Classifier-free guidance on the GPU: the guided scheduler step (dmx_sched_step_guided, csrc/sched.hip) alone against the numpy
restatement (tests/guidance_restatement.py, which tests/test_guidance_host.py holds to float64 and to the mistakes it must see) in both
builds of the library, its guards and refusals, denoise(guidance=) against the same loop written from the library's own pieces, and the
edit functions against their hand-assembled chains.  Tiny UNet / VAE of tests/test_models_gpu.py, the boxes of tests/test_edit_boxes_gpu.py."""
import ctypes

import numpy as np
import pytest
import torch

import guidance_restatement as G
from guidance_floors import FLOORS
from test_edit_boxes_gpu import BOXES, CROPS, H, ORIGINS, S, STEPS, W
from test_models_gpu import TINY_UNET, TINY_VAE
from util import rel_l2

pytestmark = pytest.mark.gpu
GUARD, SENT = 1024, 1234.5
ERR_ARG = -1


@pytest.fixture(scope="module")
def tiny_unet(cuda):
    import diffute_amd as D
    return D.UNet2DConditionModel(**TINY_UNET).cuda().requires_grad_(False)


@pytest.fixture(scope="module")
def tiny_vae(cuda):
    import diffute_amd as D
    return D.AutoencoderKL(**TINY_VAE).cuda().requires_grad_(False)


@pytest.fixture(scope="module")
def inputs(cuda):
    from diffute_amd.init import normal
    from diffute_amd.synthetic import synth_inputs
    lat, mask, mlat, ctx = synth_inputs(2, 16, 16, 77, 128, device=cuda)
    unc = normal(2, 29, 2 * 77 * 128, cuda).reshape(2, 77, 128)
    return lat, mask, mlat, ctx, unc


def _records():
    """(name, kind, record, takes noise): real scalars from the schedulers' plans; DPM-Solver++ orders 1, 2, 3 on a ring of 3"""
    import diffute_amd as D
    ddim = D.DDIMScheduler(); ddim.set_timesteps(50)
    ddpm = D.DDPMScheduler(); ddpm.set_timesteps(50)
    dpm = D.DPMSolverMultistepScheduler(solver_order=3); dpm.set_timesteps(20)
    p = dpm.plan()
    assert [r.order for r in p[:3]] == [1, 2, 3]
    return [("ddim", G.DDIM, ddim.plan(0.5)[24]), ("ddpm", G.DDPM, ddpm.plan()[24]), ("dpm1", G.DPMPP, p[0]), ("dpm2", G.DPMPP, p[1]),
            ("dpm3", G.DPMPP, p[2])]


def _with_noise(rec, on):
    from diffute_amd import _cabi
    r = _cabi.SchedRowRec.from_buffer_copy(bytes(rec))
    r.use_noise = int(on)
    return r


class _Buffers:
    """sample [2B][per], eps [2B][per], noise [B][per], hist [3][B][per], ratio [B]: each inside its own sentinel-filled allocation,
    `off` floats past a 16-byte boundary (off = 1: every row pointer is misaligned, the scalar path runs)"""

    def __init__(self, B, per, off, dev):
        self.B, self.per = B, per
        self.big, self.v = {}, {}
        for name, n in (("sample", 2 * B * per), ("eps", 2 * B * per), ("noise", B * per), ("hist", 3 * B * per), ("ratio", B)):
            self.big[name] = torch.full((GUARD + off + n + GUARD,), SENT, dtype=torch.float32, device=dev)
            self.v[name] = self.big[name][GUARD + off:GUARD + off + n]
            assert self.v[name].data_ptr() % 16 == 4 * off

    def fill(self, x, eps, nz, hist):
        B = self.B
        s = torch.from_numpy(x).clone()
        s[B:] = float("nan")                                  # rows [B, 2B) of the sample are write-only: poisoned
        for name, t in (("sample", s), ("eps", torch.from_numpy(eps)), ("noise", torch.from_numpy(nz)), ("hist", torch.from_numpy(hist))):
            self.v[name].copy_(t.reshape(-1))
        self.v["ratio"].fill_(SENT)

    def get(self, name, shape=None):
        a = self.v[name].cpu().numpy()
        return a if shape is None else a.reshape(shape)

    def assert_guards(self, what):
        for name, big in self.big.items():
            raw, n = big.cpu(), self.v[name].numel()
            lo = (self.v[name].data_ptr() - big.data_ptr()) // 4
            assert bool((raw[:lo] == SENT).all()) and bool((raw[lo + n:] == SENT).all()), f"{what}: written outside {name}"

    def snapshot(self):
        return {k: b.cpu().numpy().view(np.uint32).copy() for k, b in self.big.items()}


def _call(lib, buf, kind, rec, vpred, scale, rescale, noise=True, hist=True, n_hist=3, ratio=True, B=None, per=None, sample=True, eps=True, omr=None):
    from diffute_amd import _cabi
    P = lambda name, on: _cabi.ptr(buf.v[name]) if on else None
    return lib.dmx_sched_step_guided(P("sample", sample), P("eps", eps), P("noise", noise), P("hist", hist), n_hist if hist else 0, rec, kind, int(vpred),
                                     float(scale), float(rescale), float(1 - rescale) if omr is None else float(omr), P("ratio", ratio),
                                     buf.B if B is None else B, buf.per if per is None else per, _cabi.current_stream())


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


# ------------------------------------------------------------------------------------------------ 1. the entry alone
@pytest.mark.parametrize("build", ["bf16", "fp16"])
@pytest.mark.parametrize("per", G.PER_SAMPLE)
def test_entry_against_the_restatement(cuda, build, per):
    """all three kinds, DPM-Solver++ orders 1-3, v-prediction on / off, noise given / NULL, B in {1, 3}, aligned and one float off:
    rescale 0 is eval32 bit for bit (both halves of the sample, the ring slot); with rescale the ratio is within bound(floor) of ref64's
    and the outputs are eval32 evaluated with the kernel's own ratio, bit for bit"""
    from diffute_amd import _cabi
    lib = _cabi.lib(build)
    worst, n = 0.0, 0
    for B in G.BATCHES:
        x, eps, nz, hist = G.inputs(B, per)
        e64 = eps.astype(np.float64)
        k64 = {s: G.ratios(e64[:B], G.combine(e64[:B], e64[B:], s, np.float64), np.float64) for s in G.SCALES}
        for off in (0, 1):
            buf = _Buffers(B, per, off, cuda)
            for ri, (name, kind, rec0) in enumerate(_records()):
                dpm = kind == G.DPMPP
                for vpred in (False, True):
                    for with_noise in ((False,) if dpm else (False, True)):
                        rec = _with_noise(rec0, with_noise)
                        scale = G.SCALES[(ri + int(vpred) + int(with_noise) + B) % 3]
                        for rescale in (0.0,) + G.RESCALES:
                            if rescale != 0.0 and per < 2:
                                continue
                            what = f"{build} {name} vpred={vpred} noise={with_noise} B={B} per={per} off={off} scale={scale} rescale={rescale}"
                            buf.fill(x, eps, nz, hist)
                            rc = _call(lib, buf, kind, rec, vpred, scale, rescale, noise=with_noise, hist=dpm)
                            _cabi.check(rc, what, lib)
                            torch.cuda.synchronize()
                            got, gh, gk = buf.get("sample", (2 * B, per)), buf.get("hist", (3, B, per)), buf.get("ratio")
                            buf.assert_guards(what)
                            k = None
                            if rescale != 0.0:
                                for b in range(B):
                                    tol = G.bound(FLOORS[G.case_key(B, per, scale)][b])
                                    err = abs(float(gk[b]) - k64[scale][b]) / abs(k64[scale][b])
                                    worst = max(worst, err / tol)
                                    assert err <= tol, f"{what}: ratio[{b}] {gk[b]!r} vs {k64[scale][b]!r}: {err:.3e} > {tol:.3e}"
                                k = gk
                            else:
                                assert bool((gk == np.float32(SENT)).all()), f"{what}: ratio_out written without a rescale"
                            want, wh, _ = G.eval32(kind, rec, x, eps, nz if with_noise else None, hist if dpm else None, scale, rescale, vpred, k=k)
                            assert np.array_equal(_bits(got[:B]), _bits(want[:B])), f"{what}: rows [0, B)"
                            assert np.array_equal(_bits(got[B:]), _bits(want[B:])), f"{what}: rows [B, 2B)"
                            assert np.array_equal(_bits(gh), _bits(wh if dpm else hist)), f"{what}: the ring"
                            n += 1
    print(f"guided entry {build} per_sample={per}: {n} launches bit-equal to eval32; worst ratio error / bound {worst:.3f}")


# ------------------------------------------------------------------------------------------------ 2. guards, reproducibility, refusals
@pytest.mark.parametrize("build", ["bf16", "fp16"])
def test_reproducible_and_idle_slots_untouched(cuda, build):
    from diffute_amd import _cabi
    lib = _cabi.lib(build)
    B, per = 3, 4099
    x, eps, nz, hist = G.inputs(B, per)
    for name, kind, rec in _records():
        dpm = kind == G.DPMPP
        for off in (0, 1):
            buf = _Buffers(B, per, off, cuda)
            runs = []
            for _ in range(2):
                buf.fill(x, eps, nz, hist)
                _cabi.check(_call(lib, buf, kind, rec, False, 7.5, 0.7, noise=False, hist=dpm), name, lib)
                torch.cuda.synchronize()
                runs.append(buf.snapshot())
            assert all(np.array_equal(runs[0][k], runs[1][k]) for k in runs[0]), f"{name}: two runs differ"
            gh = buf.get("hist", (3, B, per))
            for slot in range(3):
                if not dpm or slot != rec.ring_w:
                    assert np.array_equal(_bits(gh[slot]), _bits(hist[slot])), f"{name}: ring slot {slot} was written"
            # the poison in rows [B, 2B) played no part: the same call on a clean duplicate gives the same bits
            buf.fill(x, eps, nz, hist)
            buf.v["sample"].copy_(torch.from_numpy(x).reshape(-1))
            _cabi.check(_call(lib, buf, kind, rec, False, 7.5, 0.7, noise=False, hist=dpm), name, lib)
            torch.cuda.synchronize()
            clean = buf.snapshot()
            assert all(np.array_equal(runs[0][k], clean[k]) for k in clean), f"{name}: rows [B, 2B) of the sample were read"


def test_refusals_write_nothing(cuda):
    from diffute_amd import _cabi
    lib = _cabi.lib()
    B, per = 3, 257
    x, eps, nz, hist = G.inputs(B, per)
    recs = {n: (k, r) for n, k, r in _records()}
    buf = _Buffers(B, per, 0, cuda)
    buf.fill(x, eps, nz, hist)
    before = buf.snapshot()

    def ring(order=None, **slots):
        r = _with_noise(recs["dpm3"][1], False)
        if order is not None:
            r.order = order
        for k, v in slots.items():
            setattr(r, k, v)
        return r
    ddim, dpm = recs["ddim"], recs["dpm3"]
    nan, inf = float("nan"), float("inf")
    bad = {
        "B = 0": dict(kind=ddim[0], rec=ddim[1], B=0),
        "B < 0": dict(kind=ddim[0], rec=ddim[1], B=-2),
        "NULL sample": dict(kind=ddim[0], rec=ddim[1], sample=False),
        "NULL model_output": dict(kind=ddim[0], rec=ddim[1], eps=False),
        "kind 3": dict(kind=3, rec=ddim[1]),
        "kind -1": dict(kind=-1, rec=ddim[1]),
        "dpm with noise": dict(kind=dpm[0], rec=dpm[1], noise=True),
        "dpm without a ring": dict(kind=dpm[0], rec=dpm[1], hist=False),
        "order 0": dict(kind=dpm[0], rec=ring(order=0)),
        "order 4": dict(kind=dpm[0], rec=ring(order=4)),
        "order 3 on a ring of 2": dict(kind=dpm[0], rec=ring(ring_w=0, ring_m1=1, ring_m2=1), n_hist=2),
        "ring_w past the ring": dict(kind=dpm[0], rec=ring(ring_w=3)),
        "ring_w negative": dict(kind=dpm[0], rec=ring(ring_w=-1)),
        "ring_m1 negative": dict(kind=dpm[0], rec=ring(ring_m1=-1)),
        "ring_m1 is ring_w": dict(kind=dpm[0], rec=ring(ring_w=1, ring_m1=1, ring_m2=0)),
        "ring_m2 past the ring": dict(kind=dpm[0], rec=ring(ring_m2=5)),
        "rescale with per_sample 1": dict(kind=ddim[0], rec=ddim[1], per=1, rescale=0.5),
        "rescale < 0": dict(kind=ddim[0], rec=ddim[1], rescale=-0.1),
        "rescale > 1": dict(kind=ddim[0], rec=ddim[1], rescale=1.5),
        "rescale NaN": dict(kind=ddim[0], rec=ddim[1], rescale=nan),
        "scale NaN": dict(kind=ddim[0], rec=ddim[1], scale=nan),
        "scale inf": dict(kind=ddim[0], rec=ddim[1], scale=inf),
        "1 - rescale inf": dict(kind=ddim[0], rec=ddim[1], omr=-inf),
        "1 - rescale NaN": dict(kind=ddim[0], rec=ddim[1], omr=nan),
    }
    for what, kw in bad.items():
        a = dict(vpred=False, scale=3.0, rescale=0.0, noise=False, hist=kw["kind"] == G.DPMPP)
        a.update(kw)
        assert _call(lib, buf, **a) == ERR_ARG, what
        assert lib.dmx_last_error()
    torch.cuda.synchronize()
    after = buf.snapshot()
    assert all(np.array_equal(before[k], after[k]) for k in before), "a refused call wrote something"
    # ... and the same buffers are accepted once the argument is right (per_sample 1 without a rescale included)
    assert _call(lib, buf, ddim[0], ddim[1], False, 3.0, 0.0, noise=False, hist=False, per=1) == 0
    assert _call(lib, buf, dpm[0], ring(), False, 3.0, 0.5, noise=False) == 0
    torch.cuda.synchronize()
    buf.assert_guards("after the accepted calls")


# ------------------------------------------------------------------------------------------------ 3. denoise(guidance=)
def _hand_guided(unet, sch, steps, interval, lat, mask, mlat, ctx, unc, scale, rescale=0.0, noise=None):
    """the guided loop from the library's own pieces: set_context on 2B rows, forward_parts, the combination as three separate torch ops
    (with rescale: the formula in torch), scheduler.step"""
    sch.set_timesteps(steps)
    B = lat.shape[0]
    x = (lat * sch.init_noise_sigma).contiguous()
    m2, ml2 = torch.cat([mask, mask], 0), torch.cat([mlat, mlat], 0)
    unet.set_context(torch.cat([ctx, unc], 0))
    buf = unet.step_cache(2 * B, x.shape[2], x.shape[3]) if interval > 1 else None
    for i, t in enumerate(sch.timesteps):
        td = torch.as_tensor(t).reshape(1).to(device=x.device, dtype=torch.int64)
        sc = {} if buf is None else dict(step_cache=(buf, "use" if i % interval else "fill"))
        eps = unet.forward_parts([torch.cat([x, x], 0), m2, ml2], td, **sc)
        ec, eu = eps[:B], eps[B:]
        d = ec - eu
        s = d * scale
        g = eu + s
        if rescale:
            k = ec.std(dim=(1, 2, 3), keepdim=True) / g.std(dim=(1, 2, 3), keepdim=True)
            g = rescale * (g * k) + (1 - rescale) * g
        x = (sch.step(g, t, x, variance_noise=noise[i]) if noise is not None else sch.step(g, t, x)).prev_sample
    return x


def _sched(name):
    import diffute_amd as D
    return {"ddim": D.DDIMScheduler, "ddpm": D.DDPMScheduler, "dpm": D.DPMSolverMultistepScheduler}[name]()


# With a rescale the loop written in torch takes its two deviations from torch.std, another summation order than the kernel's: the ratios
# differ in the last bits (about 1e-7 relative), and so do the latents of every step.  Measured on the MI355X over the twelve cases below
# (4 steps, scale 3, rescale 0.7, rel-L2 of the final latents against the torch loop): 5.0e-8 .. 6.9e-8, the same eager and as a graph.
# The bound is 1e-4, 1400 x the worst measured case, and the margin is for one event that did not occur in these runs but may after an
# unrelated change of a UNet kernel: a latent that differs by 1e-7 can round to the other bf16 neighbour at the UNet's input (2^-9 on one
# of a row's 1024 elements: 6e-5 rel-L2).  It stays below what the mildest wrong formula gives - one biased and one unbiased deviation move
# k by 5e-4 and the latents by 0.7 x that - which the entry test above sees at 2^-22 anyway.
RESCALE_TOL = 1e-4


@pytest.mark.parametrize("graph", [False, True], ids=["eager", "graph"])
@pytest.mark.parametrize("interval", [1, 2])
@pytest.mark.parametrize("name", ["ddim", "ddpm", "dpm"])
def test_guided_denoise_is_the_hand_written_loop(cuda, tiny_unet, inputs, name, interval, graph):
    import diffute_amd as D
    from diffute_amd.init import normal
    lat, mask, mlat, ctx, unc = inputs
    steps = 4
    nz = normal(3, 31, steps * 2 * 4 * 16 * 16, cuda).reshape(steps, 2, 4, 16, 16) if name == "ddpm" else None
    kw = dict(variance_noise=nz, cache_interval=interval, use_graph=graph)
    seen = []
    out = D.denoise(tiny_unet, _sched(name), lat, mask, mlat, ctx, steps, guidance=D.Guidance(3.0, uncond=unc),
                    callback=lambda i, t, x, e: seen.append((i, tuple(x.shape), tuple(e.shape))), **kw).clone()
    D.synchronize()
    assert out.shape == lat.shape and torch.isfinite(out).all()
    assert seen == [(i, (2, 4, 16, 16), (4, 4, 16, 16)) for i in range(steps)]
    want = _hand_guided(tiny_unet, _sched(name), steps, interval, lat, mask, mlat, ctx, unc, 3.0, noise=nz)
    assert torch.equal(out, want), f"{name} interval {interval}: rel-L2 {rel_l2(out, want):.3e}"
    assert not torch.equal(out, D.denoise(tiny_unet, _sched(name), lat, mask, mlat, ctx, steps, **kw))
    # one shared context [1,S,D], and micro-batches (a chain per row, each with its own 2-row forward)
    one = D.denoise(tiny_unet, _sched(name), lat, mask, mlat, ctx, steps, guidance=D.Guidance(3.0, uncond=unc[:1]), **kw)
    assert torch.equal(one, _hand_guided(tiny_unet, _sched(name), steps, interval, lat, mask, mlat, ctx, unc[:1].expand(2, -1, -1), 3.0, noise=nz))
    # rescale: the same loop with the formula in torch
    got = D.denoise(tiny_unet, _sched(name), lat, mask, mlat, ctx, steps, guidance=D.Guidance(3.0, 0.7, unc), **kw).clone()
    ref = _hand_guided(tiny_unet, _sched(name), steps, interval, lat, mask, mlat, ctx, unc, 3.0, 0.7, noise=nz)
    err = rel_l2(got, ref)
    print(f"guided denoise with rescale 0.7, {name} interval {interval} graph {graph}: rel-L2 {err:.3e} vs the torch loop")
    assert torch.isfinite(got).all() and err <= RESCALE_TOL and not torch.equal(got, out)
    again = D.denoise(tiny_unet, _sched(name), lat, mask, mlat, ctx, steps, guidance=D.Guidance(3.0, 0.7, unc), **kw)
    assert torch.equal(again, got)


def test_micro_batched_guided_chains(cuda, tiny_unet, inputs):
    """micro_batches = 2: each chain holds its own row twice; rows do not interact, so every chain is the B = 1 guided loop bit for bit"""
    import diffute_amd as D
    lat, mask, mlat, ctx, unc = inputs
    seen = []
    out = D.denoise(tiny_unet, D.DDIMScheduler(), lat, mask, mlat, ctx, 3, guidance=D.Guidance(3.0, 0.5, unc), micro_batches=2,
                    callback=lambda i, t, x, e: seen.append((x.clone(), e.clone())))
    for b in range(2):
        row = D.denoise(tiny_unet, D.DDIMScheduler(), lat[b:b + 1], mask[b:b + 1], mlat[b:b + 1], ctx[b:b + 1], 3,
                        guidance=D.Guidance(3.0, 0.5, unc[b:b + 1]))
        assert torch.equal(out[b:b + 1], row), b
    assert all(x.shape == (2, 4, 16, 16) and e.shape == (4, 4, 16, 16) for x, e in seen) and torch.equal(seen[-1][0], out)


# ------------------------------------------------------------------------------------------------ 4. / 5. the exact identities
def test_equal_contexts_give_the_plain_loop_on_duplicated_rows(cuda, tiny_unet, inputs):
    """uncond == the conditional context: ec == eu, so eu + 3 * (ec - eu) == eu exactly - rows [0, B) of plain denoise on the 2B rows"""
    import diffute_amd as D
    lat, mask, mlat, ctx, _ = inputs
    dup = lambda t: torch.cat([t, t], 0)
    for name in ("ddim", "dpm"):
        got = D.denoise(tiny_unet, _sched(name), lat, mask, mlat, ctx, 3, guidance=D.Guidance(3.0, uncond=ctx))
        plain = D.denoise(tiny_unet, _sched(name), dup(lat), dup(mask), dup(mlat), dup(ctx), 3)
        assert torch.equal(got, plain[:2]) and torch.equal(plain[:2], plain[2:]), name


def test_scale_one_and_none_are_todays_loop(cuda, tiny_unet, inputs):
    import diffute_amd as D
    lat, mask, mlat, ctx, unc = inputs
    for name in ("ddim", "dpm"):
        base = D.denoise(tiny_unet, _sched(name), lat, mask, mlat, ctx, 3).clone()
        assert torch.equal(D.denoise(tiny_unet, _sched(name), lat, mask, mlat, ctx, 3, guidance=None), base)
        assert torch.equal(D.denoise(tiny_unet, _sched(name), lat, mask, mlat, ctx, 3, guidance=D.Guidance(1.0)), base)
        assert torch.equal(D.denoise(tiny_unet, _sched(name), lat, mask, mlat, ctx, 3, guidance=D.Guidance(1.0, 0.0, unc)), base)


# ------------------------------------------------------------------------------------------------ 6. launch count
def _launches(lib, fn):
    from diffute_amd import _cabi
    torch.cuda.synchronize()
    lib.dmx_profile_begin()
    out = fn()
    buf = (ctypes.c_double * (4 * 32))()
    _cabi.check(lib.dmx_profile_end(buf, len(buf)), "profile_end")
    return [int(buf[4 * k]) for k in range(32)], out


@pytest.mark.parametrize("name", ["ddim", "dpm"])
def test_guidance_adds_no_launch(cuda, tiny_unet, inputs, name):
    """a guided pass at B launches exactly what a plain pass at 2B launches, with and without the rescale"""
    import diffute_amd as D
    from diffute_amd import _cabi
    lib = _cabi.lib()
    lat, mask, mlat, ctx, unc = inputs
    dup = lambda t: torch.cat([t, t], 0)
    plain, _ = _launches(lib, lambda: D.denoise(tiny_unet, _sched(name), dup(lat), dup(mask), dup(mlat), dup(ctx), 3).clone())
    for rescale in (0.0, 0.7):
        guided, _ = _launches(lib, lambda: D.denoise(tiny_unet, _sched(name), lat, mask, mlat, ctx, 3, guidance=D.Guidance(3.0, rescale, unc)).clone())
        assert sum(guided) == sum(plain) > 0, (name, rescale, sum(guided), sum(plain))
    print(f"launches of a 3-step {name} pass: plain at 2B {sum(plain)}, guided at B {sum(guided)}")


# ------------------------------------------------------------------------------------------------ 7. the edit functions
@pytest.fixture(scope="module")
def edit_setup(cuda, tiny_unet, tiny_vae):
    from diffute_amd.init import normal
    img = torch.from_numpy(np.random.RandomState(11).randint(0, 256, (H, W, 3), dtype=np.uint8)).to(cuda)
    img2 = torch.from_numpy(np.random.RandomState(12).randint(0, 256, (200, 260, 3), dtype=np.uint8)).to(cuda)
    ctx = normal(2, 13, 3 * 77 * 128, cuda).reshape(3, 77, 128)
    unc = normal(2, 37, 3 * 77 * 128, cuda).reshape(3, 77, 128)
    enc_noise = normal(4, 71, 3 * 4 * 16 * 16, cuda).reshape(3, 4, 16, 16)
    return dict(unet=tiny_unet, vae=tiny_vae, img=img, img2=img2, ctx=ctx, unc=unc, enc_noise=enc_noise)


def _hand_rows(s, pre, guidance_of, bs=2):
    """edit_latents' chain per chunk of `bs` rows: encode, guided denoise from the seed-0 draw, decode"""
    import diffute_amd as D
    vae, sf = s["vae"], s["vae"].config.scaling_factor
    init = torch.randn((1, 4, S // 8, S // 8), generator=torch.manual_seed(0), dtype=torch.float32).to(s["img"].device)
    outs = []
    for lo in range(0, 3, bs):
        hi = min(3, lo + bs)
        mlat = vae.encode(pre["masked_image"][lo:hi]).latent_dist.sample(noise=s["enc_noise"][lo:hi]) * sf
        lat = D.denoise(s["unet"], D.DDIMScheduler(), init.expand(hi - lo, -1, -1, -1).contiguous(), D.mask_to_latent(pre["mask"][lo:hi], 8), mlat,
                        s["ctx"][lo:hi], STEPS, guidance=guidance_of(lo, hi))
        with torch.no_grad():
            outs.append(vae.decode(lat / sf).sample)
    return torch.cat(outs, 0)


@pytest.mark.parametrize("rescale", [0.0, 0.7])
def test_edit_boxes_and_edit_pages_with_guidance(cuda, edit_setup, rescale):
    """N = 3 boxes in chunks of 2: bit-equal to preprocess / guided denoise / decode / postprocess by hand; the per-box uncond [3,S,D]
    follows its box across the chunk boundary and, in edit_pages, across the page boundary (2 + 1 boxes on two pages)"""
    import diffute_amd as D
    s = edit_setup
    g = D.Guidance(3.0, rescale, s["unc"])
    kw = dict(batch_size=2, enc_noise=s["enc_noise"], return_intermediate=True, size=S)
    page, image_vae, pre = D.edit_boxes(s["unet"], s["vae"], D.DDIMScheduler(), s["img"], BOXES, s["ctx"], STEPS, origins=ORIGINS, crop_scales=CROPS,
                                        guidance=g, **kw)
    hand_pre = D.prepost.preprocess_batch(s["img"], BOXES, ORIGINS, CROPS, size=S)
    hand = _hand_rows(s, hand_pre, lambda lo, hi: D.Guidance(3.0, rescale, s["unc"][lo:hi]))
    assert torch.equal(image_vae, hand) and torch.equal(page, D.prepost.postprocess_batch(hand, s["img"], BOXES, ORIGINS, CROPS))
    # the wrong row's uncond is another result: box 2 alone in its chunk with box 0's unconditional context
    wrong = _hand_rows(s, hand_pre, lambda lo, hi: D.Guidance(3.0, rescale, s["unc"][0:hi - lo]))
    assert torch.equal(wrong[:2], hand[:2]) and not torch.equal(wrong[2], hand[2])
    plain = D.edit_boxes(s["unet"], s["vae"], D.DDIMScheduler(), s["img"], BOXES, s["ctx"], STEPS, origins=ORIGINS, crop_scales=CROPS, **kw)[1]
    assert not torch.equal(plain, image_vae)
    one = D.edit_boxes(s["unet"], s["vae"], D.DDIMScheduler(), s["img"], BOXES, s["ctx"], STEPS, origins=ORIGINS, crop_scales=CROPS,
                       guidance=D.Guidance(1.0, 0.0, s["unc"]), **kw)[1]
    assert torch.equal(one, plain)
    # two pages: boxes 0, 1 on page 0 and box 2 (another size of page) on page 1
    imgs = [s["img"], s["img2"]]
    boxes2, origins2, crops2 = [BOXES[:2], [(60, 120, 140, 136)]], [ORIGINS[:2], [(50, 70)]], [CROPS[:2], [96]]
    pages, pv, _ = D.edit_pages(s["unet"], s["vae"], D.DDIMScheduler(), imgs, boxes2, s["ctx"], STEPS, origins=origins2, crop_scales=crops2,
                                guidance=g, **kw)
    pre2 = D.prepost.preprocess_pages(imgs, boxes2, origins2, crops2, size=S)
    hand2 = _hand_rows(s, pre2, lambda lo, hi: D.Guidance(3.0, rescale, s["unc"][lo:hi]))
    want = D.prepost.postprocess_pages(hand2, imgs, boxes2, origins2, crops2)
    assert torch.equal(pv, hand2) and len(pages) == 2 and all(torch.equal(a, b) for a, b in zip(pages, want))
    assert torch.equal(pv[:2], image_vae[:2])                 # (the first chunk is edit_boxes' first chunk)


def test_edit_boxes_verified_with_guidance(cuda, edit_setup):
    """K = 3 candidates of N = 3 boxes, 9 rows box-major in chunks of 2 (chunks straddle boxes): the per-box uncond is repeated per
    candidate like the conditional context - bit-equal to the chunks assembled by hand"""
    import diffute_amd as D
    s = edit_setup
    K = 3
    ocr = D.VisionEncoderDecoderModel(
        D.TrOCREncoder(device=cuda, image_size=32, patch_size=16, hidden_size=256, num_hidden_layers=1, num_attention_heads=4, intermediate_size=256),
        D.TrOCRForCausalLM(device=cuda, d_model=256, decoder_layers=1, decoder_attention_heads=4, decoder_ffn_dim=512, vocab_size=300,
                           max_position_embeddings=64))
    labels = torch.from_numpy(np.random.RandomState(3).randint(3, 300, (3, 6))).to(torch.int64)
    g = D.Guidance(3.0, 0.7, s["unc"])
    r = D.edit_boxes_verified(s["unet"], s["vae"], D.DDIMScheduler(), ocr, D.TrOCRProcessor(size=32), s["img"], BOXES, s["ctx"], labels, STEPS,
                              candidates=K, batch_size=2, ocr_batch_size=4, origins=ORIGINS, crop_scales=CROPS, enc_noise=s["enc_noise"], size=S,
                              return_intermediate=True, guidance=g)
    D.synchronize()
    vae, sf = s["vae"], s["vae"].config.scaling_factor
    pre = D.prepost.preprocess_batch(s["img"], BOXES, ORIGINS, CROPS, size=S)
    init = torch.cat([torch.randn((1, 4, S // 8, S // 8), generator=torch.manual_seed(k), dtype=torch.float32) for k in range(K)], 0).to(cuda)
    mask_lat = D.mask_to_latent(pre["mask"], 8)
    mlat, outs = {}, []
    for lo in range(0, 3 * K, 2):
        rows = list(range(lo, min(3 * K, lo + 2)))
        box = [q // K for q in rows]
        new = [b for b in sorted(set(box)) if b not in mlat]
        if new:                                            # (a box is encoded with the boxes that first appear in the same chunk)
            z = vae.encode(pre["masked_image"][new[0]:new[-1] + 1]).latent_dist.sample(noise=s["enc_noise"][new[0]:new[-1] + 1]) * sf
            for j, b in enumerate(new):
                mlat[b] = z[j:j + 1]
        lat = D.denoise(s["unet"], D.DDIMScheduler(), init[[q % K for q in rows]].contiguous(), mask_lat[box], torch.cat([mlat[b] for b in box], 0),
                        s["ctx"][box], STEPS, guidance=D.Guidance(3.0, 0.7, s["unc"][box]))
        with torch.no_grad():
            outs.append(vae.decode(lat / sf).sample)
    hand = torch.cat(outs, 0).reshape(3, K, 3, S, S)
    assert torch.equal(r.image_vae, hand)
    page, choice = D.prepost.postprocess_select_batch(hand, r.scores, s["img"], BOXES, ORIGINS, CROPS, threshold=None)
    assert torch.equal(r.image, page) and torch.equal(r.choice, choice)
    plain = D.edit_boxes_verified(s["unet"], s["vae"], D.DDIMScheduler(), ocr, D.TrOCRProcessor(size=32), s["img"], BOXES, s["ctx"], labels, STEPS,
                                  candidates=K, batch_size=2, ocr_batch_size=4, origins=ORIGINS, crop_scales=CROPS, enc_noise=s["enc_noise"], size=S,
                                  return_intermediate=True)
    assert not torch.equal(plain.image_vae, r.image_vae)
