"""The step cache on the GPU (denoise(cache_interval=n), UNet2DConditionModel.forward_parts(step_cache=)): DeepCache-style reuse of
the deep UNet features across denoise steps.  The result of a cached loop differs from the plain loop's by design, so nothing here
compares the two for closeness: the library must compute exactly the cached algorithm - against the restatement
(tests/step_cache_restatement.py, whose own claims tests/test_step_cache_host.py checks) and bit for bit against itself wherever the
algorithm says two things are equal.  Tiny config of tests/test_models_gpu.py throughout."""
import ctypes

import numpy as np
import pytest
import torch

import step_cache_restatement as SC
from test_models_gpu import E2E_EMU, TINY_UNET, TINY_VAE
from util import assert_close, rel_l2

pytestmark = pytest.mark.gpu
GUARD, SENTINEL = 4096, 0x5A


@pytest.fixture(scope="module")
def tiny_unet(cuda):
    import diffute_amd as D
    return D.UNet2DConditionModel(**TINY_UNET).cuda().requires_grad_(False)


@pytest.fixture(scope="module")
def tiny_unet_f16(cuda):
    import diffute_amd as D
    return D.UNet2DConditionModel(**TINY_UNET).to(cuda, dtype=torch.float16).requires_grad_(False)


@pytest.fixture(scope="module")
def inputs(cuda):
    from diffute_amd.synthetic import synth_inputs
    return synth_inputs(2, 16, 16, 77, 128, device=cuda)


@pytest.fixture(scope="module")
def P(tiny_unet):
    return {k: v.detach().cpu().float() for k, v in tiny_unet.state_dict().items()}


def _unet(request, build):
    return request.getfixturevalue("tiny_unet" if build == "bf16" else "tiny_unet_f16")


def _guarded_cache(unet, B, H, W):
    """a step cache inside a sentinel-filled allocation -> (whole allocation, the cache)"""
    n = unet.step_cache(B, H, W).numel()
    big = torch.full((n + 2 * GUARD,), SENTINEL, dtype=torch.uint8, device=unet.device)
    return big, big[GUARD:GUARD + n]


def _assert_guards(big, n, name):
    raw = big.cpu()
    assert bool((raw[:GUARD] == SENTINEL).all()) and bool((raw[GUARD + n:] == SENTINEL).all()), f"{name}: bytes outside the step cache were written"


def _launches(lib, fn):
    """launches per kernel class of fn() (dmx_profile_begin / dmx_profile_end: every walk inside is eager) -> (list of counts, fn's result)"""
    from diffute_amd import _cabi
    torch.cuda.synchronize()
    lib.dmx_profile_begin()
    out = fn()
    buf = (ctypes.c_double * (4 * 32))()
    _cabi.check(lib.dmx_profile_end(buf, len(buf)), "profile_end")
    return [int(buf[4 * k]) for k in range(32)], out


# ------------------------------------------------------------------------------------------------ 1. fill is invisible
@pytest.mark.parametrize("build", ["bf16", "fp16"])
@pytest.mark.parametrize("shape", [(2, 16, 16), (3, 16, 24)], ids=["B2_16x16", "B3_16x24"])
def test_fill_is_invisible(cuda, request, build, shape):
    """a FILL forward returns the bits of the plain forward, writes nothing outside the cache, and what it leaves there is the tensor
    that enters the last up-block: the "up2" tap, bit for bit"""
    from diffute_amd.synthetic import synth_inputs
    unet = _unet(request, build)
    B, H, W = shape
    lat, mask, mlat, ctx = synth_inputs(B, H, W, 77, 128, device=cuda, seed=3)
    t = torch.tensor([981], device=cuda)
    unet.set_context(ctx)
    plain = unet.forward_parts([lat, mask, mlat], t).clone()
    big, buf = _guarded_cache(unet, B, H, W)
    got = unet.forward_parts([lat, mask, mlat], t, step_cache=(buf, "fill")).clone()
    torch.cuda.synchronize()
    assert torch.equal(got, plain)
    _assert_guards(big, buf.numel(), f"fill {build} {shape}")
    C = TINY_UNET["block_out_channels"][1]
    kept = buf[:B * H * W * C * 2].view(unet.compute_dtype).reshape(B, H, W, C).permute(0, 3, 1, 2).float()
    _, taps = unet.forward_taps(torch.cat([lat, mask, mlat], 1), t, ctx)
    assert torch.equal(kept, taps["up2"]), "the step cache does not hold the up2 tensor"
    assert torch.equal(unet.forward_parts([lat, mask, mlat], t), plain)


# ------------------------------------------------------------------------------------------------ 2. identity
@pytest.mark.parametrize("build", ["bf16", "fp16"])
@pytest.mark.parametrize("graph", [False, True], ids=["eager", "graph"])
def test_use_on_its_own_cache_is_the_full_forward(cuda, request, inputs, build, graph):
    """fill, then use on the same inputs: the same kernels on the same bytes and statistics - the full forward's bits.  With graph=True
    the calls are made three times (eager, capture, replay) on a side stream."""
    unet = _unet(request, build)
    lat, mask, mlat, ctx = inputs
    stream = torch.cuda.Stream(device=cuda)
    stream.wait_stream(torch.cuda.current_stream(cuda))
    with torch.cuda.stream(stream):
        unet.set_context(ctx)
        for t in (torch.tensor([981], device=cuda), torch.tensor([981, 3], device=cuda)):
            plain = unet.forward_parts([lat, mask, mlat], t).clone()
            big, buf = _guarded_cache(unet, 2, 16, 16)
            out_f, out_u = torch.empty_like(plain), torch.empty_like(plain)
            for rep in range(3 if graph else 1):
                out_f.zero_(); out_u.zero_()
                unet.forward_parts([lat, mask, mlat], t, out=out_f, graph=graph, step_cache=(buf, "fill"))
                unet.forward_parts([lat, mask, mlat], t, out=out_u, graph=graph, step_cache=(buf, "use"))
                stream.synchronize()
                assert torch.equal(out_f, plain), f"fill, call {rep}"
                assert torch.equal(out_u, plain), f"use, call {rep}: differs in {int((out_u != plain).sum())} elements, rel-L2 {rel_l2(out_u, plain):.3e}"
            _assert_guards(big, buf.numel(), f"identity {build} graph={graph}")
    torch.cuda.current_stream(cuda).wait_stream(stream)


# ------------------------------------------------------------------------------------------------ 3. stale-cache parity
@pytest.mark.parametrize("t_fill,t_use", [([981], [961]), ([981, 3], [961, 3])], ids=["scalar", "per_row"])
def test_stale_cache_parity(cuda, tiny_unet, P, inputs, t_fill, t_use):
    """fill at (x, t), use at (x', t'): the shallow step of the restatement on the restatement's own kept tensor, within the bound the
    full forward holds against the bf16-emulating oracle - and far from the full forward at (x', t'): the deep part did not run"""
    from oracle import unet as OU
    lat, mask, mlat, ctx = inputs
    lat2 = lat + 0.3 * torch.roll(lat, 1, 0)
    tf, tu = torch.tensor(t_fill, device=cuda), torch.tensor(t_use, device=cuda)
    tiny_unet.set_context(ctx)
    buf = tiny_unet.step_cache(2, 16, 16)
    tiny_unet.forward_parts([lat, mask, mlat], tf, step_cache=(buf, "fill"))
    got = tiny_unet.forward_parts([lat2, mask, mlat], tu, step_cache=(buf, "use")).clone()
    full = tiny_unet.forward_parts([lat2, mask, mlat], tu).clone()
    taps = {}
    OU.unet_forward(P, OU.TINY_UNET, torch.cat([lat, mask, mlat], 1).cpu(), tf.cpu(), ctx.cpu(), emulate_bf16=True, taps=taps)
    ref = SC.shallow_forward(P, OU.TINY_UNET, torch.cat([lat2, mask, mlat], 1).cpu(), tu.cpu(), ctx.cpu(), taps["up2"], emulate_bf16=True)
    e = assert_close(got, ref, E2E_EMU, "shallow step on a stale cache vs the restatement")
    d = rel_l2(got, full)
    print(f"stale cache {t_fill}->{t_use}: rel-L2 {e:.2e} vs the restatement, {d:.2e} from the full forward")
    assert d > 0.1, "the shallow step is the full forward: the deep part ran anyway"


# ------------------------------------------------------------------------------------------------ 4. loops
@pytest.mark.parametrize("steps,interval", [(5, 2), (7, 3)])
def test_cached_ddim_loops(cuda, tiny_unet, P, inputs, steps, interval):
    import diffute_amd as D
    from oracle import unet as OU
    lat, mask, mlat, ctx = inputs
    cpu = [v.cpu() for v in inputs]
    out = D.denoise(tiny_unet, D.DDIMScheduler(), lat, mask, mlat, ctx, steps, cache_interval=interval)
    e16 = assert_close(out, SC.cached_denoise(P, OU.TINY_UNET, *cpu, steps, interval, emulate_bf16=True), 2e-2, "cached DDIM loop vs bf16emu")
    e32 = assert_close(out, SC.cached_denoise(P, OU.TINY_UNET, *cpu, steps, interval), 5e-2, "cached DDIM loop vs fp32")
    print(f"cached DDIM loop ({steps} steps, interval {interval}) rel-L2: vs bf16emu {e16:.2e}, vs fp32 {e32:.2e}")
    eager = D.denoise(tiny_unet, D.DDIMScheduler(), lat, mask, mlat, ctx, steps, cache_interval=interval, use_graph=False)
    assert torch.equal(eager, out), "use_graph=False differs from the captured graphs"
    assert torch.equal(D.denoise(tiny_unet, D.DDIMScheduler(), lat, mask, mlat, ctx, steps, cache_interval=interval), out)      # (replayed graphs)
    out_mb = D.denoise(tiny_unet, D.DDIMScheduler(), lat, mask, mlat, ctx, steps, cache_interval=interval, micro_batches=2)
    assert_close(out_mb, out.cpu(), 1e-2, "micro-batched cached loop (a cache per chain) vs the single chain")


def _hand_loop(unet, sch, steps, interval, lat, mask, mlat, ctx, noise=None):
    """the cached loop spelled out: forward_parts(step_cache=) + scheduler.step"""
    sch.set_timesteps(steps)
    x = (lat * sch.init_noise_sigma).contiguous()
    unet.set_context(ctx)
    buf = unet.step_cache(x.shape[0], x.shape[2], x.shape[3])
    for i, t in enumerate(sch.timesteps):
        td = torch.as_tensor(t).reshape(1).to(device=x.device, dtype=torch.int64)
        eps = unet.forward_parts([x, mask, mlat], td, step_cache=(buf, "use" if i % interval else "fill"))
        x = (sch.step(eps, t, x, variance_noise=noise[i]) if noise is not None else sch.step(eps, t, x)).prev_sample
    return x


def test_cached_ddpm_and_dpm_solver_loops(cuda, tiny_unet, inputs):
    """DDPM with injected variance noise (5 steps, interval 2) and DPM-Solver++ (6, 3): denoise is the hand-driven loop, bit for bit - the
    solver's history ring sees an eps on every step, shallow or full"""
    import diffute_amd as D
    from diffute_amd.init import normal
    lat, mask, mlat, ctx = inputs
    nz = normal(3, 31, 5 * 2 * 4 * 16 * 16, cuda).reshape(5, 2, 4, 16, 16)
    out = D.denoise(tiny_unet, D.DDPMScheduler(), lat, mask, mlat, ctx, 5, variance_noise=nz, cache_interval=2)
    assert torch.isfinite(out).all()
    assert torch.equal(out, _hand_loop(tiny_unet, D.DDPMScheduler(), 5, 2, lat, mask, mlat, ctx, noise=nz))
    out = D.denoise(tiny_unet, D.DPMSolverMultistepScheduler(), lat, mask, mlat, ctx, 6, cache_interval=3)
    assert torch.isfinite(out).all()
    assert torch.equal(out, _hand_loop(tiny_unet, D.DPMSolverMultistepScheduler(), 6, 3, lat, mask, mlat, ctx))
    assert not torch.equal(out, D.denoise(tiny_unet, D.DPMSolverMultistepScheduler(), lat, mask, mlat, ctx, 6))


# ------------------------------------------------------------------------------------------------ 5. default path and launch count
def test_default_path_and_launch_counts(cuda, tiny_unet, inputs):
    import diffute_amd as D
    from diffute_amd import _cabi
    lib = _cabi.lib()
    lat, mask, mlat, ctx = inputs
    base = D.denoise(tiny_unet, D.DDIMScheduler(), lat, mask, mlat, ctx, 3)
    assert torch.equal(D.denoise(tiny_unet, D.DDIMScheduler(), lat, mask, mlat, ctx, 3, cache_interval=1), base)
    n0, o0 = _launches(lib, lambda: D.denoise(tiny_unet, D.DDIMScheduler(), lat, mask, mlat, ctx, 3).clone())
    n1, o1 = _launches(lib, lambda: D.denoise(tiny_unet, D.DDIMScheduler(), lat, mask, mlat, ctx, 3, cache_interval=1).clone())
    assert n0 == n1 and sum(n0) > 0, (n0, n1)
    assert torch.equal(o0, base) and torch.equal(o1, base)
    t = torch.tensor([501], device=cuda)
    tiny_unet.set_context(ctx)
    buf = tiny_unet.step_cache(2, 16, 16)
    plain, _ = _launches(lib, lambda: tiny_unet.forward_parts([lat, mask, mlat], t))
    fill, _ = _launches(lib, lambda: tiny_unet.forward_parts([lat, mask, mlat], t, step_cache=(buf, "fill")))
    use, _ = _launches(lib, lambda: tiny_unet.forward_parts([lat, mask, mlat], t, step_cache=(buf, "use")))
    print(f"launches per step: full {sum(plain)}, full + cache store {sum(fill)}, shallow {sum(use)} ({sum(use) / sum(plain):.3f} of a full step)")
    assert sum(fill) == sum(plain) + 1                   # (the store of the kept tensor and its statistics: one launch)
    assert 0 < sum(use) <= 0.5 * sum(plain)


# ------------------------------------------------------------------------------------------------ 6. pass-through
def test_edit_latents_passes_cache_interval(cuda, tiny_unet):
    import diffute_amd as D
    from diffute_amd.init import normal
    from diffute_amd.synthetic import text_crop_images
    vae = D.AutoencoderKL(**TINY_VAE).cuda().requires_grad_(False)
    img = text_crop_images(1, 128, 128, device=cuda)
    mask = torch.zeros(1, 1, 128, 128, device=cuda); mask[:, :, 48:80, 16:112] = 1.0
    masked = img * (mask < 0.5)
    ctx = normal(2, 13, 77 * 128, cuda).reshape(1, 77, 128)
    en = normal(4, 71, 4 * 16 * 16, cuda).reshape(1, 4, 16, 16)
    sf = vae.config.scaling_factor
    out = D.edit_latents(tiny_unet, vae, D.DDIMScheduler(), img, masked, mask, ctx, 3, enc_noise=en, cache_interval=2)
    mlat = vae.encode(masked).latent_dist.sample(noise=en) * sf
    init = torch.randn((1, 4, 16, 16), generator=torch.manual_seed(0), dtype=torch.float32).to(cuda)
    lat = D.denoise(tiny_unet, D.DDIMScheduler(), init, D.mask_to_latent(mask, 8), mlat, ctx, 3, cache_interval=2)
    with torch.no_grad():
        assert torch.equal(out, vae.decode(lat / sf).sample)
    plain = D.edit_latents(tiny_unet, vae, D.DDIMScheduler(), img, masked, mask, ctx, 3, enc_noise=en)
    assert torch.equal(plain, D.edit_latents(tiny_unet, vae, D.DDIMScheduler(), img, masked, mask, ctx, 3, enc_noise=en, cache_interval=1))
    lat1 = D.denoise(tiny_unet, D.DDIMScheduler(), init, D.mask_to_latent(mask, 8), mlat, ctx, 3)
    with torch.no_grad():
        assert torch.equal(plain, vae.decode(lat1 / sf).sample)
    assert not torch.equal(plain, out)


def test_edit_boxes_passes_cache_interval(cuda, tiny_unet):
    import diffute_amd as D
    from diffute_amd.init import normal
    vae = D.AutoencoderKL(**TINY_VAE).cuda().requires_grad_(False)
    img = torch.from_numpy(np.random.RandomState(11).randint(0, 256, (160, 192, 3), dtype=np.uint8)).to(cuda)
    boxes, origins, crops = [(40, 60, 150, 78), (20, 100, 100, 120)], [(30, 20), (10, 30)], [128, 96]
    ctx = normal(2, 13, 2 * 77 * 128, cuda).reshape(2, 77, 128)
    en = normal(4, 71, 2 * 4 * 16 * 16, cuda).reshape(2, 4, 16, 16)
    kw = dict(origins=origins, crop_scales=crops, enc_noise=en, return_intermediate=True, size=128)
    page1, vae1, _ = D.edit_boxes(tiny_unet, vae, D.DDIMScheduler(), img, boxes, ctx, 3, **kw)
    page1b, vae1b, _ = D.edit_boxes(tiny_unet, vae, D.DDIMScheduler(), img, boxes, ctx, 3, cache_interval=1, **kw)
    page2, vae2, _ = D.edit_boxes(tiny_unet, vae, D.DDIMScheduler(), img, boxes, ctx, 3, cache_interval=2, **kw)
    D.synchronize()
    assert torch.equal(page1, page1b) and torch.equal(vae1, vae1b)
    assert page2.shape == img.shape and page2.dtype == torch.uint8 and torch.isfinite(vae2).all()
    assert not torch.equal(vae2, vae1)
    with pytest.raises(ValueError, match="cache_interval"):
        D.edit_boxes(tiny_unet, vae, D.DDIMScheduler(), img, boxes, ctx, 3, cache_interval=0, **kw)


# ------------------------------------------------------------------------------------------------ 7. argument checks of the C ABI
def test_cached_forward_argument_checks(cuda, tiny_unet, inputs):
    """null or too-small cache, unknown mode: an error code and a message, nothing launched (`out` keeps its fill)"""
    from diffute_amd import _cabi
    lib = _cabi.lib()
    lat, mask, mlat, ctx = inputs
    tiny_unet.set_context(ctx)
    sl = tiny_unet._slot(0)
    t = torch.tensor([981], device=cuda)
    buf = tiny_unet.step_cache(2, 16, 16)
    ws = torch.empty(int(lib.dmx_unet_workspace_bytes_cached(tiny_unet._h, 2, 16, 16, 77)), dtype=torch.uint8, device=cuda)
    out = torch.full((2, 4, 16, 16), 7.0, device=cuda)
    assert buf.numel() == lib.dmx_unet_step_cache_bytes(tiny_unet._h, 2, 16, 16) >= 2 * 16 * 16 * 128 * 2 + 2 * 128 * 32
    assert ws.numel() >= lib.dmx_unet_workspace_bytes(tiny_unet._h, 2, 16, 16, 77)

    def call(fn, cache, nbytes, mode):
        return fn(tiny_unet._h, _cabi.ptr(lat), 4, _cabi.ptr(mask), 1, _cabi.ptr(mlat), 4, _cabi.ptr(t), 1, _cabi.ptr(sl["ctx_cache"]), 77,
                  _cabi.ptr(out), 2, 16, 16, cache, nbytes, mode, _cabi.ptr(ws), ws.numel(), _cabi.current_stream())
    for fn in (lib.dmx_unet_forward_cached, lib.dmx_unet_forward_cached_graph):
        for cache, nbytes, mode, word in ((None, buf.numel(), _cabi.STEP_CACHE_FILL, "null step cache"),
                                          (_cabi.ptr(buf), buf.numel() - 1, _cabi.STEP_CACHE_USE, "too small"),
                                          (_cabi.ptr(buf), buf.numel(), 0, "mode"), (_cabi.ptr(buf), buf.numel(), 3, "mode")):
            assert call(fn, cache, nbytes, mode) != 0
            with pytest.raises(RuntimeError, match=word):
                _cabi.check(1, "unet_forward_cached")
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())
    with pytest.raises(ValueError, match="step_cache mode"):
        tiny_unet.forward_parts([lat, mask, mlat], t, step_cache=(buf, "off"))
    with pytest.raises(ValueError, match="uint8 buffer"):
        tiny_unet.forward_parts([lat, mask, mlat], t, step_cache=(buf.float(), "fill"))
