"""DPMSolverMultistepScheduler on the GPU: the fused step kernel (dmx_sched_step_dpmpp) bit-exact against the test-local fp32
restatement of DPM-Solver++ (tests/dpm_restatement.py), the solver's convergence on data with a closed-form ODE solution, the
denoise() loop with the tiny UNet against the oracle forward composed with the restatement, and the full-size loop."""
import pytest
import torch

import dpm_restatement as R
from util import assert_close

pytestmark = pytest.mark.gpu
TINY_UNET = dict(block_out_channels=(64, 128, 256, 256), attention_head_dim=(1, 2, 4, 4), cross_attention_dim=128)


def _drive(order, solver_type, vpred, shape, n, seed):
    """step() over an n-step grid with seeded model outputs vs the restatement: prev_sample bit-equal at every step."""
    import diffute_amd as D
    s = D.DPMSolverMultistepScheduler(solver_order=order, solver_type=solver_type,
                                      prediction_type="v_prediction" if vpred else "epsilon")
    s.set_timesteps(n)
    ts = s.timesteps.tolist()
    tab = R.tables(s.alphas_cumprod)
    plan = R.orders(len(ts), order)
    assert [o for o, _ in s.step_plan()] == plan
    g = torch.Generator().manual_seed(seed)
    x_ref = torch.randn(shape, generator=g)
    x = x_ref.cuda()
    hist = []
    for i, t in enumerate(ts):
        out = torch.randn(shape, generator=g)
        x = s.step(out.cuda(), torch.tensor(t), x).prev_sample
        x_ref, m0 = R.step(tab, ts, i, x_ref, out, hist, plan[i], solver_type, vpred)
        hist.append(m0)
        got = x.cpu()
        assert torch.equal(got, x_ref), (f"order {order} {solver_type} vpred={vpred} shape {shape}: step {i} (t={t}, order {plan[i]}) "
                                         f"differs in {int((got != x_ref).sum())} elements, max {float((got - x_ref).abs().max()):.3e}")
    return plan


@pytest.mark.parametrize("vpred", [False, True])
@pytest.mark.parametrize("solver_type", ["midpoint", "heun"])
@pytest.mark.parametrize("order", [1, 2, 3])
def test_step_bit_exact(cuda, order, solver_type, vpred):
    plan = _drive(order, solver_type, vpred, (2, 4, 8, 8), 12, seed=10 * order + vpred)
    assert set(plan) == set(range(1, order + 1))                      # every order the solver uses was exercised
    _drive(order, solver_type, vpred, (1, 3, 5, 7), 12, seed=99)      # 105 elements: the n % 4 tail
    _drive(order, solver_type, vpred, (2, 4, 8, 8), 20, seed=7)       # no lower-order final steps (>= 15 steps)


def test_cabi_in_place_unaligned_and_refusals(cuda):
    """prev_sample == sample (what denoise() does), an operand off 16-byte alignment (the scalar path), and the argument checks."""
    import diffute_amd as D
    from diffute_amd import _cabi
    lib = _cabi.lib()
    s = D.DPMSolverMultistepScheduler(solver_order=3, solver_type="heun")
    s.set_timesteps(10)
    ts = s.timesteps.tolist()
    tab = R.tables(s.alphas_cumprod)
    plan = s.step_plan()
    g = torch.Generator().manual_seed(3)
    n = 4 * 4 * 9 * 9 + 3
    for offset in (0, 1):                                             # offset 1: every pointer 4 bytes past a 16-byte boundary
        bufs = [torch.empty(n + offset, device=cuda) for _ in range(4)]
        x_dev, e_dev, h0, h1 = [b[offset:] for b in bufs]
        h2 = torch.empty(n + offset, device=cuda)[offset:]
        ring = [h0, h1, h2]
        x_ref = torch.randn(n, generator=g)
        x_dev.copy_(x_ref)
        hist = []
        for i, (o, c) in enumerate(plan):
            e = torch.randn(n, generator=g)
            e_dev.copy_(e)
            m1 = ring[(i - 1) % 3] if o >= 2 else None
            m2 = ring[(i - 2) % 3] if o >= 3 else None
            _cabi.check(lib.dmx_sched_step_dpmpp(_cabi.ptr(x_dev), _cabi.ptr(e_dev), _cabi.ptr(m1), _cabi.ptr(m2), _cabi.ptr(ring[i % 3]),
                                                 _cabi.ptr(x_dev), n, o, _cabi.DpmCoefs(**c), 0, _cabi.current_stream()), "dpmpp")
            x_ref, m0 = R.step(tab, ts, i, x_ref, e, hist, o, "heun")
            hist.append(m0)
            assert torch.equal(ring[i % 3].cpu(), m0), f"offset {offset} step {i}: x0_out"
            assert torch.equal(x_dev.cpu(), x_ref), f"offset {offset} step {i}: in-place prev_sample"
    torch.cuda.synchronize()
    _, c2 = plan[1]
    args = lambda m1, m2, x0, prev, order: (_cabi.ptr(x_dev), _cabi.ptr(e_dev), _cabi.ptr(m1), _cabi.ptr(m2), _cabi.ptr(x0), _cabi.ptr(prev),
                                            n, order, _cabi.DpmCoefs(**c2), 0, _cabi.current_stream())
    assert lib.dmx_sched_step_dpmpp(*args(h0, None, h0, x_dev, 2)) != 0            # x0_out == m1
    assert b"x0_out overlaps" in lib.dmx_last_error()
    assert lib.dmx_sched_step_dpmpp(*args(h0, h1, h1, x_dev, 3)) != 0              # x0_out == m2
    assert lib.dmx_sched_step_dpmpp(*args(h0, None, x_dev, x_dev, 2)) != 0         # x0_out == prev_sample
    assert lib.dmx_sched_step_dpmpp(*args(None, None, h1, x_dev, 2)) != 0          # order 2 without m1
    assert lib.dmx_sched_step_dpmpp(*args(h0, h1, h2, x_dev, 4)) != 0              # no order 4
    _cabi.poll_device_error()


@pytest.mark.parametrize("order,solver_type,min_ratio", [(1, "midpoint", 1.8), (2, "midpoint", 2.7), (2, "heun", 2.7), (3, "midpoint", 3.5)])
def test_product_converges_on_gaussian_data(cuda, order, solver_type, min_ratio):
    """The product class, eps computed on the device from the closed-form predictor of x0 ~ N(mu, I): error ratio 80 -> 160 steps at the
    solver's order, as the restatement shows on the host (tests/test_dpm_solver_host.py)."""
    import diffute_amd as D
    errs = {}
    for n in (80, 160):
        s = D.DPMSolverMultistepScheduler(solver_order=order, solver_type=solver_type)
        s.set_timesteps(n)
        g = R.Gaussian(R.tables(s.alphas_cumprod), int(s.timesteps[0]))
        mu = g.mu.cuda()
        x = g.xT.cuda()
        for t in s.timesteps:
            a, sg = s.alpha_t[int(t)].item(), s.sigma_t[int(t)].item()
            eps = sg * (x - a * mu) / (a * a + sg * sg)
            x = s.step(eps, t, x).prev_sample
        errs[n] = g.rel_err(x)
    assert errs[80] / errs[160] >= min_ratio, errs
    if order == 2 and solver_type == "midpoint":
        s1 = D.DPMSolverMultistepScheduler(solver_order=1)
        s1.set_timesteps(160)
        g = R.Gaussian(R.tables(s1.alphas_cumprod), int(s1.timesteps[0]))
        mu, x = g.mu.cuda(), g.xT.cuda()
        for t in s1.timesteps:
            a, sg = s1.alpha_t[int(t)].item(), s1.sigma_t[int(t)].item()
            x = s1.step(sg * (x - a * mu) / (a * a + sg * sg), t, x).prev_sample
        assert errs[160] <= 0.35 * g.rel_err(x), (errs[160], g.rel_err(x))


@pytest.fixture(scope="module")
def tiny_unet(cuda):
    import diffute_amd as D
    return D.UNet2DConditionModel(**TINY_UNET).cuda().requires_grad_(False)


def _oracle_loop(lat, mask, mlat, ctx, n, emulate_bf16):
    """oracle.unet.unet_forward (weights as scripts/make_golden.py makes them) composed with the restated DPM-Solver++ 2M."""
    import diffute_amd as D
    from oracle import unet as OU
    P = OU.make_params(OU.unet_param_spec(OU.TINY_UNET), seed=1234)
    s = D.DPMSolverMultistepScheduler()
    s.set_timesteps(n)
    ts = s.timesteps.tolist()
    tab = R.tables(s.alphas_cumprod)
    plan = R.orders(len(ts), 2)
    x = lat.cpu().float()
    m, ml, c = mask.cpu().float(), mlat.cpu().float(), ctx.cpu().float()
    hist = []
    for i, t in enumerate(ts):
        eps = OU.unet_forward(P, OU.TINY_UNET, torch.cat([x, m, ml], 1), torch.tensor(t), c, emulate_bf16=emulate_bf16)
        x, m0 = R.step(tab, ts, i, x, eps, hist, plan[i])
        hist.append(m0)
    return x


@pytest.mark.parametrize("n", [10, 20])
def test_tiny_denoise_dpmpp_vs_oracle(cuda, tiny_unet, n):
    import diffute_amd as D
    from diffute_amd.synthetic import synth_inputs
    lat, mask, mlat, ctx = synth_inputs(2, 16, 16, 77, 128, device=cuda)
    out = D.denoise(tiny_unet, D.DPMSolverMultistepScheduler(), lat, mask, mlat, ctx, n)
    e16 = assert_close(out, _oracle_loop(lat, mask, mlat, ctx, n, True), 2e-2, f"tiny DPM++ 2M {n}-step loop vs bf16emu")
    e32 = assert_close(out, _oracle_loop(lat, mask, mlat, ctx, n, False), 5e-2, f"tiny DPM++ 2M {n}-step loop vs fp32")
    print(f"tiny DPM++ 2M {n} steps rel-L2: vs bf16emu {e16:.2e}, vs fp32 {e32:.2e}")


def test_tiny_denoise_dpmpp_loop_properties(cuda, tiny_unet):
    """The reference-shaped twin loop equals denoise(); micro-batches; repeat determinism; one scheduler object reused."""
    import diffute_amd as D
    from diffute_amd.synthetic import synth_inputs
    lat, mask, mlat, ctx = synth_inputs(2, 16, 16, 77, 128, device=cuda)
    sch = D.DPMSolverMultistepScheduler()
    out = D.denoise(tiny_unet, sch, lat, mask, mlat, ctx, 20)
    assert torch.isfinite(out).all()
    assert torch.equal(D.denoise(tiny_unet, D.DPMSolverMultistepScheduler(), lat, mask, mlat, ctx, 20), out)     # two runs
    assert torch.equal(D.denoise(tiny_unet, sch, lat, mask, mlat, ctx, 20), out)                                 # the same object again

    def twin():
        sch.set_timesteps(20)
        x = lat * sch.init_noise_sigma
        with torch.no_grad():
            for t in sch.timesteps:
                inp = torch.cat([sch.scale_model_input(x, t), mask, mlat], dim=1)
                eps = tiny_unet(inp, t, ctx).sample
                x = sch.step(eps, t, x).prev_sample
        return x
    assert torch.equal(twin(), out)
    assert torch.equal(twin(), out)                                  # set_timesteps restarts the history
    out_mb = D.denoise(tiny_unet, D.DPMSolverMultistepScheduler(), lat, mask, mlat, ctx, 20, micro_batches=2)
    assert_close(out_mb, out.cpu(), 1e-2, "micro-batched DPM++ loop vs the single chain")
    o3 = D.denoise(tiny_unet, D.DPMSolverMultistepScheduler(solver_order=3), lat, mask, mlat, ctx, 10)
    assert torch.isfinite(o3).all() and not torch.equal(o3, out)
    trace = []
    cb = D.denoise(tiny_unet, D.DPMSolverMultistepScheduler(), lat, mask, mlat, ctx, 20, callback=lambda i, t, x, eps: trace.append((i, t)))
    assert trace == list(enumerate(sch.timesteps.tolist())) and torch.equal(cb, out)            # the callback sees every step
    with pytest.raises(ValueError):
        D.denoise(tiny_unet, D.DPMSolverMultistepScheduler(), lat, mask, mlat, ctx, 10, eta=0.5)
    with pytest.raises(ValueError):
        D.denoise(tiny_unet, D.DPMSolverMultistepScheduler(), lat, mask, mlat, ctx, 10, variance_noise=torch.zeros(10, 2, 4, 16, 16, device=cuda))


def test_edit_latents_with_dpmpp(cuda, tiny_unet):
    """edit_latents() takes the new scheduler: encode -> DPM-Solver++ denoise -> decode, equal to the same three calls made by hand."""
    import diffute_amd as D
    from diffute_amd.init import normal
    from diffute_amd.synthetic import text_crop_images
    vae = D.AutoencoderKL(block_out_channels=(64, 128, 128, 128), layers_per_block=1).cuda().requires_grad_(False)
    img = text_crop_images(1, 128, 128, device=cuda)
    mask = torch.zeros(1, 1, 128, 128, device=cuda); mask[:, :, 48:80, 16:112] = 1.0
    masked = img * (mask < 0.5)
    ctx = normal(2, 13, 77 * 128, cuda).reshape(1, 77, 128)
    en = normal(4, 71, 4 * 16 * 16, cuda).reshape(1, 4, 16, 16)
    init = normal(5, 72, 4 * 16 * 16, cuda).reshape(1, 4, 16, 16)
    out = D.edit_latents(tiny_unet, vae, D.DPMSolverMultistepScheduler(), img, masked, mask, ctx, 10, init_latents=init, enc_noise=en)
    sf = vae.config.scaling_factor
    with torch.no_grad():
        mlat = vae.encode(masked).latent_dist.sample(noise=en) * sf
        lat = D.denoise(tiny_unet, D.DPMSolverMultistepScheduler(), init, D.mask_to_latent(mask, 8), mlat, ctx, 10)
        ref = vae.decode(lat / sf).sample
    assert torch.isfinite(out).all() and torch.equal(out, ref)
    with pytest.raises(ValueError):
        D.edit_latents(tiny_unet, vae, D.DPMSolverMultistepScheduler(), img, masked, mask, ctx, 10, init_latents=init, enc_noise=en,
                       variance_noise=torch.zeros(10, 1, 4, 16, 16, device=cuda))


def test_full_size_dpmpp_20_steps(cuda):
    """512 px, batch 4, 20 steps of DPM++ 2M with the full SD2-inpaint UNet: finite, and bit-equal across two passes."""
    import diffute_amd as D
    from diffute_amd.synthetic import synth_inputs
    unet = D.UNet2DConditionModel(device=cuda).requires_grad_(False)
    lat, mask, mlat, ctx = synth_inputs(4, 64, 64, 577, 1024, device=cuda)
    a = D.denoise(unet, D.DPMSolverMultistepScheduler(), lat, mask, mlat, ctx, 20)
    keep = a.clone()
    b = D.denoise(unet, D.DPMSolverMultistepScheduler(), lat, mask, mlat, ctx, 20)
    torch.cuda.synchronize()
    assert torch.isfinite(keep).all() and torch.equal(keep, b)
