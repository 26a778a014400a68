"""dmx_diffusion_loss on the GPU, both builds of the library: dpred bit for bit against the float32 restatement, the per-sample sums inside the
bound that follows from the kernel's documented reduction shape, the loss bit for bit against the restated fold of the kernel's own records
(tests/loss_restatement.py: verify), the plain case against dmx_mse_loss and dmx_sched_get_velocity, row independence, guard bands,
out-of-range timesteps, autograd and train_step.

Shapes: C*hw = 4*5*7 = 140 (hw = 35: the mask is read as scalars, the rest as 16-byte quads), 3*5*7 = 105 (not a multiple of 4: a scalar last
quad, and rows 1 and 2 of a batch start off a 16-byte boundary and are read as scalars throughout), 4*8*8 (one pass of one block), 4*8*24
(non-square), 4*64*64 (the real span: 8 blocks per sample); B = 1 and 3; timesteps 0, 500, 999; masks all zero, all one, a rectangle, none."""
import numpy as np
import pytest
import torch

import loss_restatement as R

pytestmark = pytest.mark.gpu

SHAPES = [(1, 4, 5, 7), (3, 4, 5, 7), (3, 3, 5, 7), (1, 4, 8, 8), (3, 4, 8, 24), (1, 4, 64, 64), (3, 4, 64, 64)]
MASKS = ("zero", "one", "rect", None)
SENTINEL = -12345.678
GUARD = 64                     # floats either side of an output (256 bytes: the output keeps its 16-byte alignment)
TINY_UNET = dict(block_out_channels=(64, 128, 256, 256), attention_head_dim=(1, 2, 4, 4), cross_attention_dim=128)      # tests/test_models_gpu.py
TINY_VAE = dict(block_out_channels=(64, 128, 128, 128), layers_per_block=1)
_SCHED = {}


def sched(pt):
    import diffute_amd as D
    if pt not in _SCHED:
        _SCHED[pt] = D.DDPMScheduler(prediction_type=pt)
    return _SCHED[pt]


def tables(pt):
    sa, sb = sched(pt)._coef_tables("cpu")
    return dict(abar=sched(pt).alphas_cumprod.numpy(), sa=sa.numpy(), sb=sb.numpy())


def timesteps(B):
    return [0, 500, 999] if B == 3 else [500]


def bits(t):
    return t.contiguous().view(torch.int32)


def dev(case, cuda):
    g = {k: torch.from_numpy(case[k]).to(cuda) for k in ("pred", "x0", "noise", "t", "sa", "sb", "wt")}
    g["mask"] = None if case["mask"] is None else torch.from_numpy(case["mask"]).to(cuda)
    return g


def call(case, g, *, dpred=True, grad_scale=1.0, guard=GUARD):
    """-> (dpred or None, records, loss) as numpy; the outputs are written into sentinel-filled buffers whose guard bands are checked"""
    from diffute_amd import ops
    N, B = case["pred"].size, case["pred"].shape[0]
    dbuf = torch.full((N + 2 * guard,), SENTINEL, device=g["pred"].device)
    rbuf = torch.full((B * 5 + 2 * guard,), SENTINEL, device=g["pred"].device)
    lbuf = torch.full((1 + 2 * guard,), SENTINEL, device=g["pred"].device)
    dp = dbuf[guard:guard + N].view(case["pred"].shape) if dpred else None
    loss, rec, out = ops.diffusion_loss(g["pred"], g["x0"], g["noise"], g["t"], g["sa"], g["sb"], g["wt"], mask=g["mask"], v_prediction=case["v_prediction"],
                                        mask_weight=case["mask_weight"], grad_scale=grad_scale, dpred=dp, loss=lbuf[guard:guard + 1],
                                        records=rbuf[guard:guard + B * 5].view(B, 5))
    assert (out is None) == (not dpred)
    for name, buf, n in (("dpred", dbuf, N if dpred else 0), ("records", rbuf, B * 5), ("loss", lbuf, 1)):
        h = buf.cpu().numpy()
        s = np.float32(SENTINEL)
        assert (h[:guard] == s).all() and (h[guard + n:] == s).all(), f"{name}: a guard band was written"
        assert not (h[guard:guard + n] == s).any(), f"{name}: an element was not written"
    return (dbuf[guard:guard + N].view(case["pred"].shape).cpu().numpy() if dpred else None), rbuf[guard:guard + B * 5].view(B, 5).cpu().numpy(), \
        lbuf[guard:guard + 1].cpu().numpy()


def same(a, b):
    return np.array_equal(R.bits(a), R.bits(b))


@pytest.fixture(params=["bf16", "fp16"])
def build(request, cuda):
    from diffute_amd import ops
    with ops.element_type(request.param):
        yield request.param


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_kernel_against_the_restatement(cuda, build, shape):
    for pt, gamma, lam in (("epsilon", None, 0.0), ("epsilon", 5.0, 4.0), ("v_prediction", 5.0, 4.0), ("v_prediction", None, 0.5)):
        for mk in MASKS:
            case = R.make_case(tables(pt), shape, timesteps(shape[0]), mk, pt, gamma, lam, seed=100 * shape[0] + shape[2])
            g = dev(case, cuda)
            dp, rec, loss = call(case, g)
            R.verify(case, dp, rec, loss)
            dp2, rec2, loss2 = call(case, g)
            assert same(dp, dp2) and same(rec, rec2) and same(loss, loss2), "two runs differ"
            _, rec3, loss3 = call(case, g, dpred=False)                      # dpred = NULL: loss and records only, the same bits
            assert same(rec, rec3) and same(loss, loss3), "dpred = NULL changes the loss or the records"
            if mk is None:
                assert (rec[:, 1] == 0).all() and (rec[:, 3] == 0).all() and same(rec[:, 0], rec[:, 2])
            if mk == "one":
                assert (rec[:, 3] == shape[2] * shape[3]).all() and same(rec[:, 0], rec[:, 1])


def test_both_builds_agree_and_alignment_does_not_matter(cuda):
    """fp32 throughout: the bf16 and the fp16 build give the same bits; outputs and inputs one float off a 16-byte boundary (the scalar path) too"""
    from diffute_amd import ops
    case = R.make_case(tables("v_prediction"), (3, 4, 64, 64), [0, 500, 999], "rect", "v_prediction", 5.0, 4.0, seed=11)
    g = dev(case, cuda)
    want = call(case, g)
    with ops.element_type("fp16"):
        got = call(case, g)
    assert all(same(a, b) for a, b in zip(want, got))
    off = dict(g)
    for k in ("pred", "x0", "noise", "mask"):
        buf = torch.empty(g[k].numel() + 1, device=cuda)
        buf[1:].copy_(g[k].reshape(-1))
        off[k] = buf[1:].view(g[k].shape)
        assert off[k].data_ptr() % 16 == 4
    got = call(case, off, guard=GUARD + 1)
    assert all(same(a, b) for a, b in zip(want, got))


def _mse_depth(n):
    """dmx_mse_loss: a grid-stride sum over min(ceil(n / 256), 1024) blocks of 256, a tree per block, then one block over the block sums"""
    nb = min(-(-n // 256), 1024)
    return -(-n // (nb * 256)) + 8 + -(-nb // 256) + 8


@pytest.mark.parametrize("pt", ["epsilon", "v_prediction"])
@pytest.mark.parametrize("shape", [(3, 4, 5, 7), (3, 4, 64, 64)], ids=lambda s: "x".join(map(str, s)))
def test_plain_case_is_the_mse_loss(cuda, build, pt, shape):
    """wt = 1, lambda = 0: dpred is dmx_mse_loss's bit for bit on the target the parent materialises (the noise; dmx_sched_get_velocity's output
    for a v model, which pins the in-kernel target to that kernel's bits), and the two losses agree inside the sum of their bounds"""
    from diffute_amd import ops
    case = R.make_case(tables(pt), shape, [0, 500, 999], None, pt, None, 0.0, seed=5)
    g = dev(case, cuda)
    dp, rec, loss = call(case, g)
    target = g["noise"] if pt == "epsilon" else sched(pt).get_velocity(g["x0"], g["noise"], g["t"])
    mloss, mdp = ops.mse_loss(g["pred"], target)
    assert same(dp, mdp.cpu().numpy()), "dpred differs from dmx_mse_loss's on the materialised target"
    B, S = shape[0], shape[1] * shape[2] * shape[3]
    l64 = R.sums64(case)[:, 0].sum() / (B * S)
    # ours: k adds + 3 roundings of a term, the fold's B adds, 1 / N rounded, one multiplication; dmx_mse_loss: its own depth + 3 + the same 2
    lim = (R.bound(R.depth(S) + B + 2, 3) + R.bound(_mse_depth(B * S) + 2, 3)) * l64
    print(f"loss {float(loss[0])!r} mse_loss {float(mloss)!r} float64 {l64!r} bound {lim:.3e}")
    assert abs(float(loss[0]) - float(mloss)) <= lim


@pytest.mark.parametrize("shape", [(3, 3, 5, 7), (3, 4, 8, 24), (3, 4, 64, 64)], ids=lambda s: "x".join(map(str, s)))
def test_rows_are_independent(cuda, build, shape):
    """row b of a B = 3 call and the B = 1 call on that sample: the same record and the same dpred row, bit for bit.  (dpred carries
    gs = (float)(2 g / N): g = 3 in the batch of three and g = 1 alone are the same real number 2 / (C hw), hence the same float.)"""
    case = R.make_case(tables("v_prediction"), shape, [0, 500, 999], "rect", "v_prediction", 5.0, 4.0, seed=7)
    dp, rec, _ = call(case, dev(case, cuda), grad_scale=3.0)
    for b in range(3):
        one = {k: (v[b:b + 1].copy() if k in ("pred", "x0", "noise", "mask", "t") else v) for k, v in case.items()}
        dp1, rec1, loss1 = call(one, dev(one, cuda))
        R.verify(one, dp1, rec1, loss1)
        assert same(dp[b:b + 1], dp1) and same(rec[b:b + 1], rec1), f"row {b} of the batch differs from the sample alone"


@pytest.mark.parametrize("bad", [1000, -1, 1 << 40, -(1 << 62)])
def test_out_of_range_timestep(cuda, build, bad):
    """a timestep outside [0, T) in row 1 of 3: its weight, its dpred rows and the loss are NaN, nothing is read outside the tables (the index is
    clamped), rows 0 and 2 are bit-equal to a clean run"""
    for pt in ("epsilon", "v_prediction"):
        clean = R.make_case(tables(pt), (3, 4, 8, 24), [0, 500, 999], "rect", pt, 5.0, 4.0, seed=9)
        case = dict(clean, t=np.asarray([0, bad, 999], np.int64))
        dpc, recc, _ = call(clean, dev(clean, cuda))
        dp, rec, loss = call(case, dev(case, cuda))
        R.verify(case, dp, rec, loss)
        assert np.isnan(rec[1, 4]) and np.isnan(dp[1]).all() and np.isnan(loss[0])
        assert np.isfinite(rec[1, :4]).all()
        for b in (0, 2):
            assert same(dp[b], dpc[b]) and same(rec[b], recc[b]), f"row {b} differs from the clean run"


def test_autograd_and_derived_fields(cuda):
    from diffute_amd.training import diffusion_loss
    pt = "v_prediction"
    case = R.make_case(tables(pt), (3, 4, 8, 24), [0, 500, 999], "rect", pt, 5.0, 4.0, seed=13)
    g = dev(case, cuda)
    want_dp, want_rec, want_loss = call(case, g)
    kw = dict(mask=g["mask"], snr_gamma=5.0, mask_weight=4.0)
    pred = g["pred"].clone().requires_grad_(True)
    out = diffusion_loss(pred, g["x0"], g["noise"], g["t"], sched(pt), **kw)
    assert out.loss.shape == () and out.loss.requires_grad and not out.records.requires_grad
    out.loss.backward()
    assert same(pred.grad.cpu().numpy(), want_dp) and same(out.records.cpu().numpy(), want_rec) and same(out.loss.detach().cpu().numpy(), want_loss)
    pred2 = g["pred"].clone().requires_grad_(True)
    (diffusion_loss(pred2, g["x0"], g["noise"], g["t"], sched(pt), **kw).loss * 1024.0).backward()
    assert same(pred2.grad.cpu().numpy(), want_dp * np.float32(1024))
    C, hw = 4, 8 * 24
    rec = want_rec.astype(np.float64)
    np.testing.assert_allclose(out.per_sample_mse.cpu().numpy(), rec[:, 0] / (C * hw), rtol=1e-6)
    np.testing.assert_allclose(out.masked_mse.cpu().numpy(), rec[:, 1] / (C * rec[:, 3]), rtol=1e-6)
    np.testing.assert_allclose(out.unmasked_mse.cpu().numpy(), (rec[:, 0] - rec[:, 1]) / (C * (hw - rec[:, 3])), rtol=1e-6)
    assert same(out.weight.cpu().numpy(), want_rec[:, 4])
    # no mask: nothing is inside a box
    out = diffusion_loss(g["pred"], g["x0"], g["noise"], g["t"], sched(pt))
    assert torch.isnan(out.masked_mse).all() and torch.equal(out.unmasked_mse, out.per_sample_mse) and bool((out.weight == 1).all())
    zero = diffusion_loss(g["pred"], g["x0"], g["noise"], g["t"], sched(pt), mask=torch.zeros_like(g["mask"]))
    assert torch.isnan(zero.masked_mse).all() and torch.equal(bits(zero.records[:, :3]), bits(out.records[:, :3]))


def test_train_step(cuda):
    """defaults given explicitly = defaults left out, bit for bit; the weighted step returns the extra keys and its loss is diffusion_loss on the
    same injected draws, bit for bit (each from a fresh model: equal seeds, equal weights)"""
    import diffute_amd as D
    from diffute_amd.training import diffusion_loss, encode_latents, train_step
    vae = D.AutoencoderKL(**TINY_VAE).cuda().requires_grad_(False)
    sch = D.DDPMScheduler()
    gen = torch.Generator(device=cuda).manual_seed(7)
    B = 2
    masks = torch.zeros(B, 1, 128, 128, device=cuda); masks[0, :, 32:64, 16:112] = 1; masks[1, :, 80:104, 8:72] = 1
    batch = dict(pixel_values=torch.rand(B, 3, 128, 128, device=cuda, generator=gen) * 2 - 1,
                 masked_images=torch.rand(B, 3, 128, 128, device=cuda, generator=gen) * 2 - 1, masks=masks,
                 ocr_embeddings=torch.randn(B, 77, 128, device=cuda, generator=gen))
    draws = dict(noise=torch.randn(B, 4, 16, 16, device=cuda, generator=gen), timesteps=torch.tensor([700, 150], device=cuda),
                 enc_noise=torch.randn(B, 4, 16, 16, device=cuda, generator=gen), enc_noise_masked=torch.randn(B, 4, 16, 16, device=cuda, generator=gen))

    def fresh():
        unet = D.UNet2DConditionModel(**TINY_UNET).cuda()
        return unet, D.FusedAdamW(unet, lr=2e-4, weight_decay=1e-2, max_grad_norm=1.0)

    unet, opt = fresh()
    a = train_step(unet, vae, sch, opt, batch, **draws)
    unet, opt = fresh()
    b = train_step(unet, vae, sch, opt, batch, **draws, snr_gamma=None, mask_weight=0.0)
    assert set(a) == set(b) == {"loss", "grad_norm"}
    assert torch.equal(bits(a["loss"]), bits(b["loss"])) and torch.equal(a["grad_norm"], b["grad_norm"])
    unet, opt = fresh()
    c = train_step(unet, vae, sch, opt, batch, **draws, snr_gamma=5.0, mask_weight=4.0)
    assert set(c) == {"loss", "grad_norm", "per_sample_mse", "masked_mse", "unmasked_mse", "timesteps"}
    assert torch.isfinite(c["loss"]) and torch.isfinite(c["grad_norm"]) and torch.equal(c["timesteps"], draws["timesteps"])
    assert all(c[k].shape == (B,) and torch.isfinite(c[k]).all() for k in ("per_sample_mse", "masked_mse", "unmasked_mse"))
    assert not torch.equal(c["loss"], a["loss"])
    unet, _ = fresh()
    both = encode_latents(vae, torch.cat([batch["pixel_values"], batch["masked_images"]], 0), torch.cat([draws["enc_noise"], draws["enc_noise_masked"]], 0))
    lat, mlat = both[:B].contiguous(), both[B:].contiguous()
    mask = D.mask_to_latent(masks, 8).to(lat.dtype)
    noisy = sch.add_noise(lat, draws["noise"], draws["timesteps"])
    pred = unet(torch.cat([noisy, mask, mlat], 1), draws["timesteps"], batch["ocr_embeddings"]).sample
    again = diffusion_loss(pred.float(), lat, draws["noise"], draws["timesteps"], sch, mask=mask, snr_gamma=5.0, mask_weight=4.0)
    assert torch.equal(bits(again.loss.detach()), bits(c["loss"])) and torch.equal(bits(again.masked_mse), bits(c["masked_mse"]))
