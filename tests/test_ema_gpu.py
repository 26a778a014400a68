"""diffute_amd.EMAModel on the GPU: the multi-tensor kernels (dmx_ema_step_multi / dmx_copy_multi) bit-exact against
diffusers' arithmetic run by torch (tests/ema_restatement.py), the reference's `--use_ema` flow on the tiny UNet with
FusedAdamW (EMA over the master arena, no per-step sync) and with torch.optim.AdamW, store / copy_to / restore in the
middle of training, the save / load hooks (train_diffute_v1.py:642-678,934-935) and the full-size step."""
import os

import pytest
import torch

import ema_restatement as R

pytestmark = pytest.mark.gpu
TINY_UNET = dict(block_out_channels=(64, 128, 256, 256), attention_head_dim=(1, 2, 4, 4), cross_attention_dim=128)
DTYPES = (torch.float32, torch.bfloat16, torch.float16)


@pytest.fixture(scope="module")
def cuda():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def _view(n, dtype, offset, g, dev):
    """a contiguous tensor of n elements at `offset` elements into a larger buffer (misaligned for odd offsets)"""
    buf = torch.randn(n + offset + 3, generator=g).to(dtype).to(dev)
    return buf[offset:offset + n]


def test_kernel_bit_exact_all_dtype_pairs(cuda):
    from diffute_amd import EMAModel
    g = torch.Generator().manual_seed(11)
    sizes = [1, 3, 4, 5, 7, 64, 4097, 65536 + 13, 3 * 65536, 200003]
    pairs = [(sd, pd) for sd in DTYPES for pd in DTYPES]
    params, shadows = [], []
    for i in range(45):
        sd, pd = pairs[i % 9]
        n = sizes[i % len(sizes)]
        p = _view(n, pd, (i % 3) * (i % 5), g, cuda)
        p.requires_grad_(i % 7 != 3)
        params.append(p)
        shadows.append(_view(n, sd, (i % 4), g, cuda))
    hp = dict(update_after_step=2, use_ema_warmup=True, inv_gamma=1.0, power=0.75, decay=0.999)
    ema = EMAModel(params, **hp)
    ema.shadow_params = list(shadows)                         # misaligned shadows with the pair's dtype
    # references: torch's type-promotion semantics evaluated on the CPU for every tensor, and torch on the GPU for every tensor
    # whose evaluation there follows the same semantics.  (Observed with torch 2.10 / ROCm: for tensors of more than 64 Ki elements
    # with a 16-bit shadow and an fp32 intermediate, the in-place `s.sub_(m)` on the GPU rounds differently - 1-ulp differences
    # AWAY from the exactly rounded value - so those tensors are checked against the CPU evaluation only.)
    ref = [s.clone() for s in shadows]
    cpu = [s.cpu().clone() for s in shadows]
    gpu_ok = [s.dtype == p.dtype or s.dtype == torch.float32 or n <= 65536 for s, p, n in zip(shadows, params, [p.numel() for p in params])]
    for i in range(1, 11):
        with torch.no_grad():
            for p in params:
                p.add_(torch.randn(p.shape, generator=g).to(p.dtype).to(cuda) * 0.05)
        ema.step(params)
        dv = R.get_decay(i, **hp)
        R.step(ref, params, dv)
        R.step(cpu, [p.detach().cpu().requires_grad_(p.requires_grad) for p in params], dv)
        for k, (a, b, c) in enumerate(zip(ema.shadow_params, ref, cpu)):
            what = f"step {i} tensor {k} ({a.dtype} <- {params[k].dtype}, n={a.numel()}, rg={params[k].requires_grad})"
            assert a.dtype == c.dtype and torch.equal(a.cpu(), c), f"{what}: {int((a.cpu() != c).sum())} elements differ from the CPU evaluation"
            if gpu_ok[k]:
                assert torch.equal(a, b), f"{what}: {int((a != b).sum())} elements differ from torch on the GPU"
            else:
                b.copy_(a)                                   # (keep the GPU restatement on the exact trajectory)
    tgt = [_view(p.numel(), p.dtype, 1, g, cuda) for p in params]
    tgt_ref = [t.clone() for t in tgt]
    ema.copy_to(tgt)
    R.copy_to(ref, tgt_ref)
    for a, b in zip(tgt, tgt_ref):
        assert torch.equal(a, b)


def _inputs(dev):
    from diffute_amd.synthetic import synth_inputs
    lat, mask, mlat, ctx = synth_inputs(1, 8, 8, 20, 128, device=dev)
    return torch.cat([lat, mask, mlat], 1), torch.tensor([500], device=dev), ctx, torch.zeros(1, 4, 8, 8, device=dev)


def _train(unet, opt, ema, inp, steps, fused):
    from diffute_amd.models import mse_loss
    x, t, ctx, tgt = inp
    dirty = []
    for _ in range(steps):
        loss = mse_loss(unet(x, t, ctx).sample, tgt)
        loss.backward()
        opt.step()
        opt.zero_grad(set_to_none=True)
        if ema is not None:
            ema.step(unet.parameters())
            if fused:
                dirty.append(opt.dirty)
    return dirty


def _masters(unet, opt):
    """the FusedAdamW master weights in torch layouts, in unet.parameters() order, without touching the optimizer's state"""
    lib = unet._lib
    from diffute_amd import _cabi
    out = []
    for k, p in unet.named_parameters():
        d = torch.empty(p.shape, dtype=torch.float32, device=p.device)
        _cabi.check(lib.dmx_unet_grad_export(unet._h, _cabi.ptr(opt.masters), k.encode(), _cabi.ptr(d), _cabi.current_stream()), "export")
        out.append(d)
    return out


def _tiny_dir(tmp_path):
    import diffute_amd as D
    d = os.path.join(str(tmp_path), "unet")
    D.UNet2DConditionModel(**TINY_UNET).save_pretrained(d)
    return d


def test_reference_flow_fused_and_torch_adamw(cuda, tmp_path):
    import diffute_amd as D
    from diffute_amd import EMAModel
    d = _tiny_dir(tmp_path)
    inp = _inputs(cuda)
    for fused in (True, False):
        unet = D.UNet2DConditionModel.from_pretrained(d).cuda()
        ema_unet = D.UNet2DConditionModel.from_pretrained(d)
        ema = EMAModel(ema_unet.parameters(), model_cls=D.UNet2DConditionModel, model_config=ema_unet.config)
        ema.to(cuda)
        opt = D.FusedAdamW(unet, lr=1e-3) if fused else torch.optim.AdamW(unet.parameters(), lr=1e-3)
        ref = [s.clone() for s in ema.shadow_params]
        x, t, ctx, tgt = inp
        from diffute_amd.models import mse_loss
        for i in range(1, 5):
            mse_loss(unet(x, t, ctx).sample, tgt).backward()
            opt.step()
            opt.zero_grad(set_to_none=True)
            ema.step(unet.parameters())
            if fused:
                assert opt.dirty, "the fused EMA step synchronised the optimizer's Parameters"
                weights = [w.requires_grad_(True) for w in _masters(unet, opt)]     # (every parameter trains: the EMA branch)
            else:
                weights = list(unet.parameters())
            R.step(ref, weights, R.get_decay(i))
        for k, (a, b) in enumerate(zip(ema.shadow_params, ref)):
            assert torch.equal(a, b), f"fused={fused}: shadow {k} differs in {int((a != b).sum())} elements"
        if fused:
            opt.sync_to_model()
            assert all(torch.equal(a, p.detach()) for a, p in zip(_masters(unet, opt), unet.parameters()))
            # FusedAdamW's own in-kernel EMA (ema_decay=0.9999) on the same trajectory: within 1e-5 relative, not bit-equal
            u3 = D.UNet2DConditionModel.from_pretrained(d).cuda()
            o3 = D.FusedAdamW(u3, lr=1e-3, ema_decay=0.9999)
            _train(u3, o3, None, inp, 4, True)
            own = o3.ema_state_dict()
            names = [k for k, _ in unet.named_parameters()]
            for k, s in zip(names, ema.shadow_params):
                err = float((own[k] - s).abs().max() / (s.abs().max() + 1e-12))
                assert err <= 1e-5, f"{k}: FusedAdamW(ema_decay) vs EMAModel {err:.2e}"


def test_store_copy_to_restore_continues_training(cuda, tmp_path):
    import diffute_amd as D
    from diffute_amd import EMAModel
    d = _tiny_dir(tmp_path)
    inp = _inputs(cuda)
    x, t, ctx, tgt = inp
    runs = {}
    for mode in ("A", "B"):
        unet = D.UNet2DConditionModel.from_pretrained(d).cuda()
        opt = D.FusedAdamW(unet, lr=1e-3)
        ema = EMAModel(unet.parameters(), decay=0.9)
        if mode == "A":
            _train(unet, opt, ema, inp, 3, True)
            ema.store(unet.parameters())
            ema.copy_to(unet.parameters())
            with torch.no_grad():
                out_ema = unet(x, t, ctx).sample.clone()
            fresh = D.UNet2DConditionModel(**TINY_UNET).cuda()
            fresh.load_state_dict(dict(zip([k for k, _ in unet.named_parameters()], ema.shadow_params)))
            with torch.no_grad():
                out_fresh = fresh(x, t, ctx).sample
            assert torch.equal(out_ema, out_fresh), "the forward after copy_to does not run the EMA weights"
            ema.restore(unet.parameters())
            _train(unet, opt, ema, inp, 2, True)
        else:
            _train(unet, opt, ema, inp, 5, True)
        with torch.no_grad():
            out = unet(x, t, ctx).sample.clone()
        runs[mode] = (opt.masters.clone(), opt.exp_avg.clone(), opt.exp_avg_sq.clone(), out, [s.clone() for s in ema.shadow_params])
    for i, nm in enumerate(("masters", "exp_avg", "exp_avg_sq", "final forward")):
        assert torch.equal(runs["A"][i], runs["B"][i]), f"{nm} differs after store / copy_to / restore"
    assert all(torch.equal(a, b) for a, b in zip(runs["A"][4], runs["B"][4]))


def test_save_and_load_hooks_round_trip(cuda, tmp_path):
    import diffute_amd as D
    from diffute_amd import EMAModel
    d = _tiny_dir(tmp_path)
    inp = _inputs(cuda)
    res = []
    for save in (True, False):
        unet = D.UNet2DConditionModel.from_pretrained(d).cuda()
        ema_unet = D.UNet2DConditionModel.from_pretrained(d)
        ema = EMAModel(ema_unet.parameters(), model_cls=D.UNet2DConditionModel, model_config=ema_unet.config)
        ema.to(cuda)
        opt = D.FusedAdamW(unet, lr=1e-3)
        _train(unet, opt, ema, inp, 2, True)
        if save:
            out = os.path.join(str(tmp_path), "ckpt", "unet_ema")
            ema.save_pretrained(out)                                            # save hook (:664-666)
            load_model = EMAModel.from_pretrained(out, D.UNet2DConditionModel)  # load hook (:674-678)
            ema.load_state_dict(load_model.state_dict())
            ema.to(cuda)
            del load_model
            assert ema.optimization_step == 2
        _train(unet, opt, ema, inp, 1, True)
        res.append([s.clone() for s in ema.shadow_params])
    assert all(torch.equal(a, b) for a, b in zip(*res))


def test_full_size_step(cuda):
    import diffute_amd as D
    from diffute_amd import EMAModel
    unet = D.UNet2DConditionModel(device=cuda)
    params = list(unet.parameters())
    assert len(params) == 686 and sum(p.numel() for p in params) == 865_925_124
    start = [p.detach().clone() for p in params]

    def factor(i, j):
        return 1.0 + 1e-3 * ((i + j) % 5 - 2)
    runs = []
    for _ in range(2):
        with torch.no_grad():
            for p, s0 in zip(params, start):
                p.copy_(s0)
        ema = EMAModel(params, decay=0.999)
        for i in range(3):
            with torch.no_grad():
                for j, p in enumerate(params):
                    p.mul_(factor(i, j))
            ema.step(params)
        runs.append([s.clone() for s in ema.shadow_params])
        del ema
    a, b = runs
    assert all(torch.isfinite(s).all() for s in a)
    assert all(torch.equal(x, y) for x, y in zip(a, b)), "full-size step not bit-repeatable"
    # per-tensor torch evaluation on a sample of 20 tensors
    idx = list(range(0, 686, 35))[:20]
    ref = [start[k].clone() for k in idx]
    cur = [start[k].clone().requires_grad_(True) for k in idx]
    for i in range(3):
        with torch.no_grad():
            for c, k in zip(cur, idx):
                c.mul_(factor(i, k))
        R.step(ref, cur, R.get_decay(i + 1, decay=0.999))
    for n, k in enumerate(idx):
        assert torch.equal(b[k], ref[n]), f"tensor {k}"
