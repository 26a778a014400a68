"""The training path as the reference drives it: the HIP models under accelerate (train_diffute_v1.py:581-587,780,873-930;
train_vae.py:466,635,716-736) - `Accelerator.prepare`, `accelerator.accumulate`, torch's own F.mse_loss, `accelerator.backward`,
`accelerator.clip_grad_norm_`, torch.optim.AdamW, a LambdaLR warm-up - against a twin model run through the plain loop of
tests/accelerate_loops.py (which tests/test_accelerate_host.py pins to accelerate on the CPU).

Per leg (UNet with mixed_precision no / bf16 / fp16, VAE with no), two optimizer steps of two micro-steps on four different micro-batches:
 (a) bit identity with the twin: every loss, every .grad after every micro-step, every parameter after every optimizer step.  The twin runs
     WITHOUT autocast: a HIP model computes in the precision of its build whatever torch.autocast says, the wrappers add no arithmetic, `loss / 2`
     is a power-of-two scale and the HIP step is deterministic - so nothing may differ, under bf16 / fp16 autocast either;
 (b) the gradient accumulated over the first window, before the clip, against fp32 autograd over the oracle of 0.5 (loss_1 + loss_2), at the
     bars of test_tiny_unet_train_step / test_tiny_vae_train_step (no / bf16 legs);
 (c) the clip clips, and returns the fp64 norm of those gradients to fp32 rounding (1e-5);
 (d) a no-grad forward of the trained model equals a brand-new model loaded with its state_dict: the packed weights followed torch's optimizer;
 (e) sync_gradients reads False, True, False, True; AdamW counted 2 steps; the learning rate follows the warm-up.
The fp16 leg runs until an optimizer step is not skipped (at most 4: GradScaler starts at 2^16) and needs at least one.

This file starts no process."""
import pytest
import torch

from util import grad_errors, oracle_unet_train_grads

pytest.importorskip("accelerate")
import accelerate_loops as AL  # noqa: E402

pytestmark = pytest.mark.gpu
TINY_UNET = dict(block_out_channels=(64, 128, 256, 256), attention_head_dim=(1, 2, 4, 4), cross_attention_dim=128)
TINY_VAE = dict(block_out_channels=(64, 128, 128, 128), layers_per_block=1)
MAX_NORM = 0.05
TIMESTEPS = [[981, 17], [500, 3], [250, 760], [42, 999], [640, 128], [7, 333], [875, 90], [410, 555]]


@pytest.fixture
def fresh_accelerate():
    AL.reset_accelerate_state()
    yield
    AL.reset_accelerate_state()


@pytest.fixture(scope="module")
def unet_batches(cuda):
    """micro-batch 0 is test_tiny_unet_train_step's (synth_inputs, t = [981, 17], target seeded with 11); the others differ in every input"""
    from diffute_amd.synthetic import synth_inputs
    out = []
    for i, ts in enumerate(TIMESTEPS):
        lat, mask, mlat, ctx = synth_inputs(2, 16, 16, 77, 128, seed=100 * i, device=cuda)
        target = torch.randn(2, 4, 16, 16, generator=torch.Generator().manual_seed(11 + i)).to(cuda)
        out.append(((torch.cat([lat, mask, mlat], 1), torch.tensor(ts, device=cuda), ctx), target))
    return out


@pytest.fixture(scope="module")
def vae_batches(cuda):
    g = torch.Generator().manual_seed(21)
    return [(((torch.rand(2, 3, 64, 64, generator=g) * 2 - 1).cuda(),), (torch.rand(2, 3, 64, 64, generator=g) * 2 - 1).cuda()) for _ in range(4)]


def _mean_oracle(runs):
    """(loss, pred, grads) of each micro-batch of the window -> loss and gradients of 0.5 (loss_1 + loss_2)"""
    return sum(r[0] for r in runs) / len(runs), {k: sum(r[2][k] for r in runs) / len(runs) for k in runs[0][2]}


@pytest.fixture(scope="module")
def unet_oracle(cuda, unet_batches):
    """fp32 autograd over oracle.unet at the seeded initial weights on the first window: computed once, shared by the no and bf16 legs"""
    import diffute_amd as D
    from oracle import unet as OU
    sd = D.UNet2DConditionModel(**TINY_UNET).state_dict()
    return _mean_oracle([oracle_unet_train_grads(sd, OU.TINY_UNET, *inp, tgt) for inp, tgt in unet_batches[:AL.ACCUM]])


@pytest.fixture(scope="module")
def vae_oracle(cuda, vae_batches):
    import diffute_amd as D
    from oracle import pipeline as OP, vae as OV
    P = {k: v.detach().cpu() for k, v in D.AutoencoderKL(**TINY_VAE).state_dict().items()}
    return _mean_oracle([OP.vae_train_grads(P, OV.TINY_VAE, x.cpu(), tgt.cpu(), emulate_bf16=False) for (x,), tgt in vae_batches[:AL.ACCUM]])


def _assert_state_dicts_equal(a, b):
    sa, sb = a.state_dict(), b.state_dict()
    assert list(sa) == list(sb)
    for k in sa:
        assert torch.equal(sa[k], sb[k]), f"{k} differs between the two freshly constructed models"


def _run_leg(make, predict, batches, mp, name, oracle=None, bars=None, not_ranked=lambda k: False):
    import diffute_amd as D
    fp16 = mp == "fp16"
    model, twin_model = make(), make()
    _assert_state_dicts_equal(model, twin_model)
    acc = AL.accelerate_loop(model, predict, batches, mp, MAX_NORM, until_stepped=fp16)
    twin = AL.twin_loop(twin_model, predict, batches, mp, MAX_NORM, until_stepped=fp16)
    D.synchronize()
    # (a)
    AL.assert_same_run(acc, twin)
    # (e)
    AL.assert_step_accounting(acc)
    if fp16:
        assert acc.steps == 1 and not acc.skipped[-1], f"{name}: every one of {len(acc.skipped)} optimizer steps was skipped - the leg proves nothing"
    else:
        assert acc.sync == [False, True, False, True] and acc.steps == 2 and not any(acc.skipped)
    s = len(acc.skipped) - 1 if fp16 else 0                       # the optimizer step whose gradient is judged: the first one taken
    pre = twin.preclip[s]                                         # (unscaled, before the clip; without a loss scale it IS the .grad the accelerate run held)
    if not fp16:
        assert AL.first_diff(pre, acc.grads[AL.ACCUM * s + AL.ACCUM - 1]) is None
    # (c)
    norm64 = float(torch.cat([g.double().reshape(-1) for g in pre.values()]).norm())
    got = float(acc.norm[s])
    print(f"{name}: pre-clip gradient norm {got:.6f} (fp64 norm of the gradients {norm64:.6f}), max_norm {MAX_NORM}, steps skipped {sum(acc.skipped)}")
    assert got > MAX_NORM, f"{name}: the gradient norm {got} is below max_norm = {MAX_NORM}: the clip does nothing"
    assert abs(got - norm64) <= 1e-5 * norm64, f"{name}: clip_grad_norm_ returned {got}, the gradients' fp64 norm is {norm64}"
    # (b)
    if oracle is not None:
        ref_loss, ref_g = oracle
        loss = sum(float(l) for l in acc.loss[:AL.ACCUM]) / AL.ACCUM
        tot, errs = grad_errors(pre, ref_g, not_ranked)
        print(f"{name}: accumulated gradient vs the fp32 oracle: loss {loss:.6f} (oracle {ref_loss:.6f}); whole-gradient rel-L2 {tot:.2e}; "
              f"median {errs[len(errs) // 2][0]:.2e}; worst: " + ", ".join(f"{k} {e:.2e}" for e, k in errs[:3]))
        assert abs(loss - ref_loss) <= 2e-2 * abs(ref_loss), f"{name}: loss {loss} vs oracle {ref_loss}"
        assert tot <= bars[0], f"{name}: whole-gradient rel-L2 {tot:.3e}"
        assert errs[0][0] <= bars[1], f"{name}: gradient of {errs[0][1]}: rel-L2 {errs[0][0]:.3e}"
    # (d)
    fresh = make()
    fresh.load_state_dict(acc.model.state_dict())
    inputs = batches[0][0]
    with torch.no_grad():
        out_trained = predict(acc.model, *inputs)
        out_fresh = predict(fresh, *inputs)
    D.synchronize()
    assert torch.isfinite(out_trained).all()
    assert out_trained.dtype == out_fresh.dtype and torch.equal(out_trained, out_fresh), \
        f"{name}: the trained model's forward differs from a new model loaded with its state_dict (max abs {float((out_trained.float() - out_fresh.float()).abs().max()):.3e}): stale packed weights"
    moved = max(float((acc.params[-1][k] - p0).abs().max()) for k, p0 in make().state_dict().items())
    assert moved > 0, f"{name}: no parameter moved"


_unet_predict = lambda m, x, t, ctx: m(x, t, ctx).sample                       # noqa: E731  train_diffute_v1.py:913
_vae_predict = lambda m, x: m(x)["sample"]                                     # noqa: E731  train_vae.py:721-722


@pytest.mark.parametrize("mp", ["no", "bf16"])
def test_unet_under_accelerate(cuda, fresh_accelerate, unet_batches, unet_oracle, mp):
    """UNet, mixed_precision no / bf16: (a)-(e) of the module docstring.  Bars of (b) are test_tiny_unet_train_step's: loss within 2 %,
    whole-gradient rel-L2 <= 4e-2, worst parameter <= 1e-1."""
    import diffute_amd as D
    _run_leg(lambda: D.UNet2DConditionModel(**TINY_UNET).cuda(), _unet_predict, unet_batches[:4], mp, f"UNet under accelerate ({mp})",
             oracle=unet_oracle, bars=(4e-2, 1e-1))


def test_unet_under_accelerate_fp16(cuda, fresh_accelerate, unet_batches):
    """UNet, mixed_precision fp16 on the fp16 build (`.to(dtype=torch.float16)`; the Parameters stay fp32): accelerate's GradScaler against the
    twin's torch.amp.GradScaler("cuda") with torch's defaults, until one optimizer step is taken (at most 4): (a), (c), (d), (e)."""
    import diffute_amd as D

    def make():
        m = D.UNet2DConditionModel(**TINY_UNET).cuda().to(dtype=torch.float16)
        assert m.compute_dtype == torch.float16 and all(p.dtype == torch.float32 for p in m.parameters())
        return m
    _run_leg(make, _unet_predict, unet_batches[:8], "fp16", "UNet under accelerate (fp16)")


def test_vae_under_accelerate(cuda, fresh_accelerate, vae_batches, vae_oracle):
    """VAE, mixed_precision no (train_vae.py:716-736, `vae(x)["sample"]`): (a)-(e).  Bars of (b) are test_tiny_vae_train_step's: loss within
    2 %, whole-gradient rel-L2 <= 5e-2, worst parameter <= 1.5e-1 (to_k.bias is exactly 0 in exact arithmetic and is not ranked)."""
    import diffute_amd as D
    _run_leg(lambda: D.AutoencoderKL(**TINY_VAE).cuda(), _vae_predict, vae_batches, "no", "VAE under accelerate (no)",
             oracle=vae_oracle, bars=(5e-2, 1.5e-1), not_ranked=lambda k: k.endswith("to_k.bias"))
