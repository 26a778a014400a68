"""The training walks on the GPU, per parameter: one forward / mse_loss / backward through the product classes for every case of
train_walk_refs.py on both builds, every parameter gradient against torch autograd over the fp32 oracle at the bound its
recorded restatement floor gives (3 x max(own floor, median floor); whole gradient 1.5 x; loss 2 %), and the step repeated
bit for bit.  test_train_walk_host.py pins the floors, the set of parameters judged absolutely and what the bounds catch.
`pytest -rA` shows one line per check: `key whole e/b worst <name> e/b`."""
import pytest
import torch

import train_walk_refs as R

pytestmark = pytest.mark.gpu
TINY_UNET = dict(block_out_channels=(64, 128, 256, 256), attention_head_dim=(1, 2, 4, 4), cross_attention_dim=128)
TINY_VAE = dict(block_out_channels=(64, 128, 128, 128), layers_per_block=1)
KEYS = [(m, c, e) for m, c in R.GPU_KEYS for e in R.ELEMS]
_models, _refs = {}, {}


def _model(model, elem):
    """one model per (class, build) for the module; every step writes (never accumulates) its gradients after zero_grad"""
    if (model, elem) not in _models:
        import diffute_amd as D
        m = (D.UNet2DConditionModel(**TINY_UNET) if model == "unet" else D.AutoencoderKL(**TINY_VAE)).cuda()
        if elem == "fp16":
            m = m.to(dtype=torch.float16)
        assert m.compute_dtype == R.ELEMS[elem]
        _models[(model, elem)] = m
    return _models[(model, elem)]


def _reference(model, case, m):
    """the CPU oracle's reference of a case, once per module (fp32 master parameters: the same on both builds)"""
    if (model, case) not in _refs:
        P = {k: v.detach().float().cpu() for k, v in m.state_dict().items()}
        loss, g = R.reference(model, case, P)
        _refs[(model, case)] = (P, loss, g, R.absolute_set(g))
    P, loss, g, ab = _refs[(model, case)]
    assert all(torch.equal(P[k], v.detach().float().cpu()) for k, v in m.state_dict().items()), "the models of the two builds differ"
    return loss, g, ab


def _step(model, case, elem, m, cuda):
    import diffute_amd as D
    from diffute_amd.models import mse_loss
    S = R.LOSS_SCALE[elem]
    m.zero_grad(set_to_none=True)
    if model == "unet":
        x, t, ctx, target = R.unet_inputs(case)
        if R.UNET_CASES[case]["ctx16"]:
            ctx = ctx.to(R.ELEMS[elem])
        pred = m(x.to(cuda), t.to(cuda), ctx.to(cuda)).sample
    else:
        x, target = R.vae_inputs(case)
        pred = m(x.to(cuda))["sample"]
    loss = mse_loss(pred, target.to(cuda))
    if elem == "fp16":
        D.GradScaler(init_scale=S).scale(loss).backward()
    else:
        loss.backward()
    grads = {}
    for k, p in m.named_parameters():
        assert p.grad is not None and p.grad.dtype == torch.float32, f"no fp32 gradient for {k}"
        grads[k] = p.grad.detach().clone()
    return float(loss.detach()), grads


@pytest.mark.parametrize("model,case,elem", KEYS, ids=[f"{m}/{c}/{e}" for m, c, e in KEYS])
def test_train_walk_per_parameter(cuda, model, case, elem):
    key = f"{model}/{case}/{elem}"
    m = _model(model, elem)
    ref_loss, ref, ab = _reference(model, case, m)
    loss, g1 = _step(model, case, elem, m, cuda)
    loss2, g2 = _step(model, case, elem, m, cuda)
    assert set(g1) == set(ref)
    S = R.LOSS_SCALE[elem]
    R.check(key, {k: v.cpu() / S for k, v in g1.items()}, ref, loss, ref_loss, ab)
    assert loss2 == loss, f"{key}: the loss of the repeated step differs: {loss2} vs {loss}"
    diff = [k for k in g1 if not torch.equal(g1[k], g2[k])]
    assert not diff, f"{key}: {len(diff)} gradients differ between two identical steps, first {diff[0]}"


@pytest.mark.parametrize("elem", list(R.ELEMS))
def test_vae_training_refuses_sides_off_64(cuda, elem):
    """the AutoencoderKL training graph takes image sides that are multiples of 64; anything else (here train_walk_refs' host-only
    32x48 case) must be refused with that message before a kernel runs - never differentiated by another route"""
    m = _model("vae", elem)
    x, _ = R.vae_inputs("wide_b3")
    assert not R.VAE_CASES["wide_b3"]["admitted"]
    with pytest.raises(ValueError, match="multiples of 64"):
        m(x.to(cuda))
