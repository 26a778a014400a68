"""diffute_amd.EMAModel without a GPU: the decay schedule, the CPU step / copy_to against the restatement of diffusers'
EMAModel (tests/ema_restatement.py), state_dict round trips and refusals, and the save_pretrained directory read back by
EMAModel.from_pretrained and UNet2DConditionModel.from_pretrained (the reference's save / load hooks,
train_diffute_v1.py:664-678)."""
import json
import os

import pytest
import torch

import ema_restatement as R

TINY_UNET = dict(block_out_channels=(64, 128, 256, 256), attention_head_dim=(1, 2, 4, 4), cross_attention_dim=128)
SCHEDULES = [dict(), dict(use_ema_warmup=True), dict(use_ema_warmup=True, inv_gamma=2.0, power=3 / 4), dict(update_after_step=7),
             dict(update_after_step=3, use_ema_warmup=True), dict(decay=0.8), dict(min_decay=0.5), dict(decay=0.9, min_decay=0.85, use_ema_warmup=True)]


@pytest.mark.parametrize("hp", SCHEDULES)
def test_get_decay_matches_restatement(hp):
    from diffute_amd import EMAModel
    ema = EMAModel([torch.zeros(3)], **hp)
    for s in range(0, 51):
        assert ema.get_decay(s) == R.get_decay(s, **hp), f"step {s} {hp}"


def _params(seed):
    g = torch.Generator().manual_seed(seed)
    shapes = [(7,), (3, 5), (1,), (4097,), (2, 3, 3, 3)]
    ps = [torch.nn.Parameter(torch.randn(s, generator=g)) for s in shapes]
    ps[2].requires_grad_(False)
    return ps, g


@pytest.mark.parametrize("hp", [dict(), dict(use_ema_warmup=True, update_after_step=2)])
def test_cpu_step_and_copy_to_bit_equal(hp):
    from diffute_amd import EMAModel
    ps, g = _params(0)
    ema = EMAModel(ps, **hp)
    ref = [p.detach().clone() for p in ps]
    for i in range(1, 21):
        with torch.no_grad():
            for p in ps:
                p.add_(0.01 * torch.randn(p.shape, generator=g))
        ema.step(ps)
        R.step(ref, ps, R.get_decay(i, **hp))
        assert ema.optimization_step == i and ema.cur_decay_value == R.get_decay(i, **hp)
        for a, b in zip(ema.shadow_params, ref):
            assert torch.equal(a, b), f"step {i}"
    tgt = [torch.nn.Parameter(torch.zeros_like(p)) for p in ps]
    tgt_ref = [torch.zeros_like(p) for p in ps]
    ema.copy_to(tgt)
    R.copy_to(ref, tgt_ref)
    assert all(torch.equal(a.detach(), b) for a, b in zip(tgt, tgt_ref))


def test_module_argument_and_kwargs():
    from diffute_amd import EMAModel
    m = torch.nn.Linear(3, 2)
    ema = EMAModel(m)                                # diffusers: a module means its parameters, with the warmup schedule
    assert ema.use_ema_warmup and len(ema.shadow_params) == 2
    ema = EMAModel(m.parameters(), max_value=0.5, min_value=0.25, foreach=True)
    assert ema.decay == 0.5 and ema.min_decay == 0.25
    with pytest.raises(NotImplementedError):
        EMAModel(m.parameters(), offload_ema=True)


def test_store_restore_cpu():
    from diffute_amd import EMAModel
    ps, g = _params(1)
    ema = EMAModel(ps)
    with torch.no_grad():
        for p in ps:
            p.mul_(3.0)
    ema.step(ps); ema.step(ps)
    before = [p.detach().clone() for p in ps]
    ema.store(ps)
    ema.copy_to(ps)
    assert all(torch.equal(p.detach(), s) for p, s in zip(ps, ema.shadow_params))
    ema.restore(ps)
    assert all(torch.equal(p.detach(), b) for p, b in zip(ps, before))
    with pytest.raises(RuntimeError):
        ema.restore(ps)


def test_state_dict_round_trip_and_refusals():
    from diffute_amd import EMAModel
    ps, g = _params(2)
    ema = EMAModel(ps, decay=0.99, min_decay=0.1, update_after_step=3, use_ema_warmup=True, inv_gamma=2.0, power=0.75)
    for _ in range(5):
        ema.step(ps)
    sd = ema.state_dict()
    assert set(sd) == {"decay", "min_decay", "optimization_step", "update_after_step", "use_ema_warmup", "inv_gamma", "power", "shadow_params"}
    other = EMAModel([torch.zeros_like(p) for p in ps])
    other.load_state_dict(sd)
    for k in ("decay", "min_decay", "optimization_step", "update_after_step", "use_ema_warmup", "inv_gamma", "power"):
        assert getattr(other, k) == getattr(ema, k)
    assert all(torch.equal(a, b) for a, b in zip(other.shadow_params, ema.shadow_params))
    assert all(a is not b for a, b in zip(other.shadow_params, ema.shadow_params))
    for bad in (dict(decay=1.5), dict(decay=-0.1), dict(min_decay=1), dict(optimization_step=2.0), dict(update_after_step="3"),
                dict(use_ema_warmup=1), dict(inv_gamma="x"), dict(power=None), dict(shadow_params=(torch.zeros(1),)),
                dict(shadow_params=[torch.zeros(1), 3.0])):
        with pytest.raises(ValueError):
            EMAModel([torch.zeros(1)]).load_state_dict(dict(sd, **bad))


def test_save_pretrained_round_trip_tiny_unet(tmp_path):
    import diffute_amd as D
    from diffute_amd import EMAModel
    src = D.UNet2DConditionModel(**TINY_UNET)
    ema = EMAModel(src.parameters(), decay=0.995, update_after_step=1, model_cls=D.UNet2DConditionModel, model_config=src.config)
    g = torch.Generator().manual_seed(3)
    for _ in range(4):
        with torch.no_grad():
            for p in src.parameters():
                p.add_(0.01 * torch.randn(p.shape, generator=g))
        ema.step(src.parameters())
    d = os.path.join(str(tmp_path), "unet_ema")
    ema.save_pretrained(d)
    cfg = json.load(open(os.path.join(d, "config.json")))
    assert cfg["optimization_step"] == 4 and cfg["decay"] == 0.995 and cfg["_class_name"] == "UNet2DConditionModel"
    model_cfg, unused = D.UNet2DConditionModel.load_config(d, return_unused_kwargs=True)
    assert set(unused) == {"decay", "inv_gamma", "min_decay", "optimization_step", "power", "update_after_step", "use_ema_warmup"}
    assert "decay" not in model_cfg and model_cfg["cross_attention_dim"] == 128
    back = EMAModel.from_pretrained(d, D.UNet2DConditionModel)
    for k in ("decay", "min_decay", "optimization_step", "update_after_step", "use_ema_warmup", "inv_gamma", "power"):
        assert getattr(back, k) == getattr(ema, k), k
    assert len(back.shadow_params) == len(ema.shadow_params)
    assert all(torch.equal(a, b) for a, b in zip(back.shadow_params, ema.shadow_params))
    plain = D.UNet2DConditionModel.from_pretrained(d)
    assert not hasattr(plain.config, "decay")
    for p, s in zip(plain.parameters(), ema.shadow_params):
        assert torch.equal(p.detach(), s)
    # the model re-built from the config has the same structure
    again = D.UNet2DConditionModel.from_config(plain.config)
    assert [k for k, _ in again.named_parameters()] == [k for k, _ in plain.named_parameters()]


def test_to_casts_floating_shadows_only():
    from diffute_amd import EMAModel
    ema = EMAModel([torch.nn.Parameter(torch.randn(4)), torch.arange(3)])
    ema.to(dtype=torch.bfloat16)
    assert ema.shadow_params[0].dtype == torch.bfloat16 and ema.shadow_params[1].dtype == torch.int64
