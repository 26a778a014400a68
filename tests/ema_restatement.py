"""Plain-torch restatement of diffusers' EMAModel arithmetic (0.15-era; the reference's `--use_ema` path,
train_diffute_v1.py:642-646,934-935): the decay schedule, one step and copy_to, written out from the published class so
diffute_amd.EMAModel can be checked against it bit for bit."""
import torch


def get_decay(step_no, decay=0.9999, min_decay=0.0, update_after_step=0, use_ema_warmup=False, inv_gamma=1.0, power=2 / 3):
    step = max(0, step_no - update_after_step - 1)
    if step <= 0:
        return 0.0
    if use_ema_warmup:
        cur = 1 - (1 + step / inv_gamma) ** -power
    else:
        cur = (1 + step) / (10 + step)
    cur = min(cur, decay)
    return max(cur, min_decay)


@torch.no_grad()
def step(shadows, params, decay_value):
    """one EMAModel.step with the decay get_decay returned for it"""
    one_minus_decay = 1 - decay_value
    for s_param, param in zip(shadows, params):
        if param.requires_grad:
            s_param.sub_(one_minus_decay * (s_param - param))
        else:
            s_param.copy_(param)


@torch.no_grad()
def copy_to(shadows, params):
    for s_param, param in zip(shadows, params):
        param.data.copy_(s_param.to(param.device).data)
