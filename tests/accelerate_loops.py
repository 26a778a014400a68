"""The reference's optimisation loop (train_diffute_v1.py:873-930, train_vae.py:716-736), twice: `accelerate_loop` runs it through
accelerate exactly as it is written there, `twin_loop` is the plain restatement - what accelerate's wrappers do, done by hand.  Both record
every micro-step, `assert_same_run` compares two records bit for bit and names the first tensor that differs.

tests/test_accelerate_host.py pins the restatement on the CPU (a small nn.Module, no GPU), tests/test_accelerate_gpu.py runs the same two
functions on the HIP models: there a difference between the two is a defect in the glue between torch / accelerate and the HIP training graph.

`predict(model, *inputs)` is the forward as the reference writes it (`unet(x, t, ctx).sample`, `vae(x)["sample"]`); a batch is
`(inputs, target)`.  The loops start no process."""
import math
from types import SimpleNamespace

import torch
import torch.nn.functional as F

ACCUM = 2                 # --gradient_accumulation_steps
LR, WEIGHT_DECAY, WARMUP = 1e-4, 1e-2, 4


def warmup(step):
    """constant-with-warm-up multiplier of the learning rate after `step` scheduler steps"""
    return min(1.0, (step + 1) / WARMUP)


def make_optimizer(model):
    opt = torch.optim.AdamW(model.parameters(), lr=LR, weight_decay=WEIGHT_DECAY)
    return opt, torch.optim.lr_scheduler.LambdaLR(opt, warmup)


def reset_accelerate_state():
    """drop accelerate's process-wide singletons (and with them the device they chose): no test inherits an Accelerator"""
    from accelerate.state import AcceleratorState, GradientState
    AcceleratorState._reset_state(True)
    GradientState._reset_state()


def steps_taken(opt):
    """AdamW's own count of the updates it applied (0 before the first)"""
    for st in opt.state.values():
        return int(st["step"])
    return 0


def _grads(model):
    return {k: None if p.grad is None else p.grad.detach().clone() for k, p in model.named_parameters()}


def _params(model):
    return {k: p.detach().clone() for k, p in model.named_parameters()}


def _record():
    # per micro-step: loss, sync, grads (after the backward); per boundary: preclip (twin only: unscaled, before the clip), norm, skipped,
    # lr (after the scheduler), params (after the step)
    return SimpleNamespace(loss=[], sync=[], grads=[], preclip=[], norm=[], skipped=[], lr=[], params=[], steps=0, optimizer=None, model=None)


def accelerate_loop(model, predict, batches, mp, max_norm, cpu=False, until_stepped=False):
    """the reference loop, literally; `until_stepped` ends it after the first optimizer step that was not skipped (fp16: the loss scale
    starts at 2^16 and may have to back off first)"""
    from accelerate import Accelerator
    accelerator = Accelerator(gradient_accumulation_steps=ACCUM, mixed_precision=mp, cpu=cpu)
    opt, sched = make_optimizer(model)
    unet, optimizer, lr_scheduler = accelerator.prepare(model, opt, sched)
    rec = _record()
    for inputs, target in batches:
        with accelerator.accumulate(unet):
            loss = F.mse_loss(predict(unet, *inputs).float(), target.float())
            accelerator.backward(loss)
            rec.loss.append(loss.detach().clone()); rec.sync.append(bool(accelerator.sync_gradients)); rec.grads.append(_grads(unet))
            if accelerator.sync_gradients:
                rec.norm.append(accelerator.clip_grad_norm_(unet.parameters(), max_norm).detach().clone())
            optimizer.step()
            lr_scheduler.step()
            optimizer.zero_grad()
        if accelerator.sync_gradients:
            rec.skipped.append(bool(accelerator.optimizer_step_was_skipped))
            rec.lr.append(optimizer.param_groups[0]["lr"]); rec.params.append(_params(unet))
            if until_stepped and not rec.skipped[-1]:
                break
    rec.steps = steps_taken(opt); rec.optimizer = optimizer; rec.model = unet
    return rec


def twin_loop(model, predict, batches, mp, max_norm, device_type="cuda", autocast=False, until_stepped=False):
    """the same loop without accelerate: `(loss / ACCUM).backward()` per micro-step; at the boundary clip, step, schedule, zero.  fp16 goes
    through torch.amp.GradScaler with torch's defaults (scale, backward; at the boundary unscale_, clip, scaler.step, scaler.update), and a
    skipped step does not advance the schedule (accelerate's AcceleratedScheduler).  `autocast=True` runs the forward under torch.autocast as
    accelerate's prepared forward does: that decides the precision of a torch module; a HIP model computes in its own build's precision, so
    its twin runs with autocast=False and any effect of autocast on it shows as a difference."""
    opt, sched = make_optimizer(model)
    scaler = torch.amp.GradScaler(device_type) if mp == "fp16" else None
    amp_dtype = {"bf16": torch.bfloat16, "fp16": torch.float16}.get(mp)
    rec = _record()
    for i, (inputs, target) in enumerate(batches):
        boundary = (i + 1) % ACCUM == 0
        with torch.autocast(device_type=device_type, dtype=amp_dtype, enabled=autocast and amp_dtype is not None):
            pred = predict(model, *inputs)
        loss = F.mse_loss(pred.float(), target.float())
        (scaler.scale(loss / ACCUM) if scaler is not None else loss / ACCUM).backward()
        rec.loss.append(loss.detach().clone()); rec.sync.append(boundary); rec.grads.append(_grads(model))
        if not boundary:
            continue
        if scaler is not None:
            scaler.unscale_(opt)
        rec.preclip.append(_grads(model))
        rec.norm.append(torch.nn.utils.clip_grad_norm_(model.parameters(), max_norm).detach().clone())
        before = steps_taken(opt)
        if scaler is not None:
            scaler.step(opt); scaler.update()
        else:
            opt.step()
        rec.skipped.append(steps_taken(opt) == before)
        if not rec.skipped[-1]:
            sched.step()
        opt.zero_grad()
        rec.lr.append(opt.param_groups[0]["lr"]); rec.params.append(_params(model))
        if until_stepped and not rec.skipped[-1]:
            break
    rec.steps = steps_taken(opt); rec.optimizer = opt; rec.model = model
    return rec


def bit_equal(a, b):
    """same dtype, shape and bits (NaN payloads included: a skipped fp16 step holds non-finite gradients on both sides)"""
    if a is None or b is None:
        return a is b
    if a.dtype != b.dtype or a.shape != b.shape:
        return False
    it = {4: torch.int32, 2: torch.int16, 8: torch.int64}[a.element_size()]
    return torch.equal(a.contiguous().view(it), b.contiguous().view(it))


def first_diff(da, db):
    assert list(da) == list(db), "the two models name their parameters differently"
    for k in da:
        if not bit_equal(da[k], db[k]):
            return k
    return None


def assert_same_run(acc, twin):
    """assertion (a): losses and every .grad after every micro-step, every parameter after every optimizer step, and the bookkeeping"""
    assert acc.sync == twin.sync, f"sync_gradients sequence {acc.sync} vs the twin's boundaries {twin.sync}"
    assert len(acc.loss) == len(twin.loss) and acc.skipped == twin.skipped, f"skipped steps {acc.skipped} vs {twin.skipped}"
    for i, (la, lb) in enumerate(zip(acc.loss, twin.loss)):
        assert bit_equal(la, lb), f"micro-step {i}: loss {float(la)!r} (accelerate) vs {float(lb)!r} (twin)"
        k = first_diff(acc.grads[i], twin.grads[i])
        assert k is None, f"micro-step {i}: .grad of {k} differs between the accelerate run and the twin"
    for s, (pa, pb) in enumerate(zip(acc.params, twin.params)):
        assert bit_equal(acc.norm[s], twin.norm[s]), f"optimizer step {s}: clip norm {float(acc.norm[s])!r} vs {float(twin.norm[s])!r}"
        k = first_diff(pa, pb)
        assert k is None, f"optimizer step {s}: parameter {k} differs between the accelerate run and the twin"
        assert acc.lr[s] == twin.lr[s], f"optimizer step {s}: learning rate {acc.lr[s]} vs {twin.lr[s]}"
    assert acc.steps == twin.steps


def assert_step_accounting(rec):
    """assertion (e): boundaries on every ACCUM-th micro-step, AdamW counted the steps that were not skipped, the rate follows the warm-up"""
    assert rec.sync == [(i + 1) % ACCUM == 0 for i in range(len(rec.sync))], rec.sync
    done = 0
    for s, skipped in enumerate(rec.skipped):
        done += 0 if skipped else 1
        assert math.isclose(rec.lr[s], LR * warmup(done), rel_tol=1e-12), f"optimizer step {s}: lr {rec.lr[s]} after {done} scheduler steps"
    assert rec.steps == done == steps_taken(rec.optimizer), f"AdamW counted {rec.steps} steps, {done} were taken"
