"""EMAModel.step / copy_to at full size (686 tensors, 865.9 M fp32 parameters, the reference's `--use_ema` UNet):

    python scripts/bench_ema.py [--iters N] [--warmup W]

Prints one JSON line: ms per call and achieved TB/s (bytes the call must move: 12 B per element for a step - read shadow
and parameter, write shadow -, 8 B for a copy) for
  step_generic   EMAModel.step(unet.parameters()) with no fused optimizer (one dmx_ema_step_multi over the Parameters)
  step_fused     the same after a FusedAdamW.step(): one dmx_ema_step_multi over the packed master arena
  torch_loop     diffusers' per-tensor loop `s.sub_(omd * (s - p))` (3 launches per tensor)
  torch_foreach  torch._foreach_sub_(s, torch._foreach_sub(s, p), alpha=omd) (later diffusers' foreach=True)
  copy_to        EMAModel.copy_to into 686 plain fp32 tensors (one dmx_copy_multi)"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402


def timed(fn, iters, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()
    import diffute_amd as D
    from diffute_amd import EMAModel
    from diffute_amd.models import mse_loss
    from diffute_amd.synthetic import synth_inputs
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    unet = D.UNet2DConditionModel(device=dev)
    params = list(unet.parameters())
    n = sum(p.numel() for p in params)
    res = dict(tensors=len(params), elements=n)

    def rate(ms, nbytes):
        return dict(ms=round(ms, 4), tb_s=round(nbytes / (ms * 1e-3) / 1e12, 3))

    ema = EMAModel(params, decay=0.9999)
    res["step_generic"] = rate(timed(lambda: ema.step(params), args.iters, args.warmup), 12 * n)
    shadows = [p.detach().clone() for p in params]
    omd = 1 - 0.9999

    def loop():
        for s, p in zip(shadows, params):
            s.sub_(omd * (s - p))
    with torch.no_grad():
        res["torch_loop"] = rate(timed(loop, max(3, args.iters // 4), 1), 12 * n)
        res["torch_foreach"] = rate(timed(lambda: torch._foreach_sub_(shadows, torch._foreach_sub(shadows, params), alpha=omd),
                                          max(3, args.iters // 4), 1), 12 * n)
    tgt = [torch.empty_like(p.detach()) for p in params]
    res["copy_to"] = rate(timed(lambda: ema.copy_to(tgt), args.iters, args.warmup), 8 * n)
    del shadows, tgt
    # fused: one training step at a small latent size puts the weights into FusedAdamW's master arena
    opt = D.FusedAdamW(unet, lr=1e-5)
    lat, mask, mlat, ctx = synth_inputs(1, 8, 8, 77, 1024, device=dev)
    x = torch.cat([lat, mask, mlat], 1)
    mse_loss(unet(x, torch.tensor([500], device=dev), ctx).sample, torch.zeros_like(lat)).backward()
    opt.step()
    ema_f = EMAModel(params, decay=0.9999)
    ema_f.step(params)
    assert ema_f._arena is not None and opt.dirty, "the fused path was not taken"
    span = ema_f._arena["table"].elements
    res["step_fused"] = rate(timed(lambda: ema_f.step(params), args.iters, args.warmup), 12 * span)
    res["step_fused"]["elements"] = span
    res["speedup_vs_torch_loop"] = round(res["torch_loop"]["ms"] / max(res["step_generic"]["ms"], res["step_fused"]["ms"]), 2)
    D.synchronize()
    print(json.dumps(dict(bench="ema", **res)))


if __name__ == "__main__":
    main()
