"""Sampler comparison on the bench.py workload (BASELINE configs[1]: SD2-inpaint UNet, 512 px, batch 4, bf16, synthetic inputs,
random-init weights): wall-clock of one whole denoise pass with DDIM-50 (the headline), DPM-Solver++ 2M at 20 and 25 steps, and at
the reference's batch-1 operating point DPM-Solver++ 2M at 20 / 25 steps against DDPM-150 (app.ipynb:545,806-816).  All in one
process on one model; every timed pass is checked finite and bit-equal to the first pass of its configuration.  Prints one JSON line.

  python scripts/bench_solvers.py [--reps 5] [--warmup 2]"""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import diffute_amd as D  # noqa: E402
from diffute_amd import _cabi  # noqa: E402
from diffute_amd.synthetic import synth_inputs  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    unet = D.UNet2DConditionModel(device=dev).requires_grad_(False)
    unet._ensure_packed()

    def timed(name, make_sched, B, steps, variance_noise=None):
        lat, mask, mlat, ctx = synth_inputs(B, 64, 64, 577, 1024, device=dev)
        first, ts, finite, equal = None, [], True, True
        for r in range(args.warmup + args.reps):
            torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
            out = D.denoise(unet, make_sched(), lat, mask, mlat, ctx, steps, variance_noise=variance_noise)
            torch.cuda.synchronize(dev)
            if r >= args.warmup:
                ts.append(time.perf_counter() - t0)
            finite &= bool(torch.isfinite(out).all())
            if first is None:
                first = out.clone()
            else:
                equal &= torch.equal(out, first)
        _cabi.poll_device_error()
        ms = sorted(ts)[len(ts) // 2] * 1e3
        return name, {"batch": B, "unet_calls": steps, "ms_per_pass": round(ms, 1), "ms_per_unet_call": round(ms / steps, 3),
                      "images_per_s": round(B * 1e3 / ms, 3), "finite": finite, "bit_equal_across_passes": equal}

    dpm2m = D.DPMSolverMultistepScheduler
    res = dict([
        timed("b4_ddim50", D.DDIMScheduler, 4, 50),
        timed("b4_dpmpp2m_20", dpm2m, 4, 20),
        timed("b4_dpmpp2m_25", dpm2m, 4, 25),
        timed("b1_ddpm150", D.DDPMScheduler, 1, 150, variance_noise=torch.randn(150, 1, 4, 64, 64, device=dev,
                                                                                  generator=torch.Generator(dev).manual_seed(0))),
        timed("b1_dpmpp2m_20", dpm2m, 1, 20),
        timed("b1_dpmpp2m_25", dpm2m, 1, 25),
    ])
    ok = all(v["finite"] and v["bit_equal_across_passes"] for v in res.values())
    print(json.dumps({
        "metric": "denoise pass wall-clock by sampler", "unit": "ms", "ok": ok, "reps": args.reps, "warmup": args.warmup,
        "config": "SD2-inpaint UNet, 512 px (latents 64x64), glyph context [B,577,1024], bf16, random-init weights, synthetic inputs",
        "speedup_b4_dpmpp2m_20_vs_ddim50": round(res["b4_ddim50"]["ms_per_pass"] / res["b4_dpmpp2m_20"]["ms_per_pass"], 3),
        "speedup_b4_dpmpp2m_25_vs_ddim50": round(res["b4_ddim50"]["ms_per_pass"] / res["b4_dpmpp2m_25"]["ms_per_pass"], 3),
        "speedup_b1_dpmpp2m_20_vs_ddpm150": round(res["b1_ddpm150"]["ms_per_pass"] / res["b1_dpmpp2m_20"]["ms_per_pass"], 3),
        "speedup_b1_dpmpp2m_25_vs_ddpm150": round(res["b1_ddpm150"]["ms_per_pass"] / res["b1_dpmpp2m_25"]["ms_per_pass"], 3),
        "runs": res}))
    if not ok:
        sys.exit(1)


if __name__ == "__main__":
    main()
