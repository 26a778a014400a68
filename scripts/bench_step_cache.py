"""The step cache (denoise(cache_interval=n): DeepCache-style reuse of the deep UNet features) on the bench.py workload: SD2-inpaint
UNet at full size, 512 px, bf16, random-init weights, synthetic inputs, batch 4 and batch 1.  Per batch: DDIM-50 at intervals 1, 2, 3, 5
and DPM-Solver++ 2M 20 at intervals 1, 2, 3 - wall-clock of one whole denoise pass, every configuration (and the plain call without the
argument, the base) warmed and then timed round-robin in one process, so that a drift of the machine hits all of them alike; launches
of a full and of a shallow step (dmx_profile_begin / dmx_profile_end), the time of each as a replayed graph, the shallow step's share
of a forward's FLOPs (diffute_amd.flops) and the rel-L2 of the final latents from interval 1's.  That deviation says how far the cached
algorithm moves the result WITH RANDOM WEIGHTS: it is no statement about image quality, which needs trained weights and is not measured
here.  Prints one JSON line (kept as profiles/step_cache_line.json).

  python scripts/bench_step_cache.py [--reps 5] [--warmup 2]"""
import argparse
import ctypes
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import diffute_amd as D  # noqa: E402
from diffute_amd import _cabi, flops  # noqa: E402
from diffute_amd.synthetic import synth_inputs  # noqa: E402

CLASS_NAMES = {2: "splitk_reduce", 3: "attention", 4: "groupnorm", 5: "layernorm", 6: "other", 26: "xf_chain", 27: "conv_halo", 28: "skinny"}


def rel_l2(a, b):
    return float((a - b).norm() / b.norm())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    lib = _cabi.lib()
    unet = D.UNet2DConditionModel(device=dev).requires_grad_(False)
    unet._ensure_packed()
    side = torch.cuda.Stream(device=dev)
    scheds = {"ddim50": (D.DDIMScheduler, 50, (1, 2, 3, 5)), "dpmpp2m_20": (D.DPMSolverMultistepScheduler, 20, (1, 2, 3))}
    ok, by_batch = True, {}

    for B in (4, 1):
        lat, mask, mlat, ctx = synth_inputs(B, 64, 64, 577, 1024, device=dev)

        # ---- one step: launches (profiled, eager) and time (replayed graph) of a full and of a shallow step; identity at full size
        t = torch.tensor([501], device=dev)
        unet.set_context(ctx)
        buf = unet.step_cache(B, 64, 64)
        plain = unet.forward_parts([lat, mask, mlat], t).clone()

        def profiled(**kw):
            torch.cuda.synchronize(dev)
            lib.dmx_profile_begin()
            out = unet.forward_parts([lat, mask, mlat], t, **kw).clone()
            pb = (ctypes.c_double * (4 * 32))()
            _cabi.check(lib.dmx_profile_end(pb, len(pb)), "profile_end")
            per = {(CLASS_NAMES.get(k) or f"gemm_class_{k}"): {"launches": int(pb[4 * k]), "ms": round(pb[4 * k + 1], 4)} for k in range(32) if pb[4 * k]}
            return out, sum(v["launches"] for v in per.values()), per

        o_full, n_full, _ = profiled()
        o_fill, n_fill, _ = profiled(step_cache=(buf, "fill"))
        o_use, n_use, per_use = profiled(step_cache=(buf, "use"))
        identity = torch.equal(o_full, plain) and torch.equal(o_fill, plain) and torch.equal(o_use, plain)
        ok &= identity

        def step_ms(n=30, **kw):
            out = torch.empty_like(plain)
            side.wait_stream(torch.cuda.current_stream(dev))
            with torch.cuda.stream(side):
                for _ in range(4):                     # eager, capture, replays
                    unet.forward_parts([lat, mask, mlat], t, out=out, graph=True, **kw)
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(side)
                for _ in range(n):
                    unet.forward_parts([lat, mask, mlat], t, out=out, graph=True, **kw)
                e1.record(side)
            side.synchronize()
            return e0.elapsed_time(e1) / n
        step = {"full_ms": None, "fill_ms": None, "shallow_ms": None}
        for _ in range(2):                             # (two interleaved rounds: the second is kept, the first warms every graph)
            step["full_ms"] = round(step_ms(), 3)
            step["fill_ms"] = round(step_ms(step_cache=(buf, "fill")), 3)
            step["shallow_ms"] = round(step_ms(step_cache=(buf, "use")), 3)
        f_full = flops.unet_flops(unet.config, B, 64, 64, 577, cached_ctx_kv=True, phase_upsample=True)
        f_sh = flops.unet_flops(unet.config, B, 64, 64, 577, cached_ctx_kv=True, phase_upsample=True, shallow=True)

        # ---- whole passes, round-robin
        cases = [(f"{name}_base", mk, steps, None) for name, (mk, steps, _) in scheds.items()]
        cases += [(f"{name}_interval{n}", mk, steps, n) for name, (mk, steps, ivs) in scheds.items() for n in ivs]
        times, first, finite, equal = {c[0]: [] for c in cases}, {}, {c[0]: True for c in cases}, {c[0]: True for c in cases}
        for r in range(args.warmup + args.reps):
            for name, mk, steps, n in cases:
                kw = {} if n is None else {"cache_interval": n}
                torch.cuda.synchronize(dev)
                t0 = time.perf_counter()
                out = D.denoise(unet, mk(), lat, mask, mlat, ctx, steps, **kw)
                torch.cuda.synchronize(dev)
                if r >= args.warmup:
                    times[name].append(time.perf_counter() - t0)
                finite[name] &= bool(torch.isfinite(out).all())
                if name not in first:
                    first[name] = out.clone()
                else:
                    equal[name] &= torch.equal(out, first[name])
        _cabi.poll_device_error()
        runs = {}
        for name, mk, steps, n in cases:
            ts = sorted(times[name])
            sname = name.rsplit("_", 1)[0]
            ms = ts[len(ts) // 2] * 1e3
            n_sh = 0 if n in (None, 1) else steps - (steps + n - 1) // n
            runs[name] = {"unet_calls": steps, "shallow_steps": n_sh, "ms_per_pass": round(ms, 1), "ms_min": round(ts[0] * 1e3, 1), "ms_max": round(ts[-1] * 1e3, 1),
                          "vs_interval1": round(ms / (sorted(times[sname + "_interval1"])[len(ts) // 2] * 1e3), 3),
                          "rel_l2_from_interval1_random_weights_no_quality_meaning": rel_l2(first[name], first[sname + "_interval1"]),
                          "finite": finite[name], "bit_equal_across_passes": equal[name]}
            ok &= finite[name] and equal[name]
        for sname in scheds:
            ok &= torch.equal(first[sname + "_base"], first[sname + "_interval1"])      # cache_interval=1 IS the plain loop
        by_batch[f"b{B}"] = {
            "launches_full_step": n_full, "launches_fill_step": n_fill, "launches_shallow_step": n_use,
            "launch_ratio_shallow_to_full": round(n_use / n_full, 3),
            "shallow_flop_share": round(f_sh / f_full, 4), "step_graph_replay": step,
            "shallow_to_full_step_time": round(step["shallow_ms"] / step["full_ms"], 3),
            "shallow_step_by_class_profiled": per_use, "fill_then_use_bit_equal_to_full": identity, "runs": runs}

    print(json.dumps({
        "metric": "denoise pass wall-clock with the step cache (cache_interval)", "unit": "ms", "ok": bool(ok), "reps": args.reps, "warmup": args.warmup,
        "config": "SD2-inpaint UNet, 512 px (latents 64x64), glyph context [B,577,1024], bf16, random-init weights, synthetic inputs",
        "quality": "not measured here: rel_l2_from_interval1 is taken with random weights and says nothing about image quality",
        "batches": by_batch}))
    if not ok:
        sys.exit(1)


if __name__ == "__main__":
    main()
