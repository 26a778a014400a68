"""Classifier-free guidance (denoise(guidance=Guidance(...)): the fused guided scheduler step, dmx_sched_step_guided) on the bench.py
workload: SD2-inpaint UNet at full size, 512 px, bf16, random-init weights, synthetic inputs, DDIM-50 and DPM-Solver++ 2M 20, B = 1 and 4.
Per (scheduler, B) four loops, each one whole denoise pass, warmed and then timed round-robin in one process (a drift of the machine
hits all of them alike), median of --reps:

  guided            denoise(guidance=Guidance(7.5))                    - 2B-row forward + ONE guided step launch
  guided_rescale    denoise(guidance=Guidance(7.5, rescale=0.7))       - the same, the launch also reduces the two deviations per sample
  plain_2B          denoise at batch 2B, no guidance                   - the floor: the same forwards, the plain step
  unfused           the guided loop from existing pieces: the 2B-row forward (captured graph, time-embedding table, as denoise runs it),
                    the combination as torch ops (plus torch.std for the rescale variant, unfused_rescale), schedulers.launch_step,
                    torch.cat of the new latents into the 2B-row input

and the launches of one pass of each: the library's (dmx_profile_begin / dmx_profile_end) and, for the unfused loops, the torch ops per
step on top.  No speed-up is promised; the line says what the run gave.  Prints one JSON line (kept as profiles/guidance_line.json).

  python scripts/bench_guidance.py [--reps 7] [--warmup 2]"""
import argparse
import ctypes
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import diffute_amd as D  # noqa: E402
from diffute_amd import _cabi  # noqa: E402
from diffute_amd.schedulers import launch_step  # noqa: E402
from diffute_amd.synthetic import synth_inputs  # noqa: E402

SCALE, RESCALE = 7.5, 0.7
TORCH_OPS = {False: 4, True: 11}      # per step: sub, mul, add, cat; with the rescale also 2 x std, div, 2 x mul, mul, add


class Unfused:
    """the guided loop without the fused step; fixed-address buffers, a side stream and the captured forward, as pipeline._Run has them"""

    def __init__(self, unet, lat, mask, mlat, ctx, rescale):
        self.unet, self.rescale, self.B = unet, rescale, lat.shape[0]
        self.lat, self.ctx2 = lat, torch.cat([ctx, torch.zeros_like(ctx)], 0)
        self.m2, self.ml2 = torch.cat([mask, mask], 0), torch.cat([mlat, mlat], 0)
        self.x2, self.eps = torch.cat([lat, lat], 0), torch.empty(2 * self.B, *lat.shape[1:], device=lat.device)
        self.x = torch.empty_like(lat)
        self.step_idx = torch.zeros(1, dtype=torch.int32, device=lat.device)
        self.t_cur = torch.empty(1, dtype=torch.int64, device=lat.device)
        self.stream = torch.cuda.Stream(device=lat.device)

    def __call__(self, sch, steps):
        unet, B, dev = self.unet, self.B, self.lat.device
        sch.set_timesteps(steps)
        ts = sch.timesteps.to(device=dev, dtype=torch.int64).contiguous()
        table, rows = unet.temb_table(ts), torch.arange(len(ts), dtype=torch.int32, device=dev)
        vpred = int(sch.config.prediction_type == "v_prediction")
        main = torch.cuda.current_stream(dev)
        self.stream.wait_stream(main)
        with torch.cuda.stream(self.stream):
            hist = [torch.empty_like(self.lat) for _ in range(sch.config.solver_order if sch.kind == _cabi.SCHED_DPMPP else 0)]
            self.x.copy_(self.lat * sch.init_noise_sigma)
            torch.cat([self.x, self.x], 0, out=self.x2)
            unet.set_context(self.ctx2, slot=0)
            for i, rec in enumerate(sch.iter_plan(0.0)):
                self.step_idx.copy_(rows[i:i + 1], non_blocking=True)
                unet.forward_parts([self.x2, self.m2, self.ml2], self.t_cur, out=self.eps, graph=True, slot=0, temb=(table, self.step_idx))
                ec, eu = self.eps[:B], self.eps[B:]
                d = ec - eu
                s = d * SCALE
                g = eu + s
                if self.rescale:
                    k = ec.std(dim=(1, 2, 3), keepdim=True) / g.std(dim=(1, 2, 3), keepdim=True)
                    g = self.rescale * (g * k) + (1 - self.rescale) * g
                launch_step(sch.kind, rec, self.x, g, None, hist[rec.ring_m1] if rec.order >= 2 else None, hist[rec.ring_m2] if rec.order >= 3 else None,
                            hist[rec.ring_w] if hist else None, self.x, vpred, _cabi.current_stream())
                torch.cat([self.x, self.x], 0, out=self.x2)
        main.wait_stream(self.stream)
        return self.x


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    lib = _cabi.lib()
    unet = D.UNet2DConditionModel(device=dev).requires_grad_(False)
    unet._ensure_packed()
    scheds = {"ddim50": (D.DDIMScheduler, 50), "dpmpp2m_20": (D.DPMSolverMultistepScheduler, 20)}
    ok, by_batch = True, {}

    def launches(fn):
        torch.cuda.synchronize(dev)
        lib.dmx_profile_begin()
        fn()
        torch.cuda.synchronize(dev)
        pb = (ctypes.c_double * (4 * 32))()
        _cabi.check(lib.dmx_profile_end(pb, len(pb)), "profile_end")
        return sum(int(pb[4 * k]) for k in range(32))

    for B in (1, 4):
        lat, mask, mlat, ctx = synth_inputs(B, 64, 64, 577, 1024, device=dev)
        dup = lambda t: torch.cat([t, t], 0)
        lat2, mask2, mlat2, ctx2 = dup(lat), dup(mask), dup(mlat), torch.cat([ctx, torch.zeros_like(ctx)], 0)
        unf = {False: Unfused(unet, lat, mask, mlat, ctx, 0.0), True: Unfused(unet, lat, mask, mlat, ctx, RESCALE)}
        cases = {}
        for name, (mk, steps) in scheds.items():
            cases[f"{name}_guided"] = (steps, lambda mk=mk, steps=steps: D.denoise(unet, mk(), lat, mask, mlat, ctx, steps, guidance=D.Guidance(SCALE)))
            cases[f"{name}_guided_rescale"] = (steps, lambda mk=mk, steps=steps: D.denoise(unet, mk(), lat, mask, mlat, ctx, steps,
                                                                                          guidance=D.Guidance(SCALE, RESCALE)))
            cases[f"{name}_plain_2B"] = (steps, lambda mk=mk, steps=steps: D.denoise(unet, mk(), lat2, mask2, mlat2, ctx2, steps))
            cases[f"{name}_unfused"] = (steps, lambda mk=mk, steps=steps: unf[False](mk(), steps))
            cases[f"{name}_unfused_rescale"] = (steps, lambda mk=mk, steps=steps: unf[True](mk(), steps))
        times, first, good = {c: [] for c in cases}, {}, {c: True for c in cases}
        for r in range(args.warmup + args.reps):
            print(f"B = {B}: round {r + 1} of {args.warmup + args.reps}", file=sys.stderr, flush=True)
            for name, (steps, fn) in cases.items():
                torch.cuda.synchronize(dev)
                t0 = time.perf_counter()
                out = fn()
                torch.cuda.synchronize(dev)
                if r >= args.warmup:
                    times[name].append(time.perf_counter() - t0)
                good[name] &= bool(torch.isfinite(out).all())
                if name not in first:
                    first[name] = out.clone()
                else:
                    good[name] &= torch.equal(out, first[name])
        _cabi.poll_device_error()
        runs = {}
        for name, (steps, fn) in cases.items():
            ts = sorted(times[name])
            sname = name.split("_guided")[0].split("_plain")[0].split("_unfused")[0]
            med = lambda c: sorted(times[c])[len(times[c]) // 2] * 1e3
            n = launches(fn)
            extra = TORCH_OPS["rescale" in name] if "unfused" in name else 0
            runs[name] = {"steps": steps, "ms_per_pass": round(med(name), 1), "ms_min": round(ts[0] * 1e3, 1), "ms_max": round(ts[-1] * 1e3, 1),
                          "vs_plain_2B": round(med(name) / med(sname + "_plain_2B"), 4),
                          "vs_unfused": round(med(name) / med(sname + ("_unfused_rescale" if "rescale" in name else "_unfused")), 4),
                          "library_launches_per_pass": n, "library_launches_per_step": round(n / steps, 2), "torch_ops_per_step": extra,
                          "finite_and_bit_equal_across_passes": good[name]}
            ok &= good[name]
        for sname in scheds:      # the fused step computes the unfused loop's arithmetic (rescale 0: the same three roundings, then the same step)
            ok &= torch.equal(first[sname + "_guided"], first[sname + "_unfused"])
            runs[sname + "_guided_rescale"]["rel_l2_from_unfused_rescale"] = float((first[sname + "_guided_rescale"] - first[sname + "_unfused_rescale"]).norm()
                                                                                   / first[sname + "_unfused_rescale"].norm())
            ok &= runs[sname + "_guided"]["library_launches_per_pass"] == runs[sname + "_plain_2B"]["library_launches_per_pass"]
        by_batch[f"b{B}"] = runs

    print(json.dumps({
        "metric": "guided denoise pass wall-clock: fused guided step vs the unfused loop and the plain loop at 2B", "unit": "ms", "ok": bool(ok),
        "reps": args.reps, "warmup": args.warmup, "guidance_scale": SCALE, "rescale": RESCALE,
        "config": "SD2-inpaint UNet, 512 px (latents 64x64), glyph context [B,577,1024] + the zero context, bf16, random-init weights, synthetic inputs",
        "batches": by_batch}))
    if not ok:
        sys.exit(1)


if __name__ == "__main__":
    main()
