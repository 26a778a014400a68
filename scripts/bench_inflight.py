"""In-flight batching (diffute_amd.DenoiseEngine) against what denoise() offers requests that do not line up, same process, same requests:

    python scripts/bench_inflight.py [--requests N] [--iters N] [--warmup W] [--out FILE]

Full-size UNet with random weights, 512 px (64 x 64 latents, 577 context tokens), DDIM.  N = 16 single-row requests, all queued at the start,
their step counts drawn with a fixed seed from {20, 30, 50}.  Prints one JSON line (and writes it to --out, default
profiles/inflight_line.json); total ms per pass over all requests (wall clock, synchronised) and requests/s of three arms:
  engine    DenoiseEngine(capacity=4): submit all, run_until_idle (the engine lives across passes, as in a service)
  single    one batch-1 denoise() per request
  grouped   the best available without the engine: requests grouped by equal step count into denoise() batches of up to 4
and, in the same run, the engine's ms per tick beside denoise()'s ms per step at B = 4.  The engine's latents of request 0 are compared with the
batch-1 chain's (relative L2; the two run different batch sizes, hence other tile plans - no threshold is applied)."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from bench_edit import timed  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--requests", type=int, default=16)
    ap.add_argument("--capacity", type=int, default=4)
    ap.add_argument("--iters", type=int, default=2)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "inflight_line.json"))
    args = ap.parse_args()
    import diffute_amd as D
    from diffute_amd.synthetic import synth_inputs
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    N, cap = args.requests, args.capacity
    steps = [int(s) for s in np.random.RandomState(args.seed).choice([20, 30, 50], size=N)]
    unet = D.UNet2DConditionModel(device=dev).requires_grad_(False)
    reqs = [synth_inputs(1, 64, 64, 577, 1024, seed=10 * i, device=dev) for i in range(N)]
    res = dict(bench="inflight", requests=N, capacity=cap, steps=steps, total_steps=sum(steps), iters=args.iters, scheduler="ddim")
    kept = {}

    eng = D.DenoiseEngine(unet, D.DDIMScheduler(), capacity=cap, latent_shape=(4, 64, 64), ctx_len=577)

    def engine():
        t0 = eng.planner.ticks
        tk = [eng.submit(*reqs[i], steps[i]) for i in range(N)]
        eng.run_until_idle()
        kept["ticks"] = eng.planner.ticks - t0
        kept["engine0"] = eng.result(tk[0])
        for t in tk[1:]:
            eng.result(t)

    def single():
        for i in range(N):
            out = D.denoise(unet, D.DDIMScheduler(), *reqs[i], steps[i])
            if i == 0:
                kept["single0"] = out

    groups = []
    for T in sorted(set(steps)):
        ids = [i for i in range(N) if steps[i] == T]
        groups += [(T, ids[k:k + cap]) for k in range(0, len(ids), cap)]
    batches = [(T, [torch.cat([reqs[i][j] for i in ids], 0) for j in range(4)]) for T, ids in groups]

    def grouped():
        for T, b in batches:
            D.denoise(unet, D.DDIMScheduler(), *b, T)

    b4 = [torch.cat([reqs[i][j] for i in range(cap)], 0) for j in range(4)]

    def denoise_b4():
        D.denoise(unet, D.DDIMScheduler(), *b4, 50)

    for name, fn in (("engine", engine), ("single", single), ("grouped", grouped)):
        ms = timed(fn, args.iters, args.warmup)
        res[f"{name}_ms"] = round(ms, 2)
        res[f"{name}_requests_per_s"] = round(N / ms * 1e3, 3)
    res["grouped_batches"] = [[T, len(ids)] for T, ids in groups]
    res["engine_ticks"] = kept["ticks"]
    res["engine_rows_busy"] = round(sum(steps) / (cap * kept["ticks"]), 4)
    res["engine_ms_per_tick"] = round(res["engine_ms"] / kept["ticks"], 4)
    res[f"denoise_b{cap}_ms_per_step"] = round(timed(denoise_b4, max(args.iters, 2), 1) / 50, 4)
    res["single_over_engine"] = round(res["single_ms"] / res["engine_ms"], 3)
    res["grouped_over_engine"] = round(res["grouped_ms"] / res["engine_ms"], 3)
    a, b = kept["engine0"].float(), kept["single0"].float()
    res["request0_rel_l2_engine_vs_single"] = round(float((a - b).norm() / b.norm()), 6)
    D.synchronize()
    eng.close()
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
