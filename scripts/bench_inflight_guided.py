"""In-flight batching with per-request classifier-free guidance (DenoiseEngine.submit(guidance=)) against what denoise() offers the same
requests, same process:

    python scripts/bench_inflight_guided.py [--requests N] [--iters N] [--warmup W] [--out FILE]

Full-size UNet with random weights, 512 px (64 x 64 latents, 577 context tokens), DDIM, an engine of capacity 8.  N = 16 single-sample
requests, all queued at the start, their step counts drawn with a fixed seed from {20, 30, 50}; half of them guided (the zero unconditional
context), scales drawn from {3.0, 7.5}, half of the guided ones with rescale 0.7.  A guided request holds two engine rows.  Prints one JSON
line (and writes it to --out, default profiles/inflight_guided_line.json); total ms per pass over all requests (wall clock, synchronised) and
requests/s of three arms:
  engine    DenoiseEngine(capacity=8): submit all, run_until_idle (the engine lives across passes, as in a service)
  single    one batch-1 denoise() / denoise(guidance=) per request
  grouped   the best available without the engine: requests of equal step count and equal guidance in one denoise() batch of up to 8 rows
and, in the same run on the same engine, ms per tick of a full engine of guided pairs (4 requests of 50 steps: a guided row in every tick)
beside ms per tick of a full all-plain engine (8 requests of 50 steps).  No ratio is promised; the structural expectation - a tick with
guided rows launches what a plain tick launches - is held by tests/test_inflight_guided_gpu.py."""
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
    ap.add_argument("--capacity", type=int, default=8)
    ap.add_argument("--iters", type=int, default=2)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "inflight_guided_line.json"))
    args = ap.parse_args()
    import diffute_amd as D
    from diffute_amd.inflight import Planner
    from diffute_amd.synthetic import synth_inputs
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    N, cap = args.requests, args.capacity
    rng = np.random.RandomState(args.seed)
    steps = [int(s) for s in rng.choice([20, 30, 50], size=N)]
    guided = sorted(int(i) for i in rng.choice(N, size=N // 2, replace=False))
    scales = {i: float(s) for i, s in zip(guided, rng.choice([3.0, 7.5], size=len(guided)))}
    rescaled = set(int(i) for i in rng.choice(guided, size=len(guided) // 2, replace=False))
    key = [None if i not in scales else (scales[i], 0.7 if i in rescaled else 0.0) for i in range(N)]        # the guidance of request i
    guidance = [None if k is None else D.Guidance(*k) for k in key]
    unet = D.UNet2DConditionModel(device=dev).requires_grad_(False)
    reqs = [synth_inputs(1, 64, 64, 577, 1024, seed=10 * i, device=dev) for i in range(N)]
    res = dict(bench="inflight_guided", requests=N, capacity=cap, steps=steps, guidance=[list(k) if k else None for k in key],
               total_steps=sum(steps), total_row_steps=sum(s * (2 if k else 1) for s, k in zip(steps, key)), iters=args.iters, scheduler="ddim")
    kept = {}

    eng = D.DenoiseEngine(unet, D.DDIMScheduler(), capacity=cap, latent_shape=(4, 64, 64), ctx_len=577)

    def engine():
        t0 = eng.planner.ticks
        tk = [eng.submit(*reqs[i], steps[i], guidance=guidance[i]) for i in range(N)]
        eng.run_until_idle()
        kept["ticks"] = eng.planner.ticks - t0
        kept["engine"] = [eng.result(t) for t in tk]

    def single():
        kept["single"] = [D.denoise(unet, D.DDIMScheduler(), *reqs[i], steps[i], guidance=guidance[i]) for i in range(N)]

    groups = []
    for T, k in sorted(set(zip(steps, key)), key=lambda v: (v[0], v[1] or (0.0, 0.0))):
        ids = [i for i in range(N) if steps[i] == T and key[i] == k]
        per = cap if k is None else cap // 2                   # a guided batch of b samples is a 2b-row forward
        groups += [(T, k, ids[j:j + per]) for j in range(0, len(ids), per)]
    batches = [(T, k, [torch.cat([reqs[i][j] for i in ids], 0) for j in range(4)]) for T, k, ids in groups]

    def grouped():
        for T, k, b in batches:
            D.denoise(unet, D.DDIMScheduler(), *b, T, guidance=None if k is None else D.Guidance(*k))

    def full(g):
        """a full engine for 50 ticks: capacity plain requests, or capacity / 2 guided ones"""
        n = cap if g is None else cap // 2

        def run():
            tk = [eng.submit(*reqs[i], 50, guidance=g) for i in range(n)]
            eng.run_until_idle()
            for t in tk:
                eng.result(t)
        return run

    for name, fn in (("engine", engine), ("single", single), ("grouped", grouped)):
        ms = timed(fn, args.iters, args.warmup)
        res[f"{name}_ms"] = round(ms, 2)
        res[f"{name}_requests_per_s"] = round(N / ms * 1e3, 3)
    res["grouped_batches"] = [[T, list(k) if k else None, len(ids)] for T, k, ids in groups]
    # the ticks of the engine pass and those with a guided request running: the same submits through a planner of its own (no device)
    pl, gt, with_guided = Planner(cap), set(), 0
    for i in range(N):
        t = pl.submit(2 if key[i] else 1, steps[i], 0)
        if key[i]:
            gt.add(t)
    while pl.busy():
        pl.admit()
        with_guided += int(any(t in gt for t in pl.running))
        pl.advance()
    assert pl.ticks == kept["ticks"], (pl.ticks, kept["ticks"])
    res["engine_ticks"] = kept["ticks"]
    res["engine_ticks_with_guided_rows"] = with_guided
    res["engine_rows_busy"] = round(res["total_row_steps"] / (cap * kept["ticks"]), 4)
    res["engine_ms_per_tick"] = round(res["engine_ms"] / kept["ticks"], 4)
    res["full_guided_ms_per_tick"] = round(timed(full(D.Guidance(7.5, 0.7)), max(args.iters, 2), 1) / 50, 4)
    res["full_plain_ms_per_tick"] = round(timed(full(None), max(args.iters, 2), 1) / 50, 4)
    res["guided_over_plain_tick"] = round(res["full_guided_ms_per_tick"] / res["full_plain_ms_per_tick"], 4)
    res["single_over_engine"] = round(res["single_ms"] / res["engine_ms"], 3)
    res["grouped_over_engine"] = round(res["grouped_ms"] / res["engine_ms"], 3)
    # the engine's latents against the batch-1 chains (other batch sizes, hence other tile plans: no threshold is applied)
    rel = [float((a.float() - b.float()).norm() / b.float().norm()) for a, b in zip(kept["engine"], kept["single"])]
    res["rel_l2_engine_vs_single_max_plain"] = round(max(r for r, k in zip(rel, key) if k is None), 6)
    res["rel_l2_engine_vs_single_max_guided"] = round(max(r for r, k in zip(rel, key) if k is not None), 6)
    res["finite"] = bool(all(torch.isfinite(o).all() for o in kept["engine"]))
    D.synchronize()
    eng.close()
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
