"""The feathered, colour-matched paste for quads (prepost.postprocess_quads / postprocess_select_quads with blend=QuadBlend(...)) against
the plain quad paste of the SAME quads, same process, same pages, in both frames:

    python scripts/bench_quad_blend.py [--iters N] [--warmup W] [--out FILE]

B = 4 / 16 / 64 text lines skewed by +-3 degrees on 1100 x 1300 uint8 pages (B <= 16: one line per page; B = 64: four lines on each of 16
pages), S = 512, the lines of scripts/bench_edit_quads.py.  Prints one JSON line (and writes it to --out, default
profiles/quad_blend_line.json); ms per call, wall clock around `iters` synchronised calls, the MEDIAN of 7 such windows taken round-robin
over the candidates; per frame ("similarity", "projective") and B:
  plain_ms            one postprocess_quads call, blend=None (one launch)
  feather_ms          blend=QuadBlend(feather=4, grow=4) (one launch)
  match_ms            blend=QuadBlend(match_color=True) (stats + paste: two launches)
  both_ms             blend=QuadBlend(feather=4, grow=4, match_color=True) (two launches)
  select_plain_ms     one postprocess_select_quads call over K = 2 candidates per quad, blend=None (one launch)
  select_both_ms      the same with the blend of both_ms: choose -> stats -> paste (three launches)
*_over_plain is the ratio to plain_ms of the same run, select_both_over_select_plain the verified triple against the plain select paste;
*_spread is (max - min) / median over the 7 windows.  Whole-call times, host included: every candidate uploads its tables once."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from bench_edit_quads import tilted, window  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "quad_blend_line.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise RuntimeError("bench_quad_blend: no GPU visible; nothing is measured on the CPU")
    import diffute_amd as D
    from diffute_amd import prepost
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    h, w, S, K = 1100, 1300, 512, 2
    res = dict(bench="quad_blend", page=[h, w], size=S, iters=args.iters, windows=7, candidates=K, skew_degrees=3)
    feather, match = D.QuadBlend(feather=4, grow=4), D.QuadBlend(match_color=True)
    both = D.QuadBlend(feather=4, grow=4, match_color=True)
    for persp in (False, True):
        frame_res = {}
        for B in (4, 16, 64):
            P = min(B, 16)
            per = B // P
            rs = np.random.RandomState(B)
            imgs = [torch.from_numpy(rs.randint(0, 256, (h, w, 3), dtype=np.uint8)).to(dev) for _ in range(P)]
            quads = [[tilted(350 + 600 * (j % 2), 200 + 250 * (j // 2) + 40 * (p % 4), 200 + 60 * ((p + j) % 4), (18, 40, 60, 80)[(p + j) % 4],
                             3 if (p + j) % 2 else -3) for j in range(per)] for p in range(P)]
            frames = prepost.plan_quads(quads, [(h, w)] * P, persp, S)
            dec = (torch.randn(B, K, 3, S, S, generator=torch.Generator().manual_seed(5)) * 0.6).clamp(-1.3, 1.3).to(dev)
            dec0 = dec[:, 0].contiguous()
            scores = torch.randn(B, K, generator=torch.Generator().manual_seed(6)).to(dev)
            outs = [torch.empty_like(img) for img in imgs]

            def paste(blend):
                return lambda: prepost.postprocess_quads(dec0, imgs, quads, frames, out=outs, perspective=persp, blend=blend)

            def select(blend):
                return lambda: prepost.postprocess_select_quads(dec, scores, imgs, quads, frames, out=outs, perspective=persp, blend=blend)

            cands = {"plain_ms": paste(None), "feather_ms": paste(feather), "match_ms": paste(match), "both_ms": paste(both),
                     "select_plain_ms": select(None), "select_both_ms": select(both)}
            for fn in cands.values():
                for _ in range(args.warmup):
                    fn()
            times = {k: [] for k in cands}
            for _ in range(7):                                   # round-robin: a drift of the machine hits every candidate alike
                for k, fn in cands.items():
                    times[k].append(window(fn, args.iters))
            r = dict(pages=P, quads_per_page=per)
            for k, v in times.items():
                r[k] = round(float(np.median(v)), 4)
                r[k.replace("_ms", "_spread")] = round(float((max(v) - min(v)) / np.median(v)), 3)
            for k in ("feather", "match", "both"):
                r[f"{k}_over_plain"] = round(r[f"{k}_ms"] / r["plain_ms"], 3)
            r["select_both_over_select_plain"] = round(r["select_both_ms"] / r["select_plain_ms"], 3)
            frame_res[f"B{B}"] = r
        res["projective" if persp else "similarity"] = frame_res
    D.synchronize()
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
