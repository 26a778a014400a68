"""Quadrilateral regions with oriented crops (prepost.preprocess_quads / postprocess_quads / rectify_quads) against the axis-aligned
paged pair on the quads' bounding rectangles, same process, same pages:

    python scripts/bench_edit_quads.py [--iters N] [--warmup W] [--out FILE]

B = 4 / 16 / 64 text lines skewed by +-3 degrees on 1100 x 1300 uint8 pages (B <= 16: one line per page; B = 64: four lines on each of 16
pages), S = 512.  Prints one JSON line (and writes it to --out, default profiles/edit_quads_line.json); ms per call, wall clock around
`iters` synchronised calls, the MEDIAN of 7 such windows taken round-robin over the three candidates:
  quads_ms     one preprocess_quads + one postprocess_quads
  boxes_ms     one preprocess_pages + one postprocess_pages on the bounding rectangles (crop plan: prepost.plan_pages, seeded)
  rectify_ms   one rectify_quads
quads_over_boxes is their ratio; *_spread is (max - min) / median over the 7 windows.  min_bytes is what the quad pair must move at
least (every page read and written once by the paste, four taps of three bytes read and the four outputs written per crop pixel) and
quads_gbps that over quads_ms - a whole-call rate, host time included, not a kernel's share of peak.  Both pairs move the same bytes,
do two launches and two table uploads; what differs is the per-pixel integer work and the host's table preparation.
mask_spared: the share of the bounding rectangle's mask pixels that the quad mask leaves alone, for an 800 x 30 line at 3 and 10 degrees
(counted on the host; no timing)."""
import argparse
import json
import math
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402


def tilted(cx, cy, length, height, degrees):
    t = math.radians(degrees)
    ux, uy, vx, vy = math.cos(t), math.sin(t), -math.sin(t), math.cos(t)
    return [(int(round(cx + sx * length / 2 * ux + sy * height / 2 * vx)), int(round(cy + sx * length / 2 * uy + sy * height / 2 * vy)))
            for sx, sy in ((-1, -1), (1, -1), (1, 1), (-1, 1))]


def bbox(quad):
    xs, ys = [c[0] for c in quad], [c[1] for c in quad]
    return (min(xs), min(ys), max(xs), max(ys))


def quad_pixels(quad):
    x1, y1, x2, y2 = bbox(quad)
    Y, X = np.mgrid[y1:y2 + 1, x1:x2 + 1].astype(np.int64)
    ok = np.ones(X.shape, bool)
    for k in range(4):
        (xa, ya), (xb, yb) = quad[k], quad[(k + 1) % 4]
        ok &= (xb - xa) * (Y - ya) - (yb - ya) * (X - xa) >= 0
    return int(ok.sum()), (x2 - x1 + 1) * (y2 - y1 + 1)


def window(fn, iters):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / iters * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=300)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "edit_quads_line.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise RuntimeError("bench_edit_quads: no GPU visible; nothing is measured on the CPU")
    import diffute_amd as D
    from diffute_amd import prepost
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    h, w, S = 1100, 1300, 512
    res = dict(bench="edit_quads", page=[h, w], size=S, iters=args.iters, windows=7, skew_degrees=3)
    spared = {}
    for deg in (3, 10):
        inside, box = quad_pixels(tilted(650, 550, 800, 30, deg))
        spared[f"{deg}deg"] = round(1.0 - inside / box, 4)
    res["mask_spared"] = spared
    for B in (4, 16, 64):
        P = min(B, 16)
        per = B // P
        rs = np.random.RandomState(B)
        imgs = [torch.from_numpy(rs.randint(0, 256, (h, w, 3), dtype=np.uint8)).to(dev) for _ in range(P)]
        quads = [[tilted(350 + 600 * (j % 2), 200 + 250 * (j // 2) + 40 * (p % 4), 200 + 60 * ((p + j) % 4), (18, 40, 60, 80)[(p + j) % 4], 3 if (p + j) % 2 else -3)
                  for j in range(per)] for p in range(P)]
        frames = prepost.plan_quads(quads, [(h, w)] * P)
        boxes = [[bbox(q) for q in qs] for qs in quads]
        plans = prepost.plan_pages(boxes, [(h, w)] * P, np.random.RandomState(1))
        origins, crops = [[p[:2] for p in pl] for pl in plans], [[p[2] for p in pl] for pl in plans]
        dec = (torch.randn(B, 3, S, S, generator=torch.Generator().manual_seed(5)) * 0.6).clamp(-1.3, 1.3).to(dev)
        outs = [torch.empty_like(img) for img in imgs]

        def quad_pair():
            pre = prepost.preprocess_quads(imgs, quads, frames, size=S)
            return pre, prepost.postprocess_quads(dec, imgs, quads, frames, out=outs)

        def box_pair():
            pre = prepost.preprocess_pages(imgs, boxes, origins, crops, size=S)
            return pre, prepost.postprocess_pages(dec, imgs, boxes, origins, crops, out=outs)

        def rectify():
            return prepost.rectify_quads(imgs, quads)

        cands = {"quads_ms": quad_pair, "boxes_ms": box_pair, "rectify_ms": rectify}
        for fn in cands.values():
            for _ in range(args.warmup):
                fn()
        times = {k: [] for k in cands}
        for _ in range(7):                                   # round-robin: a drift of the machine hits every candidate alike
            for k, fn in cands.items():
                times[k].append(window(fn, args.iters))
        r = dict(pages=P, quads_per_page=per, crop_scales=sorted({f[2] for fs in frames for f in fs}))
        for k, v in times.items():
            r[k] = round(float(np.median(v)), 4)
            r[k.replace("_ms", "_spread")] = round(float((max(v) - min(v)) / np.median(v)), 3)
        r["quads_over_boxes"] = round(r["quads_ms"] / r["boxes_ms"], 3)
        min_bytes = 2 * P * h * w * 3 + B * S * S * (4 * 3 + (3 + 3) * 4 + 1)      # (the paste's reads of the decoder outputs - quad pixels only - left out)
        r["min_bytes"] = int(min_bytes)
        r["quads_gbps"] = round(min_bytes / (r["quads_ms"] * 1e-3) / 1e9, 1)
        res[f"B{B}"] = r
    D.synchronize()
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
