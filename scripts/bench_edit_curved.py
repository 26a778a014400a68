"""Curved regions (prepost.preprocess_curved / postprocess_curved / rectify_curved) against the projective quad calls on the SAME lines
given as one quad (n = 2), same process, same pages:

    python scripts/bench_edit_curved.py [--iters N] [--warmup W] [--out FILE]

B = 4 / 16 / 64 text lines on arcs - about 300 pixels long, 40 high, bent through 30 degrees, every arc a polygon of 14 points (M = 6
cells, 12 affine pieces) - on 1100 x 1300 uint8 pages (B <= 16: one line per page; B = 64: four lines on each of 16 pages), S = 512.
Prints one JSON line (and writes it to --out, default profiles/edit_curved_line.json); ms per call, wall clock around `iters`
synchronised calls, the MEDIAN of 7 such windows taken round-robin over the four candidates:
  curved_ms           one preprocess_curved + one postprocess_curved, frames from plan_curved
  persp_ms            one preprocess_quads + one postprocess_quads, perspective=True, on the arcs' four outer points as quads
  rectify_curved_ms   one rectify_curved
  rectify_persp_ms    one rectify_quads(perspective=True)
curved_over_persp and rectify_curved_over_rectify_persp are the ratios; *_spread is (max - min) / median over the 7 windows.  Whole-call
times, WALL CLOCK WITH THE HOST INCLUDED: both pairs do two launches and two table uploads; the curved pair prepares twelve exact
128-bit piece tables per line where the projective pair prepares one (once in the prepare entry and once more in each launch entry's
re-check).  prepare_us is that host preparation alone: one dmx_edit_curved_prepare call over the B items, median of 200.  No ratio is
expected in advance: the numbers are what the run found."""
import argparse
import json
import math
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from bench_edit_quads import window  # noqa: E402

CELLS = 6


def arc(cx, cy, r_in, r_out, deg0, deg1, n):
    """an annular sector as 2n points: the outer arc from deg0 to deg1 (y down), the inner arc back"""
    ang = [math.radians(deg0 + (deg1 - deg0) * k / (n - 1)) for k in range(n)]
    top = [(int(round(cx + r_out * math.cos(a))), int(round(cy + r_out * math.sin(a)))) for a in ang]
    bot = [(int(round(cx + r_in * math.cos(a))), int(round(cy + r_in * math.sin(a)))) for a in ang]
    return top + bot[::-1]


def as_quad(poly):
    n = len(poly) // 2
    return [poly[0], poly[n - 1], poly[n], poly[2 * n - 1]]


def prepare_us(prepost, polygons, frames, h, w, S):
    """the host preparation of the curved tables alone, in microseconds: median of 200 calls"""
    from diffute_amd import _cabi
    flat = [prepost._polygon(q) for qs in polygons for q in qs]
    flat_f = [f for fs in frames for f in fs]
    P, B, NP = len(polygons), len(flat), sum(len(c) - 2 for c in flat)
    pages, host, pieces = (_cabi.EditPage * P)(), (_cabi.EditCurved * B)(), (_cabi.CurvedPiece * NP)()
    lo = 0
    for p, qs in enumerate(polygons):
        pages[p].original, pages[p].H, pages[p].W, pages[p].item_lo, pages[p].item_hi = 64, h, w, lo, lo + len(qs)
        for b in range(lo, lo + len(qs)):
            for k, (x, y) in enumerate(flat[b]):
                host[b].x[k], host[b].y[k] = x, y
            host[b].count, host[b].page = len(flat[b]), p
            host[b].ci2, host[b].cj2, host[b].crop_scale = flat_f[b]
        lo += len(qs)
    lib = _cabi.lib()
    ts = []
    for _ in range(200):
        t0 = time.perf_counter()
        rc = lib.dmx_edit_curved_prepare(pages, P, host, pieces, B, S)
        ts.append(time.perf_counter() - t0)
        _cabi.check(rc, "edit_curved_prepare")
    return round(float(np.median(ts)) * 1e6, 1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=300)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "edit_curved_line.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise RuntimeError("bench_edit_curved: no GPU visible; nothing is measured on the CPU")
    import diffute_amd as D
    from diffute_amd import prepost
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    h, w, S = 1100, 1300, 512
    res = dict(bench="edit_curved", page=[h, w], size=S, iters=args.iters, windows=7, cells=CELLS, arc_degrees=30, timing="wall clock, host included")
    for B in (4, 16, 64):
        P = min(B, 16)
        per = B // P
        rs = np.random.RandomState(B)
        imgs = [torch.from_numpy(rs.randint(0, 256, (h, w, 3), dtype=np.uint8)).to(dev) for _ in range(P)]
        # the arcs' centres lie 600 pixels below their lines: radii 580 .. 620, 255 to 285 degrees
        polys = [[arc(350 + 600 * (j % 2), 800 + 250 * (j // 2) + 40 * (p % 4), 580, 620 + 10 * ((p + j) % 3), 255, 285, CELLS + 1) for j in range(per)]
                 for p in range(P)]
        quads = [[as_quad(q) for q in qs] for qs in polys]
        cframes = prepost.plan_curved(polys, [(h, w)] * P, size=S)
        pframes = prepost.plan_quads(quads, [(h, w)] * P, perspective=True, size=S)
        dec = (torch.randn(B, 3, S, S, generator=torch.Generator().manual_seed(5)) * 0.6).clamp(-1.3, 1.3).to(dev)
        outs = [torch.empty_like(img) for img in imgs]

        def curved_pair():
            pre = prepost.preprocess_curved(imgs, polys, cframes, size=S)
            return pre, prepost.postprocess_curved(dec, imgs, polys, cframes, out=outs)

        def persp_pair():
            pre = prepost.preprocess_quads(imgs, quads, pframes, size=S, perspective=True)
            return pre, prepost.postprocess_quads(dec, imgs, quads, pframes, out=outs, perspective=True)

        def rectify_curved():
            return prepost.rectify_curved(imgs, polys)

        def rectify_persp():
            return prepost.rectify_quads(imgs, quads, perspective=True)

        cands = {"curved_ms": curved_pair, "persp_ms": persp_pair, "rectify_curved_ms": rectify_curved, "rectify_persp_ms": rectify_persp}
        for fn in cands.values():
            for _ in range(args.warmup):
                fn()
        times = {k: [] for k in cands}
        for _ in range(7):                                   # round-robin: a drift of the machine hits every candidate alike
            for k, fn in cands.items():
                times[k].append(window(fn, args.iters))
        r = dict(pages=P, lines_per_page=per, crop_scales=sorted({f[2] for fs in cframes for f in fs}))
        for k, v in times.items():
            r[k] = round(float(np.median(v)), 4)
            r[k.replace("_ms", "_spread")] = round(float((max(v) - min(v)) / np.median(v)), 3)
        r["curved_over_persp"] = round(r["curved_ms"] / r["persp_ms"], 3)
        r["rectify_curved_over_rectify_persp"] = round(r["rectify_curved_ms"] / r["rectify_persp_ms"], 3)
        r["prepare_us"] = prepare_us(prepost, polys, cframes, h, w, S)
        res[f"B{B}"] = r
    D.synchronize()
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
