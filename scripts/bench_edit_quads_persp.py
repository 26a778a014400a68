"""The projective frame for quadrilateral regions (prepost.preprocess_quads / postprocess_quads / rectify_quads with perspective=True)
against the similarity frame on the SAME quads, same process, same pages:

    python scripts/bench_edit_quads_persp.py [--iters N] [--warmup W] [--out FILE]

The workload of scripts/bench_edit_quads.py - B = 4 / 16 / 64 text lines skewed by +-3 degrees on 1100 x 1300 uint8 pages (B <= 16: one
line per page; B = 64: four lines on each of 16 pages), S = 512 - with a mild keystone on every line: its right edge shrunk to 0.8 of
its left edge's height about its own midpoint.  Prints one JSON line (and writes it to --out, default
profiles/edit_quads_persp_line.json); ms per call, wall clock around `iters` synchronised calls, the MEDIAN of 7 such windows taken
round-robin over the four candidates:
  persp_ms            one preprocess_quads + one postprocess_quads, perspective=True, frames from plan_quads(perspective=True)
  quads_ms            the same pair through the similarity frames of plan_quads
  rectify_persp_ms    one rectify_quads(perspective=True)
  rectify_ms          one rectify_quads
persp_over_quads and rectify_persp_over_rectify are the ratios; *_spread is (max - min) / median over the 7 windows.  Whole-call times,
host included: both pairs do two launches and two table uploads; the projective pair adds the exact 128-bit table preparation on the
host (once in the prepare entry and once more in each launch entry's re-check) and four 64-bit divisions per pixel on the device.
prepare_us is the host preparation alone: one dmx_edit_quads_persp_prepare call over the B items, median of 200."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from bench_edit_quads import tilted, window  # noqa: E402


def keystoned(quad, ratio=0.8):
    """the right edge (TR, BR) shrunk to `ratio` of its length about its midpoint, rounded"""
    (x0, y0), (x1, y1), (x2, y2), (x3, y3) = quad
    mx, my = (x1 + x2) / 2.0, (y1 + y2) / 2.0
    tr = (int(round(mx + ratio * (x1 - mx))), int(round(my + ratio * (y1 - my))))
    br = (int(round(mx + ratio * (x2 - mx))), int(round(my + ratio * (y2 - my))))
    return [(x0, y0), tr, br, (x3, y3)]


def prepare_us(prepost, quads, frames, h, w, S):
    """the host preparation of the projective table alone, in microseconds: median of 200 calls"""
    import ctypes
    from diffute_amd import _cabi
    flat_q = [prepost._corners(q) for qs in quads for q in qs]
    flat_f = [f for fs in frames for f in fs]
    P, B = len(quads), len(flat_q)
    pages, host, persp = (_cabi.EditPage * P)(), (_cabi.EditQuad * B)(), (_cabi.QuadPersp * B)()
    lo = 0
    for p, qs in enumerate(quads):
        pages[p].original, pages[p].H, pages[p].W, pages[p].item_lo, pages[p].item_hi = 64, h, w, lo, lo + len(qs)
        lo += len(qs)
    for b, (c, f) in enumerate(zip(flat_q, flat_f)):
        for k in range(4):
            host[b].x[k], host[b].y[k] = c[k]
        host[b].cx2, host[b].cy2, host[b].crop_scale, host[b].ux, host[b].uy = 2 * c[0][0], 2 * c[0][1], 1, 1, 0
        host[b].page = next(p for p in range(P) if pages[p].item_lo <= b < pages[p].item_hi)
        persp[b].ci2, persp[b].cj2, persp[b].crop_scale = f
    lib = _cabi.lib()
    _cabi.check(lib.dmx_edit_quads_prepare(pages, P, host, B, S), "edit_quads_prepare")
    ts = []
    for _ in range(200):
        t0 = time.perf_counter()
        rc = lib.dmx_edit_quads_persp_prepare(pages, P, host, persp, B, S)
        ts.append(time.perf_counter() - t0)
        _cabi.check(rc, "edit_quads_persp_prepare")
    return round(float(np.median(ts)) * 1e6, 1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=300)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "edit_quads_persp_line.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise RuntimeError("bench_edit_quads_persp: no GPU visible; nothing is measured on the CPU")
    import diffute_amd as D
    from diffute_amd import prepost
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    h, w, S = 1100, 1300, 512
    res = dict(bench="edit_quads_persp", page=[h, w], size=S, iters=args.iters, windows=7, skew_degrees=3, keystone=0.8)
    for B in (4, 16, 64):
        P = min(B, 16)
        per = B // P
        rs = np.random.RandomState(B)
        imgs = [torch.from_numpy(rs.randint(0, 256, (h, w, 3), dtype=np.uint8)).to(dev) for _ in range(P)]
        quads = [[keystoned(tilted(350 + 600 * (j % 2), 200 + 250 * (j // 2) + 40 * (p % 4), 200 + 60 * ((p + j) % 4), (18, 40, 60, 80)[(p + j) % 4],
                                   3 if (p + j) % 2 else -3)) for j in range(per)] for p in range(P)]
        frames = prepost.plan_quads(quads, [(h, w)] * P)
        pframes = prepost.plan_quads(quads, [(h, w)] * P, perspective=True, size=S)
        dec = (torch.randn(B, 3, S, S, generator=torch.Generator().manual_seed(5)) * 0.6).clamp(-1.3, 1.3).to(dev)
        outs = [torch.empty_like(img) for img in imgs]

        def persp_pair():
            pre = prepost.preprocess_quads(imgs, quads, pframes, size=S, perspective=True)
            return pre, prepost.postprocess_quads(dec, imgs, quads, pframes, out=outs, perspective=True)

        def quad_pair():
            pre = prepost.preprocess_quads(imgs, quads, frames, size=S)
            return pre, prepost.postprocess_quads(dec, imgs, quads, frames, out=outs)

        def rectify_persp():
            return prepost.rectify_quads(imgs, quads, perspective=True)

        def rectify():
            return prepost.rectify_quads(imgs, quads)

        cands = {"persp_ms": persp_pair, "quads_ms": quad_pair, "rectify_persp_ms": rectify_persp, "rectify_ms": rectify}
        for fn in cands.values():
            for _ in range(args.warmup):
                fn()
        times = {k: [] for k in cands}
        for _ in range(7):                                   # round-robin: a drift of the machine hits every candidate alike
            for k, fn in cands.items():
                times[k].append(window(fn, args.iters))
        r = dict(pages=P, quads_per_page=per, crop_scales=sorted({f[2] for fs in pframes for f in fs}))
        for k, v in times.items():
            r[k] = round(float(np.median(v)), 4)
            r[k.replace("_ms", "_spread")] = round(float((max(v) - min(v)) / np.median(v)), 3)
        r["persp_over_quads"] = round(r["persp_ms"] / r["quads_ms"], 3)
        r["rectify_persp_over_rectify"] = round(r["rectify_persp_ms"] / r["rectify_ms"], 3)
        r["prepare_us"] = prepare_us(prepost, quads, pframes, h, w, S)
        res[f"B{B}"] = r
    D.synchronize()
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
