"""What a change to the denoise loop does to the PAGE a user gets back, measured on the edited boxes with diffute_amd.metrics:

    python scripts/eval_edits.py [--weights DIR] [--ocr DIR --labels FILE.json] [--steps 50] [--guidance] [--out FILE]

A synthetic 1100 x 1300 page (white, dark strokes), N = 4 boxes (scripts/bench_edit.py's), 512 px.  The base is the plain DDIM-50 loop;
the variants are cache_interval 2 / 3 / 5, DPM-Solver++ 20 / 25 and, where the library is built, the fp16 build.  Per variant, against
the base's page and all from box_metrics / outside_diff: per-box MSE / PSNR / SSIM, their mean and worst box, and changed_outside against
the ORIGINAL page, which must be 0 for every variant (the script exits 1 otherwise).

--weights DIR: a diffusers directory with unet/ and vae/.  Without it the weights are random and the line says so: the figures then are
pixel-space distances between runs of a random network - better than the rel-L2 of latents they replace, no statement about quality.
--ocr DIR (a TrOCR VisionEncoderDecoder directory) with --labels FILE.json (N lists of token ids, the text each box should show): also the
share of boxes whose teacher-forced arg-max equals the labels (ocr.score), per variant.
--guidance: also the guided variants - classifier-free guidance (diffute_amd.Guidance, the zero context as the unconditional one) at
scale 3 and 7.5, and 7.5 with rescale 0.7 - on the base's loop.  Without the flag the line is what it always was.

It also times box_metrics_pages at N = 4 / 16 / 64 boxes of 40 x 200 px against the same numbers from a chain of torch ops on the device
(per box one conv2d over x, y, x^2, y^2, xy with the 11 x 11 window): median of 7, one process.  Prints one JSON line
(profiles/eval_edits_line.json)."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from bench_edit import boxes_for  # noqa: E402


def synthetic_page(h, w, seed=0):
    """a document: white, dark horizontal strokes of word size in text lines"""
    rs = np.random.RandomState(seed)
    img = np.full((h, w, 3), 255, dtype=np.uint8)
    for y in range(40, h - 40, 32):
        x = 40
        while x < w - 120:
            n = int(rs.randint(20, 110))
            img[y:y + int(rs.randint(8, 20)), x:x + n] = rs.randint(10, 90, 3)
            x += n + int(rs.randint(8, 30))
    return img


def median_ms(fn, reps=7, warmup=2):
    ts = []
    for r in range(warmup + reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        if r >= warmup:
            ts.append((time.perf_counter() - t0) * 1e3)
    return sorted(ts)[len(ts) // 2]


def torch_chain(a, b, boxes, window):
    """the numbers of box_metrics from torch ops on the device, box by box: (sse [N,3] int64, ssim [N,3] fp32)"""
    c1, c2 = (0.01 * 255) ** 2, (0.03 * 255) ** 2
    sse, ssim = [], []
    for x1, y1, x2, y2 in boxes:
        x, y = (t[y1:y2, x1:x2].permute(2, 0, 1).unsqueeze(1).to(torch.float32) for t in (a, b))
        d = (x - y).to(torch.int64)
        sse.append((d * d).sum((1, 2, 3)))
        m = torch.nn.functional.conv2d(torch.cat([x, y, x * x, y * y, x * y]), window)
        ux, uy, xx, yy, xy = m[0:3], m[3:6], m[6:9], m[9:12], m[12:15]
        vx, vy, vxy = xx - ux * ux, yy - uy * uy, xy - ux * uy
        s = ((2 * ux * uy + c1) * (2 * vxy + c2)) / ((ux * ux + uy * uy + c1) * (vx + vy + c2))
        ssim.append(s.mean((1, 2, 3)))
    return torch.stack(sse), torch.stack(ssim)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--weights", default=None, help="diffusers directory with unet/ and vae/ (default: random weights)")
    ap.add_argument("--ocr", default=None, help="TrOCR VisionEncoderDecoder directory: report the share of boxes that read as their labels")
    ap.add_argument("--labels", default=None, help="JSON file: N lists of token ids (needed with --ocr)")
    ap.add_argument("--steps", type=int, default=50, help="DDIM steps of the base")
    ap.add_argument("--guidance", action="store_true", help="add the classifier-free-guidance variants (scale 3, 7.5, 7.5 with rescale 0.7)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if (args.ocr is None) != (args.labels is None):
        ap.error("--ocr and --labels go together")
    import diffute_amd as D
    from diffute_amd import _cabi, metrics, prepost
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    h, w, S, N = 1100, 1300, 512, 4
    page = torch.from_numpy(synthetic_page(h, w)).to(dev)
    if args.weights:
        unet = D.UNet2DConditionModel.from_pretrained(args.weights, subfolder="unet").to(dev).requires_grad_(False)
        vae = D.AutoencoderKL.from_pretrained(args.weights, subfolder="vae").to(dev).requires_grad_(False)
    else:
        unet = D.UNet2DConditionModel(device=dev).requires_grad_(False)
        vae = D.AutoencoderKL(device=dev).requires_grad_(False)
    boxes = boxes_for(N, h, w)
    plans = prepost.plan_edits(boxes, h, w, np.random.RandomState(1))
    origins, crops = [p[:2] for p in plans], [p[2] for p in plans]
    ctx = torch.randn(N, 577, 1024, generator=torch.Generator().manual_seed(2)).to(dev)
    noise = torch.randn(N, 4, S // 8, S // 8, generator=torch.Generator().manual_seed(3)).to(dev)
    ocr = proc = labels = None
    if args.ocr:
        ocr = D.VisionEncoderDecoderModel.from_pretrained(args.ocr).to(dev)
        proc = D.TrOCRProcessor.from_pretrained(args.ocr) if os.path.exists(os.path.join(args.ocr, "preprocessor_config.json")) else D.TrOCRProcessor()
        with open(args.labels) as f:
            labels = torch.tensor(json.load(f), dtype=torch.int64)
        if labels.shape[0] != N:
            ap.error(f"--labels holds {labels.shape[0]} rows, the page has {N} boxes")

    def edit(sched, steps, **kw):
        return D.edit_boxes(unet, vae, sched, page, boxes, ctx, steps, origins=origins, crop_scales=crops, enc_noise=noise, size=S, **kw)

    def reads_as_labels(edited):
        if ocr is None:
            return None
        pv = proc(images=[edited[y1:y2, x1:x2] for x1, y1, x2, y2 in boxes]).pixel_values
        pred = ocr.score(pv, labels=labels.to(dev)).predictions
        return round(float(((pred == labels.to(dev)) | (labels.to(dev) < 0)).all(1).double().mean()), 4)

    variants = [(f"ddim{args.steps}_interval{n}", lambda n=n: edit(D.DDIMScheduler(), args.steps, cache_interval=n)) for n in (2, 3, 5)]
    variants += [(f"dpmpp2m_{s}", lambda s=s: edit(D.DPMSolverMultistepScheduler(), s)) for s in (20, 25)]
    if args.guidance:
        variants += [(f"ddim{args.steps}_guidance{sc:g}" + (f"_rescale{rs:g}" if rs else ""),
                      lambda sc=sc, rs=rs: edit(D.DDIMScheduler(), args.steps, guidance=D.Guidance(sc, rs))) for sc, rs in ((3.0, 0.0), (7.5, 0.0), (7.5, 0.7))]
    base = edit(D.DDIMScheduler(), args.steps)
    ok = bool(torch.equal(base, edit(D.DDIMScheduler(), args.steps)))            # the base itself repeats bit for bit
    base_out = metrics.outside_diff(page, base, boxes)
    ok &= int(base_out.changed[0]) == 0
    res = {}

    def report(name, edited):
        nonlocal ok
        m, o = metrics.box_metrics(base, edited, boxes), metrics.outside_diff(page, edited, boxes)
        r = dict(mse=[round(v, 4) for v in m.mse.tolist()], psnr=[round(v, 3) for v in m.psnr.tolist()], ssim=[round(v, 6) for v in m.ssim.tolist()],
                 mse_mean=round(float(m.mse.mean()), 4), mse_worst=round(float(m.mse.max()), 4), psnr_mean=round(float(m.psnr.mean()), 3),
                 psnr_worst=round(float(m.psnr.min()), 3), ssim_mean=round(float(m.ssim.mean()), 6), ssim_worst=round(float(m.ssim.min()), 6),
                 changed_outside=int(o.changed[0]), sse_outside=int(o.sse[0]))
        share = reads_as_labels(edited)
        if share is not None:
            r["boxes_reading_as_labels"] = share
        ok &= r["changed_outside"] == 0
        res[name] = r

    for name, fn in variants:
        report(name, fn())
    if os.path.exists(_cabi._LIB_PATH_F16):                                      # the fp16 build, where present: the same weights, the same loop
        unet.to(dtype=torch.float16)
        vae.to(dtype=torch.float16)
        report(f"ddim{args.steps}_fp16_build", edit(D.DDIMScheduler(), args.steps))
    base_vs_original = metrics.box_metrics(page, base, boxes)
    D.synchronize()

    # ---- the metrics themselves, timed: N boxes of 40 x 200 px on the two pages
    g = np.exp(-(np.arange(-5, 6) ** 2) / 4.5)
    win = torch.from_numpy(np.outer(g / g.sum(), g / g.sum())).to(dev, torch.float32).reshape(1, 1, 11, 11)
    other = base.flip(0).contiguous()                                           # any second page of the same size
    timing = {}
    for n in (4, 16, 64):
        grid = [(10 + 210 * (i % 6), 10 + 45 * (i // 6), 10 + 210 * (i % 6) + 200, 10 + 45 * (i // 6) + 40) for i in range(n)]
        kept = {}

        def hip():
            kept["m"] = metrics.box_metrics_pages([base], [other], [grid])

        def chain():
            kept["t"] = torch_chain(base, other, grid, win)

        t_hip, t_chain = median_ms(hip), median_ms(chain)
        sse_equal = bool(torch.equal(kept["m"].sse, kept["t"][0]))
        ok &= sse_equal
        timing[f"n{n}"] = dict(box_metrics_pages_ms=round(t_hip, 4), torch_chain_ms=round(t_chain, 4), chain_over_hip=round(t_chain / t_hip, 2),
                               sse_equal=sse_equal, ssim_max_abs_diff_from_plain_fp32_torch=float((kept["m"].ssim_rgb - kept["t"][1]).abs().max()))
    D.synchronize()
    line = json.dumps(dict(
        bench="eval_edits", image=[h, w], size=S, boxes=N, box_sizes=[[x2 - x1, y2 - y1] for x1, y1, x2, y2 in boxes],
        weights=args.weights or "random", base=f"ddim{args.steps}", ok=ok,
        note=None if args.weights else "random weights: distances between runs of a random network in pixel space, no statement about image quality",
        base_vs_original=dict(psnr=[round(v, 3) for v in base_vs_original.psnr.tolist()], ssim=[round(v, 6) for v in base_vs_original.ssim.tolist()],
                              changed_outside=int(base_out.changed[0])),
        base_reads_as_labels=reads_as_labels(base), variants_vs_base=res,
        metrics_timing=dict(box_px=[200, 40], reps=7, unit="ms per call, host wall clock around a synchronise", **timing)))
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    if not ok:
        sys.exit(1)


if __name__ == "__main__":
    main()
