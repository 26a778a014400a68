"""Text boxes on SEVERAL pages: the paged path (pipeline.edit_pages over prepost.preprocess_pages / postprocess_pages) against what a
service holding one request per image runs without it, same process, same boxes:

    python scripts/bench_edit_pages.py [--iters N] [--warmup W] [--steps T] [--edit-iters N] [--out FILE]

P = 4 and P = 16 pages of 1100 x 1300 uint8 with ONE box each (the crop ladder gives crops of 128 .. 512).  Prints one JSON line (and
writes it to --out, default profiles/edit_pages_line.json); ms per call (wall clock, synchronised):
  prepost    pages     one preprocess_pages + one postprocess_pages
             loop      P x (preprocess_batch + postprocess_batch) of one box: the one-page batched kernels, page after page
  edit       pages     edit_pages(batch_size=4): full-size UNet / VAE with random weights, 512 px, T DDIM steps
             loop      P sequential single-box chains, the notebook's operating point: preprocess -> edit_latents -> postprocess per page
The results of the two sides are compared as well: prepost bit for bit, edit by the relative L2 distance of the decoder outputs.  No
threshold is applied: the model work of the two edit sides is that of scripts/bench_edit.py, so its ratio is the expectation."""
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


def box_for(i, h, w):
    """one word-sized box per page, at another place on every page; heights cycle so that the ladder gives crops of 128, 256, 384 and 512"""
    bh = (18, 40, 60, 80)[i % 4]
    x1, y1 = 60 + (i % 4) * 300, 80 + (i // 4) * 250 + (i % 4) * 7
    box = (x1, y1, x1 + 100 + 10 * (i % 3), y1 + bh)
    assert box[2] < w and box[3] < h
    return box


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--steps", type=int, default=50, help="DDIM steps of the edit timing")
    ap.add_argument("--edit-iters", type=int, default=2)
    ap.add_argument("--no-edit", action="store_true", help="pre/post-processing only (no models)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "edit_pages_line.json"))
    args = ap.parse_args()
    import diffute_amd as D
    from diffute_amd import prepost
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    h, w, S = 1100, 1300, 512
    res = dict(bench="edit_pages", page=[h, w], boxes_per_page=1, size=S, iters=args.iters, ddim_steps=args.steps, edit_iters=args.edit_iters)
    if not args.no_edit:
        unet = D.UNet2DConditionModel(device=dev).requires_grad_(False)
        vae = D.AutoencoderKL(device=dev).requires_grad_(False)
    for P in (4, 16):
        rs = np.random.RandomState(P)
        imgs = [torch.from_numpy(rs.randint(0, 256, (h, w, 3), dtype=np.uint8)).to(dev) for _ in range(P)]
        boxes = [[box_for(i, h, w)] for i in range(P)]
        plans = prepost.plan_pages(boxes, [(h, w)] * P, np.random.RandomState(1))
        origins, crops = [[p[:2] for p in pl] for pl in plans], [[p[2] for p in pl] for pl in plans]
        dec = (torch.randn(P, 3, S, S, generator=torch.Generator().manual_seed(5)) * 0.6).clamp(-1.3, 1.3).to(dev)
        outs = [torch.empty_like(img) for img in imgs]
        r = dict(crop_scales=[c[0] for c in crops])

        def paged():
            pre = prepost.preprocess_pages(imgs, boxes, origins, crops, size=S)
            return pre, prepost.postprocess_pages(dec, imgs, boxes, origins, crops, out=outs)

        def loop():
            pres, pages = [], []
            for p in range(P):
                pres.append(prepost.preprocess_batch(imgs[p], boxes[p], origins[p], crops[p], size=S))
            for p in range(P):
                pages.append(prepost.postprocess_batch(dec[p:p + 1], imgs[p], boxes[p], origins[p], crops[p]))
            return pres, pages

        (pb, ob), (pl, ol) = paged(), loop()
        r["prepost_bit_equal"] = bool(all(torch.equal(a, b) for a, b in zip(ob, ol)) and all(torch.equal(pb[k][p:p + 1], pl[p][k]) for p in range(P) for k in pb))
        r["prepost_pages_ms"] = round(timed(paged, args.iters, args.warmup), 4)
        r["prepost_loop_ms"] = round(timed(loop, args.iters, args.warmup), 4)
        r["prepost_loop_over_pages"] = round(r["prepost_loop_ms"] / r["prepost_pages_ms"], 2)
        if not args.no_edit:
            ctx = torch.randn(P, 577, 1024, generator=torch.Generator().manual_seed(2)).to(dev)
            noise = torch.randn(P, 4, S // 8, S // 8, generator=torch.Generator().manual_seed(3)).to(dev)
            init = torch.randn((1, 4, S // 8, S // 8), generator=torch.manual_seed(0), dtype=torch.float32).to(dev)
            kept = {}

            def edit_paged():
                kept["p"] = D.edit_pages(unet, vae, D.DDIMScheduler(), imgs, boxes, ctx, args.steps, origins=origins, crop_scales=crops, batch_size=4,
                                         enc_noise=noise, return_intermediate=True, size=S)

            def edit_loop():
                pages, vs = [], []
                for p in range(P):
                    (x_s, y_s), crop = origins[p][0], crops[p][0]
                    pre = prepost.preprocess(imgs[p], boxes[p][0], x_s, y_s, crop, size=S)
                    v = D.edit_latents(unet, vae, D.DDIMScheduler(), pre["image"], pre["masked_image"], pre["mask"], ctx[p:p + 1], args.steps,
                                       init_latents=init, enc_noise=noise[p:p + 1])
                    vs.append(v)
                    pages.append(prepost.postprocess(v, imgs[p], boxes[p][0], x_s, y_s, crop))
                kept["l"] = (pages, torch.cat(vs, 0))

            r["edit_pages_ms"] = round(timed(edit_paged, args.edit_iters, 1), 2)
            r["edit_loop_ms"] = round(timed(edit_loop, args.edit_iters, 1), 2)
            r["edit_loop_over_pages"] = round(r["edit_loop_ms"] / r["edit_pages_ms"], 3)
            r["edit_boxes_per_s_pages"] = round(P / r["edit_pages_ms"] * 1e3, 2)
            r["edit_boxes_per_s_loop"] = round(P / r["edit_loop_ms"] * 1e3, 2)
            vp, vl = kept["p"][1].float(), kept["l"][1].float()
            r["edit_image_vae_rel_l2"] = round(float((vp - vl).norm() / vl.norm()), 5)
        res[f"P{P}"] = r
    D.synchronize()
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
