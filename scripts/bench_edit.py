"""Several text boxes of one image: the batched path (pipeline.edit_boxes over prepost.preprocess_batch / postprocess_batch) against
the single-box calls it replaces, same process, same box:

    python scripts/bench_edit.py [--iters N] [--warmup W] [--steps T] [--edit-iters N]

A 1100 x 1300 uint8 image, B boxes spread over it with the reference's crop ladder (crops of 128 .. 512).  Prints one JSON line; for
B = 4 and B = 16, ms per call (wall clock, synchronised):
  prepost    batched   one preprocess_batch + one postprocess_batch
             loop      B x (generate_mask + preprocess) + B chained postprocess, the single-box functions
  edit       batched   edit_boxes(batch_size=4): full-size UNet / VAE with random weights, 512 px, T DDIM steps
             loop      B sequential batch-1 edits: preprocess -> edit_latents -> postprocess per box, same scheduler and steps
The results of the two sides are compared as well: prepost bit for bit, edit by the relative L2 distance of the decoder outputs."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402


def timed(fn, iters, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / iters * 1e3


def boxes_for(B, h, w):
    """B word-sized boxes on a grid over the page; heights cycle so that the ladder gives crops of 128, 256, 384 and 512"""
    boxes = []
    for i in range(B):
        bh = (18, 40, 60, 80)[i % 4]
        x1 = 60 + (i % 4) * 300
        y1 = 80 + (i // 4) * 250 + (i % 4) * 7
        boxes.append((x1, y1, x1 + 100 + 10 * (i % 3), y1 + bh))
    assert all(x2 < w and y2 < h for _, _, x2, y2 in boxes)
    return boxes


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--steps", type=int, default=50, help="DDIM steps of the edit timing")
    ap.add_argument("--edit-iters", type=int, default=2)
    ap.add_argument("--no-edit", action="store_true", help="pre/post-processing only (no models)")
    args = ap.parse_args()
    import diffute_amd as D
    from diffute_amd import prepost
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    h, w, S = 1100, 1300, 512
    img = torch.from_numpy(np.random.RandomState(0).randint(0, 256, (h, w, 3), dtype=np.uint8)).to(dev)
    res = dict(bench="edit_boxes", image=[h, w], size=S, iters=args.iters, ddim_steps=args.steps, edit_iters=args.edit_iters)
    if not args.no_edit:
        unet = D.UNet2DConditionModel(device=dev).requires_grad_(False)
        vae = D.AutoencoderKL(device=dev).requires_grad_(False)
    for B in (4, 16):
        boxes = boxes_for(B, h, w)
        plans = prepost.plan_edits(boxes, h, w, np.random.RandomState(1))
        origins, crops = [p[:2] for p in plans], [p[2] for p in plans]
        g = torch.Generator().manual_seed(5)
        dec = (torch.randn(B, 3, S, S, generator=g) * 0.6).clamp(-1.3, 1.3).to(dev)
        r = dict(crop_scales=crops)

        def batched():
            pre = prepost.preprocess_batch(img, boxes, origins, crops, size=S)
            return pre, prepost.postprocess_batch(dec, img, boxes, origins, crops)

        def loop():
            pres, out = [], img
            for b in range(B):
                pres.append(prepost.preprocess(img, boxes[b], origins[b][0], origins[b][1], crops[b], size=S))     # includes its generate_mask
            for b in range(B):
                out = prepost.postprocess(dec[b:b + 1], out, boxes[b], origins[b][0], origins[b][1], crops[b])
            return pres, out

        (pb, ob), (pl, ol) = batched(), loop()
        r["prepost_bit_equal"] = bool(torch.equal(ob, ol) and all(torch.equal(pb[k][b:b + 1], pl[b][k]) for b in range(B) for k in pb))
        r["prepost_batched_ms"] = round(timed(batched, args.iters, args.warmup), 4)
        r["prepost_loop_ms"] = round(timed(loop, args.iters, args.warmup), 4)
        r["prepost_loop_over_batched"] = round(r["prepost_loop_ms"] / r["prepost_batched_ms"], 2)
        if not args.no_edit:
            ctx = torch.randn(B, 577, 1024, generator=torch.Generator().manual_seed(2)).to(dev)
            noise = torch.randn(B, 4, S // 8, S // 8, generator=torch.Generator().manual_seed(3)).to(dev)
            init = torch.randn((1, 4, S // 8, S // 8), generator=torch.manual_seed(0), dtype=torch.float32).to(dev)
            kept = {}

            def edit_batched():
                kept["b"] = D.edit_boxes(unet, vae, D.DDIMScheduler(), img, boxes, ctx, args.steps, origins=origins, crop_scales=crops,
                                         batch_size=4, enc_noise=noise, return_intermediate=True, size=S)

            def edit_loop():
                out, vs = img, []
                for b in range(B):
                    pre = prepost.preprocess(img, boxes[b], origins[b][0], origins[b][1], crops[b], size=S)
                    v = D.edit_latents(unet, vae, D.DDIMScheduler(), pre["image"], pre["masked_image"], pre["mask"], ctx[b:b + 1], args.steps,
                                       init_latents=init, enc_noise=noise[b:b + 1])
                    vs.append(v)
                    out = prepost.postprocess(v, out, boxes[b], origins[b][0], origins[b][1], crops[b])
                kept["l"] = (out, torch.cat(vs, 0))

            r["edit_batched_ms"] = round(timed(edit_batched, args.edit_iters, 1), 2)
            r["edit_loop_ms"] = round(timed(edit_loop, args.edit_iters, 1), 2)
            r["edit_loop_over_batched"] = round(r["edit_loop_ms"] / r["edit_batched_ms"], 3)
            r["edit_boxes_per_s_batched"] = round(B / r["edit_batched_ms"] * 1e3, 2)
            r["edit_boxes_per_s_loop"] = round(B / r["edit_loop_ms"] * 1e3, 2)
            vb, vl = kept["b"][1].float(), kept["l"][1].float()
            r["edit_image_vae_rel_l2"] = round(float((vb - vl).norm() / vl.norm()), 5)
        res[f"B{B}"] = r
    D.synchronize()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
