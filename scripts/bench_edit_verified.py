"""Verified edits: K candidates per text box, read back by the OCR model, the best-reading one pasted (pipeline.edit_boxes_verified),
with its stages timed one by one and against the unfused chain built from the functions that existed before it, same process:

    python scripts/bench_edit_verified.py [--steps T] [--iters N] [--stage-iters N] [--tokens T] [--out FILE]

Full-size UNet / VAE / TrOCR (large, 384 x 384) with random weights, 512 px, the 1100 x 1300 page of scripts/bench_edit.py, N = 4 boxes,
K = 1 / 2 / 4.  Prints one JSON line (and writes it to --out); per K, ms per call (wall clock around work that ends in a synchronise):
  total               edit_boxes_verified, everything
  denoise_decode      preprocess + VAE encode + denoise + VAE decode of the N*K rows (prepost.preprocess_batch + pipeline._candidate_rows)
  readback            prepost.readback_pixel_values: ONE launch                      | chain_readback: N*K postprocess + slice, one processor call
  encoder / score     ocr.encoder on the N*K pixel_values / the decoder's teacher-forced scoring pass on its states
  select_paste        prepost.postprocess_select_batch: ONE launch, no host sync     | chain_select_paste: scores to the host, arg-max there,
                                                                                       postprocess_batch of the chosen rows
Both sides' results are compared bit for bit.  Random weights: the scores mean nothing, no threshold is set, quality is not measured."""
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


def timed(fn, iters, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / iters * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=50, help="DDIM steps")
    ap.add_argument("--iters", type=int, default=2, help="timed calls of the whole function and of the denoise + decode stage")
    ap.add_argument("--stage-iters", type=int, default=30, help="timed calls of the small stages")
    ap.add_argument("--tokens", type=int, default=12, help="label length T")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import diffute_amd as D
    from diffute_amd import pipeline, prepost
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    h, w, S, N = 1100, 1300, 512, 4
    img = torch.from_numpy(np.random.RandomState(0).randint(0, 256, (h, w, 3), dtype=np.uint8)).to(dev)
    unet = D.UNet2DConditionModel(device=dev).requires_grad_(False)
    vae = D.AutoencoderKL(device=dev).requires_grad_(False)
    ocr = D.VisionEncoderDecoderModel(D.TrOCREncoder(device=dev), D.TrOCRForCausalLM(device=dev))
    proc = D.TrOCRProcessor()
    boxes = boxes_for(N, h, w)
    plans = prepost.plan_edits(boxes, h, w, np.random.RandomState(1))
    origins, crops = [p[:2] for p in plans], [p[2] for p in plans]
    ctx = torch.randn(N, 577, 1024, generator=torch.Generator().manual_seed(2)).to(dev)
    noise = torch.randn(N, 4, S // 8, S // 8, generator=torch.Generator().manual_seed(3)).to(dev)
    labels = torch.from_numpy(np.random.RandomState(4).randint(3, ocr.decoder.config.vocab_size, (N, args.tokens))).to(torch.int64)
    res = dict(bench="edit_boxes_verified", image=[h, w], size=S, boxes=N, crop_scales=crops, ddim_steps=args.steps, label_tokens=args.tokens,
               iters=args.iters, stage_iters=args.stage_iters, weights="random", quality="not measured")
    for K in (1, 2, 4):
        kept = {}

        def total():
            kept["r"] = D.edit_boxes_verified(unet, vae, D.DDIMScheduler(), ocr, proc, img, boxes, ctx, labels, args.steps, candidates=K,
                                              origins=origins, crop_scales=crops, enc_noise=noise, size=S, return_intermediate=True)

        def denoise_decode():
            pre = prepost.preprocess_batch(img, boxes, origins, crops, size=S)
            pipeline._candidate_rows(unet, vae, D.DDIMScheduler(), pre, dev, ctx, args.steps, list(range(K)), 4, None, noise, None, S)

        r = dict(total_ms=round(timed(total, args.iters, 1), 2), denoise_decode_ms=round(timed(denoise_decode, args.iters, 1), 2))
        v = kept["r"]
        lab = labels.to(dev).repeat_interleave(K, 0)

        def readback():
            kept["pv"] = prepost.readback_pixel_values(v.image_vae, img, boxes, origins, crops, proc)

        def chain_readback():
            slices = []
            for b, (x1, y1, x2, y2) in enumerate(boxes):
                for k in range(K):
                    slices.append(prepost.postprocess(v.image_vae[b, k], img, boxes[b], origins[b][0], origins[b][1], crops[b])[y1:y2, x1:x2])
            kept["cpv"] = proc(images=slices).pixel_values

        def encoder():
            kept["enc"] = ocr.encoder(v.pixel_values).last_hidden_state

        def score():
            kept["s"] = ocr.score(encoder_hidden_states=kept["enc"], labels=lab)

        def select_paste():
            kept["page"] = prepost.postprocess_select_batch(v.image_vae, v.scores, img, boxes, origins, crops)

        def chain_select_paste():
            c = np.nanargmax(v.scores.cpu().numpy(), 1)                                     # (no NaN here; the device rule is tests/' business)
            kept["cpage"] = prepost.postprocess_batch(v.image_vae[torch.arange(N), torch.from_numpy(c)], img, boxes, origins, crops)

        for name, fn in (("readback", readback), ("chain_readback", chain_readback), ("encoder", encoder), ("score", score),
                         ("select_paste", select_paste), ("chain_select_paste", chain_select_paste)):
            r[name + "_ms"] = round(timed(fn, args.stage_iters, 3), 4)
        r["chain_over_fused_readback"] = round(r["chain_readback_ms"] / r["readback_ms"], 2)
        r["chain_over_fused_select_paste"] = round(r["chain_select_paste_ms"] / r["select_paste_ms"], 2)
        r["readback_bit_equal"] = bool(torch.equal(kept["pv"], kept["cpv"]) and torch.equal(kept["pv"], v.pixel_values))
        r["page_bit_equal"] = bool(torch.equal(kept["page"][0], kept["cpage"]) and torch.equal(kept["page"][0], v.image))
        r["choice"] = v.choice.tolist()
        res[f"K{K}"] = r
    D.synchronize()
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
