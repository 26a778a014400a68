"""TrOCRProcessor per call: the device path (diffute_amd.TrOCRProcessor, one H2D copy + one HIP launch) against the host path the
reference runs (`processor(images=ttf_imgs, return_tensors="pt").pixel_values.cuda()`), same process, same box:

    python scripts/bench_glyph.py [--iters N] [--warmup W]

Glyph images are the reference draw_text's canvases, 60 x (len(text)+2)*40, text lengths cycling through 1..20.  Prints one JSON line:
per batch size ms per call (wall clock, synchronised) of
  device_host_in   uint8 numpy images on the host -> fp32 CUDA pixel_values
  device_gpu_in    the same images already on the GPU (read in place)
  host             transformers' ViTImageProcessorPil if importable, else PIL resize + numpy, including the upload of its fp32 pixel_values"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

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


def host_path():
    try:
        from transformers import ViTImageProcessorPil
        proc = ViTImageProcessorPil(do_resize=True, size={"height": 384, "width": 384}, resample=2, do_rescale=True, rescale_factor=1 / 255,
                                    do_normalize=True, image_mean=[0.5] * 3, image_std=[0.5] * 3)
        return "transformers ViTImageProcessorPil", lambda imgs: proc(images=imgs, return_tensors="pt").pixel_values
    except Exception:
        pass
    try:
        from PIL import Image
    except Exception:
        return None, None

    def run(imgs):
        out = [np.asarray(Image.fromarray(im).resize((384, 384), resample=2)).transpose(2, 0, 1) for im in imgs]
        x = (np.stack(out).astype(np.float64) * (1 / 255)).astype(np.float32)
        return torch.from_numpy((x - np.float32(0.5)) / np.float32(0.5))
    return "PIL + numpy", run


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    args = ap.parse_args()
    import diffute_amd as D
    from glyph_cases import make_input
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    proc = D.TrOCRProcessor()
    host_name, host = host_path()
    res = dict(bench="glyph_processor", host_impl=host_name, iters=args.iters)
    for B in (1, 8, 16):
        lens = [(7 * i + 3) % 20 + 1 for i in range(B)]                         # text lengths spread over 1..20
        imgs = [make_input(f"bench{n}", "glyph", (60, (n + 2) * 40)) for n in lens]
        gimgs = [torch.from_numpy(im).to(dev) for im in imgs]
        r = dict(text_lengths=lens, in_bytes=int(sum(im.nbytes for im in imgs)), out_bytes=B * 3 * 384 * 384 * 4)
        r["device_host_in_ms"] = round(timed(lambda: proc(images=imgs, return_tensors="pt").pixel_values, args.iters, args.warmup), 4)
        r["device_gpu_in_ms"] = round(timed(lambda: proc(images=gimgs, return_tensors="pt").pixel_values, args.iters, args.warmup), 4)
        if host is not None:
            ref = host(imgs)
            got = proc(images=imgs, return_tensors="pt").pixel_values
            r["bit_equal_to_host"] = bool(torch.equal(got.cpu(), ref))
            r["host_ms"] = round(timed(lambda: host(imgs).to(dev), max(5, args.iters // 5), 2), 4)
            r["host_over_device"] = round(r["host_ms"] / r["device_host_in_ms"], 2)
        # the kernel alone, by device events, on inputs already in HBM
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        for _ in range(args.iters):
            proc(images=gimgs, return_tensors="pt")
        b.record(); b.synchronize()
        r["device_gpu_in_event_ms"] = round(a.elapsed_time(b) / args.iters, 4)
        res[f"B{B}"] = r
    D.synchronize()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
