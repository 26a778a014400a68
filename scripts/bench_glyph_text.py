"""Glyph stage per call, from strings to the processor's fp32 pixel_values on the GPU, three ways, same process, same box:

    python scripts/bench_glyph_text.py [--iters N] [--warmup W] [--rounds R]

  fused        GlyphRenderer.pixel_values(texts, processor): host layout, one H2D copy of the tables, ONE launch, no canvas in memory
  two_launch   the same with fused=False: dmx_glyph_render into device canvases + dmx_glyph_resize_normalize on them
  pil_host     what a caller does today: PIL draw_text on the CPU (the reference's canvas rule, BASIC layout) + diffute_amd.TrOCRProcessor
               with host images in (needs Pillow with FreeType; left out of the line if there is none)

Texts have lengths cycling through 1..20, batches of 1 / 8 / 16.  The atlas is the one of tests/golden/glyph_text.npz, so no font is
needed for the device paths.  Per path: the median over `rounds` windows of `iters` calls each (wall clock around a synchronise), the
three paths alternating round by round; per device path also the device-event time per call.  Prints one JSON line."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

ALPHABET = "abcdefghijklmnopqrstuvwxyz ABCDEFGHIJKLMNOPQRSTUVWXYZ 0123456789 .,:;/-#$%&()"


def window(fn, iters):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / iters * 1e3


def events(fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(iters):
        fn()
    b.record(); b.synchronize()
    return a.elapsed_time(b) / iters


def pil_font(atlas_size):
    """(name, font) - the fixture's font if it is installed, else Pillow's embedded one; (None, None) without Pillow + FreeType"""
    try:
        from PIL import ImageFont, features
        if not features.check("freetype2"):
            return None, None
        from glyph_text_cases import FONT_PATH
        if os.path.exists(FONT_PATH):
            return os.path.basename(FONT_PATH), ImageFont.truetype(FONT_PATH, atlas_size, layout_engine=ImageFont.Layout.BASIC)
        return "ImageFont.load_default", ImageFont.load_default(size=atlas_size)
    except Exception:
        return None, None


def pil_draw_text(font, text):
    from PIL import Image, ImageDraw
    img = Image.new("RGB", ((len(text) + 2) * 40, 60), (255, 255, 255))
    ImageDraw.Draw(img).text((40, 10), text, fill=(0, 0, 0), font=font)
    return np.asarray(img)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=7)
    args = ap.parse_args()
    import diffute_amd as D
    from glyph_text_cases import load_golden
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    atlas = D.GlyphAtlas.from_arrays(load_golden(), "atlas.")
    renderer = D.GlyphRenderer(atlas, dev)
    proc = D.TrOCRProcessor()
    font_name, font = pil_font(atlas.size)
    rng = np.random.RandomState(0)
    res = dict(bench="glyph_text", iters=args.iters, rounds=args.rounds, pil_font=font_name)
    for B in (1, 8, 16):
        lens = [(7 * i + 3) % 20 + 1 for i in range(B)]                         # text lengths spread over 1..20, as bench_glyph.py
        texts = ["".join(ALPHABET[j] for j in rng.randint(0, len(ALPHABET), n)) for n in lens]
        paths = {"fused": lambda: renderer.pixel_values(texts, proc, fused=True).pixel_values,
                 "two_launch": lambda: renderer.pixel_values(texts, proc, fused=False).pixel_values}
        if font is not None:
            paths["pil_host"] = lambda: proc(images=[pil_draw_text(font, t) for t in texts], return_tensors="pt").pixel_values
        r = dict(text_lengths=lens, out_bytes=B * 3 * 384 * 384 * 4)
        outs = {k: fn() for k, fn in paths.items()}
        D.synchronize()
        r["fused_bit_equal_to_two_launch"] = bool(torch.equal(outs["fused"], outs["two_launch"]))
        if font is not None and font_name != "ImageFont.load_default":         # (the embedded font is another font than the atlas's)
            r["fused_bit_equal_to_pil_host"] = bool(torch.equal(outs["fused"], outs["pil_host"]))
        iters = {k: (max(5, args.iters // 10) if k == "pil_host" else args.iters) for k in paths}
        for k, fn in paths.items():
            window(fn, args.warmup)
        times = {k: [] for k in paths}
        for _ in range(args.rounds):                                            # alternate the paths: the host is shared
            for k, fn in paths.items():
                times[k].append(window(fn, iters[k]))
        for k in paths:
            r[k + "_ms"] = round(statistics.median(times[k]), 4)
            r[k + "_ms_min_max"] = [round(min(times[k]), 4), round(max(times[k]), 4)]
        for k in ("fused", "two_launch"):
            r[k + "_event_ms"] = round(events(paths[k], args.iters), 4)
        r["two_launch_over_fused"] = round(r["two_launch_ms"] / r["fused_ms"], 3)
        if "pil_host_ms" in r:
            r["pil_host_over_fused"] = round(r["pil_host_ms"] / r["fused_ms"], 2)
        res[f"B{B}"] = r
    D.synchronize()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
