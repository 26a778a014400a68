"""Synthetic document pages per call: P pages of 1100 x 1300 with 16 lines each, same process, same box:

    python scripts/bench_synthetic_pages.py [--iters N] [--warmup W] [--rounds R] [--out profiles/synthetic_pages_line.json]

  compose      SyntheticDocuments.compose(records): host layout of the tables, one H2D copy, ONE dmx_page_compose launch
  batch        compose + sample_boxes + training_batch (the 256 -> 512 crop of one box per page, and its glyph context through the
               full-size TrOCR encoder with random weights): everything train_step needs from the records
  pil_host     the same pages on the CPU - the noise background as a numpy array, ImageDraw.text per line - plus the upload of the
               uint8 pages (needs Pillow with FreeType and the atlas's font; left out of the line otherwise)

The records are laid out before the clock starts (ds[i] is host work a loader does ahead of time; its time per page is reported on its
own).  Per path: the median over `rounds` windows of `iters` calls each, wall clock around a synchronise, after `warmup` calls; the paths
alternate round by round.  Prints one JSON line and writes it to --out.  `train_step_ms` is the 84.9 ms training step (README, batch 8)
this stage has to stay hidden behind."""
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

TRAIN_STEP_MS = 84.9


def window(fn, iters):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / iters * 1e3


def pil_font(size):
    try:
        from PIL import ImageFont, features
        from glyph_text_cases import FONT_PATH
        if features.check("freetype2") and os.path.exists(FONT_PATH):
            return ImageFont.truetype(FONT_PATH, size, layout_engine=ImageFont.Layout.BASIC)
    except Exception:
        pass
    return None


def pil_pages(font, records, backgrounds, dev):
    from PIL import Image, ImageDraw
    out = []
    for r, bg in zip(records, backgrounds):
        img = Image.fromarray(bg.copy(), "RGB")
        draw = ImageDraw.Draw(img)
        for ln in r["lines"]:
            draw.text(tuple(ln["pen"]), ln["text"], font=font, fill=tuple(ln["ink"]))
        out.append(torch.from_numpy(np.asarray(img).copy()).to(dev))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "synthetic_pages_line.json"))
    args = ap.parse_args()
    import diffute_amd as D
    from glyph_text_cases import load_golden
    import page_compose_restatement as T
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    atlas = D.GlyphAtlas.from_arrays(load_golden(), "atlas.")
    renderer = D.GlyphRenderer(atlas, dev)
    ds = D.SyntheticDocuments(renderer, page_size=(1100, 1300), lines=(16, 16), seed=0)
    enc = D.TrOCREncoder(device=dev)
    glyph = (renderer, D.TrOCRProcessor(), enc)
    font = pil_font(atlas.size)
    res = dict(bench="synthetic_pages", page=[1100, 1300], iters=args.iters, rounds=args.rounds, train_step_ms=TRAIN_STEP_MS,
               pil=font is not None)
    for P in (1, 8, 32):
        t0 = time.perf_counter()
        records = [ds[i] for i in range(P)]
        r = dict(lines_per_page=round(sum(len(x["lines"]) for x in records) / P, 2), layout_ms_per_page=round((time.perf_counter() - t0) / P * 1e3, 3),
                 page_bytes=P * 1100 * 1300 * 3)
        rng = np.random.default_rng(0)

        def batch():
            pages = ds.compose(records)
            return D.training_batch(pages, *D.sample_boxes(records, rng), glyph)

        paths = {"compose": lambda: ds.compose(records), "batch": batch}
        if font is not None:
            backgrounds = [T.background(x["size"], x["bg"], x["tex_seed"], x["tex_amp"]) for x in records]
            paths["pil_host"] = lambda: pil_pages(font, records, backgrounds, dev)
            got, want = paths["compose"](), paths["pil_host"]()
            D.synchronize()
            r["compose_bit_equal_to_pil_host"] = all(bool(torch.equal(a, b)) for a, b in zip(got, want))
        iters = {k: (max(2, args.iters // (4 if P > 1 else 2)) if k != "compose" else args.iters) for k in paths}
        for k, fn in paths.items():
            window(fn, args.warmup)
        times = {k: [] for k in paths}
        for _ in range(args.rounds):                                            # alternate the paths: the host is shared
            for k, fn in paths.items():
                times[k].append(window(fn, iters[k]))
        for k in paths:
            r[k + "_ms"] = round(statistics.median(times[k]), 4)
            r[k + "_ms_min_max"] = [round(min(times[k]), 4), round(max(times[k]), 4)]
        r["batch_over_train_step"] = round(r["batch_ms"] / TRAIN_STEP_MS, 3)
        if "pil_host_ms" in r:
            r["pil_host_over_compose"] = round(r["pil_host_ms"] / r["compose_ms"], 2)
        res[f"P{P}"] = r
    D.synchronize()
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
