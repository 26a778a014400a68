"""The cases of the TrOCRProcessor tests (tests/test_glyph_processor_host.py, tests/test_glyph_processor_gpu.py) and their seeded inputs;
scripts/make_glyph_golden.py records Pillow's and transformers' results for them in tests/golden/glyph_processor.npz.  Inputs are not
stored where a seed regenerates them: the golden keeps a CRC32 of each instead."""
import os
import zlib

import numpy as np

BILINEAR, BICUBIC = 2, 3
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "glyph_processor.npz")

# name, kind, (H, W), (out_h, out_w), resample.  Glyph canvases are the reference draw_text's 60 x (len(text) + 2) * 40.
CASES = [
    ("glyph_len3", "glyph", (60, 200), (384, 384), BILINEAR),                # both axes up
    ("glyph_len12", "glyph", (60, 560), (384, 384), BILINEAR),               # horizontal down 1.46x
    ("glyph_len40", "glyph", (60, 1680), (384, 384), BILINEAR),              # 11 taps
    ("noise_37x181", "sparse", (37, 181), (384, 384), BILINEAR),             # arbitrary source size
    ("noise_500x700", "blocks", (500, 700), (96, 96), BILINEAR),             # both axes down 5-7x
    ("identity_384", "glyph", (384, 384), (384, 384), BILINEAR),             # both passes skipped
    ("tiny_1x1", "noise", (1, 1), (8, 8), BILINEAR),                         # degenerate sizes
    ("tiny_2x3", "noise", (2, 3), (5, 7), BILINEAR),
    ("glyph_len3_bicubic", "glyph", (60, 200), (384, 384), BICUBIC),         # negative taps, clip8 at 0 and 255
    ("noise_500x700_bicubic", "blocks", (500, 700), (96, 96), BICUBIC),
]
CASE_IDS = [c[0] for c in CASES]
MIXED_BATCH = [c[0] for c in CASES if c[3] == (384, 384) and c[4] == BILINEAR]      # every bilinear 384-target case in one call


def make_input(name, kind, hw):
    """uint8 [H][W][3]; numpy's legacy RandomState streams are frozen, so a name reproduces its image"""
    h, w = hw
    rng = np.random.RandomState(sum(map(ord, name.replace("_bicubic", ""))))
    if kind == "noise":
        return rng.randint(0, 256, (h, w, 3), dtype=np.uint8)
    if kind == "blocks":                       # dense noise; a third of its 25 x 25 blocks saturated to 0 or 255, so that a bicubic
        img = rng.randint(0, 256, (h, w, 3), dtype=np.uint8)          # downscale overshoots both ends of the byte range at block edges
        for y in range(0, h, 25):
            for x in range(0, w, 25):
                u = rng.rand()
                if u < 1 / 3:
                    img[y:y + 25, x:x + 25] = 0 if u < 1 / 6 else 255
        return img
    img = np.full((h, w, 3), 255, dtype=np.uint8)
    if kind == "sparse":                       # white ground, 2 % of the pixels one of four dark / saturated colours
        pal = np.array([[0, 0, 0], [255, 0, 0], [0, 0, 255], [40, 40, 40]], dtype=np.uint8)
        m = rng.rand(h, w) < 0.02
        img[m] = pal[rng.randint(0, 4, int(m.sum()))]
        return img
    for x0 in range(40, w - 40, 40):           # one "character" per 40-px cell: two to four black bars, 2-5 px wide (E, H, L, T ...)
        for _ in range(rng.randint(2, 5)):
            t = int(rng.randint(2, 6))
            if rng.rand() < 0.5:
                y = int(rng.randint(8, h - 8 - t)); a, b = sorted(rng.randint(4, 36, 2)); img[y:y + t, x0 + a:x0 + b + 1] = 0
            else:
                x = x0 + int(rng.randint(4, 36 - t)); a, b = sorted(rng.randint(8, h - 8, 2)); img[a:b + 1, x:x + t] = 0
    return img


def crc(a):
    return zlib.crc32(np.ascontiguousarray(a).tobytes())


def load_golden():
    return np.load(GOLDEN)


def case_input(golden, case):
    name, kind, hw, _, _ = case
    img = make_input(name, kind, hw)
    assert crc(img) == int(golden[name + ".input_crc"]), f"{name}: the seeded input differs from the one the golden was made from"
    return img
