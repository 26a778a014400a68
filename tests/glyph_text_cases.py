"""The cases of tests/test_glyph_text_*.py and scripts/make_glyph_text_golden.py: (id, text, (H, W) or None for the reference's canvas, origin).
Between them they hold what the compositing rule can get wrong: "/\\" overlaps (a maximum differs), "rn" kerns by -1/64 px and "AV" by
a few 1/64 px (a truncated pen differs; dropped kerning shows once the pairs add up to half a pixel: "ToToToToToTo"), descenders and punctuation, the widest reference canvas (20 characters: 880
columns), and "jW" on a canvas too small for it, so that glyphs are clipped on the left, right and bottom."""
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "glyph_text.npz")
FONT_PATH = "/usr/share/fonts/truetype/dejavu/DejaVuSans.ttf"      # the font the fixture was rasterised from (live-Pillow test only)
FONT_SIZE = 40
ORIGIN = (40, 10)

CASES = [
    ("empty", "", None, ORIGIN),
    ("one_letter", "a", None, ORIGIN),
    ("overlap", "/\\", None, ORIGIN),
    ("subpixel_kerning", "rn m", None, ORIGIN),
    ("kerning", "AVATAR To.", None, ORIGIN),
    ("descenders", "gjpqy,;_|", None, ORIGIN),
    ("len20", "Invoice #2024/07: $9", None, ORIGIN),
    ("clip_a", "jW", (50, 30), (0, 10)),                # 30 columns x 50 rows
    ("clip_b", "jW", (50, 30), (-3, 25)),
    ("kerning_chain", "ToToToToToTo", None, ORIGIN),
]
CASE_IDS = [c[0] for c in CASES]
BATCH = CASES[:8]                       # the ragged batch of B = 8
SINGLE = CASES[8:9]                     # clip_b goes through a B = 1 call
assert len(CASES[6][1]) == 20


def canvas_size(text, size):
    return tuple(size) if size is not None else (60, (len(text) + 2) * 40)


def load_golden():
    with np.load(GOLDEN, allow_pickle=False) as z:
        return {k: z[k] for k in z.files}


def rgb(grey):
    """one grey plane [H][W] -> the canvas [H][W][3]"""
    return np.ascontiguousarray(np.repeat(grey[:, :, None], 3, axis=2))
