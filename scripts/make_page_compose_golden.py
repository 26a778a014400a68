#!/usr/bin/env python3
"""Writes tests/golden/page_compose.npz: the pages of tests/page_compose_cases.py as Pillow draws them - the background of the header's
hash rule as an image, then one ImageDraw.text(pen, text, font=font, fill=ink) per line under the BASIC layout.  The GPU machine then
needs neither Pillow nor the font.  The font is the one tests/golden/glyph_text.npz was rasterised from; the script refuses to write if
the atlas built here differs from that fixture, or if the numpy restatement (tests/page_compose_restatement.py) differs from Pillow on
any page.

  python scripts/make_page_compose_golden.py            # needs Pillow with FreeType and DejaVuSans.ttf"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import page_compose_cases as C          # noqa: E402
import page_compose_restatement as T    # noqa: E402


def pil_page(font, pg):
    """the page as Pillow draws it, uint8 [H][W][3]"""
    from PIL import Image, ImageDraw
    img = Image.fromarray(T.background(pg["size"], pg["bg"], pg["tex_seed"], pg["tex_amp"]), "RGB")
    draw = ImageDraw.Draw(img)
    for ln in pg["lines"]:
        draw.text(tuple(ln["pen"]), ln["text"], font=font, fill=tuple(ln["ink"]))
    return np.asarray(img).copy()


def main():
    import PIL
    from PIL import ImageFont
    from diffute_amd.glyphs import GlyphAtlas
    arrays = C.load_atlas_arrays()
    atlas = GlyphAtlas.from_arrays(arrays, "atlas.")
    built = GlyphAtlas.from_font(C.FONT_PATH, C.FONT_SIZE)
    for k in ("rec", "pool", "kern_pairs", "kern_values"):
        if not np.array_equal(getattr(built, k), getattr(atlas, k)):
            raise SystemExit(f"the atlas built from {C.FONT_PATH} differs from tests/golden/glyph_text.npz in {k}")
    font = ImageFont.truetype(C.FONT_PATH, C.FONT_SIZE, layout_engine=ImageFont.Layout.BASIC)
    out = {"versions": np.array(f"Pillow {PIL.__version__}, numpy {np.__version__}")}
    for name, pg in C.CASES:
        want = pil_page(font, pg)
        got = T.compose(atlas, pg)
        if not np.array_equal(got, want):
            raise SystemExit(f"{name}: the restatement differs from Pillow in {int((got != want).sum())} bytes")
        out["page." + name] = want
    np.savez_compressed(C.GOLDEN, **out)
    print(f"{C.GOLDEN}: {len(C.CASES)} pages, {os.path.getsize(C.GOLDEN)} bytes")


if __name__ == "__main__":
    main()
