"""Writes tests/golden/glyph_text.npz: the size-40 printable-ASCII atlas of DejaVuSans (GlyphAtlas.arrays under "atlas."), Pillow's own
canvases - `ImageDraw.text` under the BASIC layout, one grey plane each, the three channels are equal - for the cases of
tests/glyph_text_cases.py, and the Pillow version.

    python scripts/make_glyph_text_golden.py        # needs Pillow with FreeType and the DejaVuSans font; the tests only need the file

Rasterised glyphs of a freely redistributable font: data, not program text."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from glyph_text_cases import CASES, FONT_PATH, FONT_SIZE, GOLDEN, canvas_size  # noqa: E402


def pil_draw_text(font, text, size, origin):
    """the reference's draw_text on an H x W canvas -> uint8 [H][W][3]"""
    from PIL import Image, ImageDraw
    H, W = size
    img = Image.new("RGB", (W, H), (255, 255, 255))
    ImageDraw.Draw(img).text(tuple(origin), text, fill=(0, 0, 0), font=font)
    return np.asarray(img)


def main():
    import PIL
    from PIL import ImageFont
    from diffute_amd.glyphs import GlyphAtlas
    font = ImageFont.truetype(FONT_PATH, FONT_SIZE, layout_engine=ImageFont.Layout.BASIC)
    data = GlyphAtlas.from_font(font, FONT_SIZE).arrays("atlas.")
    for name, text, size, origin in CASES:
        img = pil_draw_text(font, text, canvas_size(text, size), origin)
        assert np.array_equal(img[..., 0], img[..., 1]) and np.array_equal(img[..., 0], img[..., 2])
        data["canvas." + name] = np.ascontiguousarray(img[..., 0])
    data["versions"] = np.array([f"Pillow {PIL.__version__}", f"numpy {np.__version__}"])
    np.savez_compressed(GOLDEN, **data)
    size = os.path.getsize(GOLDEN)
    print(f"{GOLDEN}: {size} bytes, {len(CASES)} cases")
    if size > 384 * 1024:
        sys.exit("golden file larger than 384 KB")


if __name__ == "__main__":
    main()
