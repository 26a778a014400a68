"""numpy statement of what `ImageDraw.text(origin, text, fill=black)` writes on a white canvas under Pillow's BASIC layout, from glyph
data alone (bitmaps, offsets, advances and pair kernings in 1/64 px) - independent of diffute_amd.glyphs:

  pen position in 1/64 px: before a glyph the kerning of (previous, this) is added, after it the glyph's advance;
  a glyph's bitmap pixel (x0, y0) lands in column floor((pen + 32) / 64) + left + x0 and row top + y0, relative to the origin;
  coverage is composed in text order, m = s + round(m * (255 - s) / 255); the canvas byte is 255 - m in every channel;
  whatever leaves the canvas is clipped.

`fault` injects one deliberate error ("max": composite by maximum; "no_kerning"; "truncate": floor(pen / 64)), for the test that shows
the case list can see each of them."""
import numpy as np


def place(atlas, text, origin=(40, 10), fault=None):
    """[(glyph index, x, y)] - atlas: anything with .chars, .rec [G,6] = (offset, w, h, left, top, advance), .kern_pairs, .kern_values"""
    index = {c: i for i, c in enumerate(atlas.chars)}
    kern = {(int(a), int(b)): int(v) for (a, b), v in zip(atlas.kern_pairs, atlas.kern_values)}
    out, pen, prev = [], 0, None
    for ch in text:
        g = index[ch]
        _, w, h, left, top, adv = (int(v) for v in atlas.rec[g])
        if prev is not None and fault != "no_kerning":
            pen += kern.get((prev, g), 0)
        px = pen // 64 if fault == "truncate" else (pen + 32) // 64
        out.append((g, int(origin[0]) + px + left, int(origin[1]) + top))
        pen += adv
        prev = g
    return out


def draw_text_grey(atlas, text, size=None, origin=(40, 10), fault=None):
    """uint8 [H][W]: one channel of the canvas (the three are equal)"""
    H, W = size if size is not None else (60, (len(text) + 2) * 40)
    m = np.zeros((H, W), dtype=np.int64)
    for g, x, y in place(atlas, text, origin, fault):
        off, w, h = (int(v) for v in atlas.rec[g, :3])
        a = np.asarray(atlas.pool[off:off + w * h], dtype=np.int64).reshape(h, w)
        x0, y0, x1, y1 = max(x, 0), max(y, 0), min(x + w, W), min(y + h, H)
        if x1 <= x0 or y1 <= y0:
            continue
        s = a[y0 - y:y1 - y, x0 - x:x1 - x]
        d = m[y0:y1, x0:x1]
        if fault == "max":
            m[y0:y1, x0:x1] = np.maximum(d, s)
        else:
            m[y0:y1, x0:x1] = s + (2 * d * (255 - s) + 255) // 510          # round half up of d * (255 - s) / 255
    return (255 - m).astype(np.uint8)


def draw_text(atlas, text, size=None, origin=(40, 10)):
    """uint8 [H][W][3]"""
    return np.repeat(draw_text_grey(atlas, text, size, origin)[:, :, None], 3, axis=2)
