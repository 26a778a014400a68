"""numpy statement of what dmx_page_compose writes (include/diffute_hip.h), from the header comment and glyph data alone - independent of
diffute_amd.data and of the kernel:

  background  byte (y, x, c) = clip8(bg[c] + off), off = h % (2 * tex_amp + 1) - tex_amp, with the 32-bit hash (mod 2^32)
                h = tex_seed + 0x9E3779B1 * y + 0x85EBCA77 * x + 0xC2B2AE3D * c
                h ^= h >> 16;  h *= 0x7FEB352D;  h ^= h >> 15;  h *= 0x846CA68B;  h ^= h >> 16
  lines       in order: m = the line's coverage (tests/glyph_text_restatement.py: placements composed in text order), then per channel
                v = round((v * (255 - m) + ink[c] * m) / 255),  round half up, one rounding of the sum
              which is Pillow's masked fill: ImageDraw.text(pen, text, font=font, fill=ink) on an RGB image under the BASIC layout.

A page is a dict: size (H, W), bg (r, g, b), tex_seed, tex_amp, lines [dict(text, pen (x, y), ink (r, g, b))].

`fault` injects one deliberate error, for the test that shows the case list can see each of them: "max" (a line's coverage by maximum),
"merged" (all lines composed into one coverage, blended once with the last line's ink), "no_round" (the blend without its rounding
term), "reverse" (lines drawn last to first), "tex_wrap" (the textured background wraps modulo 256 instead of being clamped), "two_round"
(two rounded products instead of one rounding of the sum)."""
import numpy as np

import glyph_text_restatement as T

FAULTS = ("max", "merged", "no_round", "reverse", "tex_wrap", "two_round")


def tex_hash(seed, y, x, c):
    """uint32 arrays (broadcast) -> uint32"""
    with np.errstate(over="ignore"):
        h = (np.uint32(seed) + np.uint32(0x9E3779B1) * y.astype(np.uint32) + np.uint32(0x85EBCA77) * x.astype(np.uint32)
             + np.uint32(0xC2B2AE3D) * c.astype(np.uint32))
        h ^= h >> np.uint32(16); h *= np.uint32(0x7FEB352D)
        h ^= h >> np.uint32(15); h *= np.uint32(0x846CA68B)
        h ^= h >> np.uint32(16)
    return h


def background(size, bg, tex_seed=0, tex_amp=0, fault=None):
    """uint8 [H][W][3]"""
    H, W = size
    v = np.broadcast_to(np.asarray(bg, dtype=np.int64).reshape(1, 1, 3), (H, W, 3)).copy()
    if tex_amp:
        y, x, c = np.meshgrid(np.arange(H, dtype=np.uint32), np.arange(W, dtype=np.uint32), np.arange(3, dtype=np.uint32), indexing="ij")
        v += (tex_hash(tex_seed, y, x, c) % np.uint32(2 * tex_amp + 1)).astype(np.int64) - tex_amp
    return (v % 256 if fault == "tex_wrap" else np.clip(v, 0, 255)).astype(np.uint8)


def line_coverage(atlas, line, size, fault=None):
    """int64 [H][W] in 0 .. 255"""
    return 255 - T.draw_text_grey(atlas, line["text"], size, line["pen"], fault="max" if fault == "max" else None).astype(np.int64)


def blend(v, m, ink, fault=None):
    """v int64 [H][W][3], m int64 [H][W], ink (r, g, b) -> int64 [H][W][3]"""
    m = m[:, :, None]
    ink = np.asarray(ink, dtype=np.int64).reshape(1, 1, 3)
    if fault == "no_round":
        return (v * (255 - m) + ink * m) // 255
    if fault == "two_round":
        return (2 * v * (255 - m) + 255) // 510 + (2 * ink * m + 255) // 510
    return (2 * (v * (255 - m) + ink * m) + 255) // 510                      # round half up of t / 255


def compose(atlas, page, fault=None):
    """uint8 [H][W][3]"""
    size = tuple(int(s) for s in page["size"])
    v = background(size, page["bg"], page.get("tex_seed", 0), page.get("tex_amp", 0), fault).astype(np.int64)
    lines = list(page["lines"])
    if fault == "reverse":
        lines = lines[::-1]
    if fault == "merged" and lines:
        m = np.zeros(size, dtype=np.int64)
        for ln in lines:
            s = line_coverage(atlas, ln, size)
            m = s + (2 * m * (255 - s) + 255) // 510
        return blend(v, m, lines[-1]["ink"]).astype(np.uint8)
    for ln in lines:
        v = blend(v, line_coverage(atlas, ln, size, fault), ln["ink"], fault)
    return v.astype(np.uint8)
