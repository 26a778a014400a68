"""The pages of tests/test_page_compose_*.py and scripts/make_page_compose_golden.py: (id, page) with a page in the form
tests/page_compose_restatement.py takes.  The atlas is the one of tests/golden/glyph_text.npz (DejaVu Sans, 40 px).  Between them the
pages hold what the composer can get wrong:

  inks        black, white, mid-grey and saturated inks over a textured background (a blend without its rounding term, or with two
              rounded products, differs at partial coverage);
  overlap_*   two lines of different ink across each other, in both orders (a maximum over lines, one coverage for all lines or the
              reverse order differ);
  kerned      "/\\", "AV", "To", "rn": pairs whose bitmaps overlap inside ONE line (a maximum inside the line differs);
  partly_off / wholly_off   a line hanging off, and one beyond, each of the four edges;
  clamp_*     backgrounds 0, 3, 252, 255 with tex_amp 0 and 6: both clamps of the textured background fire (a wrap differs);
  grid_*      widths one below, at and one above the block of 128 and at twice the block plus one, heights 1 and 61;
  many        24 lines - the most the dataset puts on a page - at a pitch of 7 rows, so every line runs over its neighbours;
  empty       no line at all."""
import os

import numpy as np

import glyph_text_cases as GC

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "page_compose.npz")
FONT_PATH, FONT_SIZE = GC.FONT_PATH, GC.FONT_SIZE
BLOCK = 128
MAX_LINES = 24

BLACK, WHITE, GREY, RED, BLUE, GREEN = (0, 0, 0), (255, 255, 255), (128, 128, 128), (255, 0, 0), (0, 0, 255), (0, 255, 0)


def page(size, bg, lines, tex_seed=0, tex_amp=0):
    return dict(size=tuple(size), bg=tuple(bg), tex_seed=int(tex_seed), tex_amp=int(tex_amp),
                lines=[dict(text=t, pen=tuple(p), ink=tuple(i)) for t, p, i in lines])


def _cases():
    out = [("empty", page((9, 130), (250, 248, 240), [], 1, 6)),
           ("inks", page((196, 257), (200, 190, 180), [("Black jg", (4, 0), BLACK), ("White To", (4, 46), WHITE), ("Grey AV", (4, 92), GREY),
                                                         ("Red", (4, 140), RED), ("Blue", (120, 140), BLUE)], 2, 6)),
           ("overlap_ab", page((70, 200), (240, 240, 230), [("AVATAR", (3, 2), RED), ("WWMM##", (10, 16), BLUE)], 3, 6)),
           ("overlap_ba", page((70, 200), (240, 240, 230), [("WWMM##", (10, 16), BLUE), ("AVATAR", (3, 2), RED)], 3, 6)),
           ("kerned", page((61, 300), (30, 30, 40), [("/\\AVToTorn/\\", (5, 5), (240, 230, 90))], 4, 6)),
           ("partly_off", page((120, 180), (230, 235, 240), [("jWleft", (-25, 30), BLACK), ("right jW", (100, 60), (90, 0, 120)),
                                                               ("top gjW", (40, -22), (0, 90, 30)), ("bottom", (30, 95), (120, 60, 0))], 5, 6)),
           ("wholly_off", page((50, 140), (225, 225, 225), [("in", (50, 2), BLACK), ("left", (-400, 5), RED), ("right", (141, 5), RED),
                                                              ("above", (20, -80), RED), ("below", (20, 51), RED)], 6, 0))]
    for bg in (0, 3, 252, 255):
        for amp in (0, 6):
            ink = WHITE if bg < 128 else BLACK
            out.append((f"clamp_{bg}_{amp}", page((20, 130), (bg, bg, bg), [("xo", (100, -14), ink)], 7 + bg, amp)))
    k = 0
    for H in (1, 61):
        for W in (BLOCK - 1, BLOCK, BLOCK + 1, 2 * BLOCK + 1):
            bg = ((250, 250, 245), (20, 25, 30), (255, 252, 3), (0, 3, 252))[k % 4]
            ink = (250, 240, 200) if k % 4 == 1 else (10, 20, 60)
            out.append((f"grid_{H}x{W}", page((H, W), bg, [("gjW#Qy", (W - 118, -20 if H == 1 else 6), ink)], 100 + k, 6)))
            k += 1
    inks = (BLACK, RED, BLUE, GREEN, GREY, (90, 0, 120))
    out.append(("many", page((200, 257), (245, 245, 235), [(f"L{i:02d} xyz", (3 + 5 * (i % 7), -8 + 7 * i), inks[i % 6]) for i in range(MAX_LINES)],
                             9, 6)))
    return out


CASES = _cases()
CASE_IDS = [c[0] for c in CASES]
BY_ID = dict(CASES)
# one ragged launch: no lines, one line, the dataset's maximum, pages of different sizes
RAGGED = ["empty", "grid_61x129", "many", "overlap_ab", "grid_1x257", "partly_off", "wholly_off", "clamp_0_6"]
assert len(BY_ID["many"]["lines"]) == MAX_LINES and not BY_ID["empty"]["lines"] and len(BY_ID["grid_61x129"]["lines"]) == 1


def load_golden():
    with np.load(GOLDEN, allow_pickle=False) as z:
        return {k: z[k] for k in z.files}


def load_atlas_arrays():
    return GC.load_golden()
