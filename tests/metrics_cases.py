"""The inputs of the metrics tests (test_metrics_host.py, test_metrics_gpu.py): two pages of different sizes, box tables at the smallest
shapes at which csrc/metrics.hip can go wrong, five kinds of content.  Everything is generated from seeds; nothing here needs a GPU.

A tile is TILE = 16 window centres a side and reads TILE + 10 = 26 pixels a side, so 25 / 26 / 27 are the sizes around the first tile edge."""
import numpy as np

from metrics_restatement import TILE, WIN

SIZES = [(37, 53), (64, 150)]                       # (H, W) of page 0 and page 1
E = TILE + WIN - 1                                  # 26: the largest box of one tile

# boxes are (x1, y1, x2, y2), exclusive upper corner; per page
MAIN = [
    [   # page 0, 37 x 53
        (0, 0, 11, 11),                             # one window; the top-left corner
        (42, 0, 53, 12),                            # 12 x 11 (h x w); the top-right corner
        (0, 26, 12, 37),                            # 11 x 12; the bottom-left corner
        (42, 25, 53, 37),                           # the bottom-right corner
        (0, 0, 53, 37),                             # the whole page: 3 tiles in x, 2 in y
        (5, 3, 35, 13),                             # 10 x 30: no window (NaN)
        (7, 2, 17, 32),                             # 30 x 10: no window (NaN)
        (20, 20, 21, 21),                           # 1 x 1
    ],
    [   # page 1, 64 x 150
        (3, 2, 3 + E - 1, 2 + E),                   # widths 25 / 26 / 27 at height 26
        (30, 2, 30 + E, 2 + E),
        (60, 2, 60 + E + 1, 2 + E),
        (90, 1, 90 + E, 1 + E - 1),                 # heights 25 / 27 at width 26
        (90, 30, 90 + E, 30 + E + 1),
        (10, 30, 55, 60),                           # 45 x 30: 3 tiles in x, 2 in y, none of them full
        (60, 30, 90, 55), (75, 40, 110, 64),        # two overlapping boxes
        (118, 35, 148, 60), (118, 35, 148, 60),     # two identical boxes
        (139, 53, 150, 64),                         # the bottom-right corner, one window
        (0, 0, 150, 64),                            # the whole page
    ],
]
ONE = [[], [(30, 2, 30 + E, 2 + E)]]                # B = 1, and a page without boxes


def _many(seed=5, counts=(40, 25)):
    """B = 65, past the 64 mark of the edit tables: small seeded boxes, some too small for a window"""
    rs = np.random.RandomState(seed)
    out = []
    for (H, W), n in zip(SIZES, counts):
        boxes = []
        for _ in range(n):
            w, h = int(rs.randint(1, 30)), int(rs.randint(1, 30))
            x1, y1 = int(rs.randint(0, W - w + 1)), int(rs.randint(0, H - h + 1))
            boxes.append((x1, y1, x1 + w, y1 + h))
        out.append(boxes)
    return out


GEOMETRY = {"main": MAIN, "one": ONE, "b65": _many()}
CONTENTS = ("noise", "page", "same", "flat", "pixel")
PIXEL = [(5, 5), (80, 45)]                          # (x, y) of the one changed pixel of `pixel`, per page
REDRAWN = [(10, 8, 40, 30), (60, 30, 110, 60)]      # the region of `page` that b draws again, per page
CASES = [(f"{c}/main", c, "main") for c in CONTENTS] + [("noise/one", "noise", "one"), ("noise/b65", "noise", "b65"), ("page/b65", "page", "b65")]


def _strokes(img, rs, region, n):
    """n dark horizontal / vertical strokes, 1 - 2 pixels wide, inside region (x1, y1, x2, y2)"""
    x1, y1, x2, y2 = region
    for _ in range(n):
        v = rs.randint(20, 90, 3)
        t = int(rs.randint(1, 3))
        if rs.randint(2):
            y, xa, xb = int(rs.randint(y1, y2 - t + 1)), *sorted(int(u) for u in rs.randint(x1, x2 + 1, 2))
            img[y:y + t, xa:xb + 1] = v
        else:
            x, ya, yb = int(rs.randint(x1, x2 - t + 1)), *sorted(int(u) for u in rs.randint(y1, y2 + 1, 2))
            img[ya:yb + 1, x:x + t] = v


def pair(content, page):
    """the two versions (a, b) of page `page` with the given content: uint8 [H][W][3]"""
    H, W = SIZES[page]
    rs = np.random.RandomState(100 * CONTENTS.index(content) + page)
    if content in ("noise", "same"):
        a = rs.randint(0, 256, (H, W, 3)).astype(np.uint8)
        b = a.copy() if content == "same" else np.clip(a.astype(np.int64) + rs.randint(-20, 21, (H, W, 3)), 0, 255).astype(np.uint8)
    elif content == "page":                          # a document: white, dark strokes; b draws one region again
        a = np.full((H, W, 3), 255, dtype=np.uint8)
        _strokes(a, rs, (0, 0, W, H), 30)
        b = a.copy()
        x1, y1, x2, y2 = REDRAWN[page]
        b[y1:y2, x1:x2] = 255
        _strokes(b, rs, (x1, y1, x2 - 1, y2 - 1), 12)
    else:
        a = np.full((H, W, 3), 255, dtype=np.uint8)
        b = a.copy()
        if content == "flat":
            b[:] = 253
        else:
            x, y = PIXEL[page]
            b[y, x] = 254
    return a, b


def pages(content):
    """([a_0, a_1], [b_0, b_1])"""
    ps = [pair(content, p) for p in range(len(SIZES))]
    return [p[0] for p in ps], [p[1] for p in ps]


def flat_boxes(geometry):
    """[(page, box)] page-major, the order of the kernel's rows"""
    return [(p, bx) for p, boxes in enumerate(GEOMETRY[geometry]) for bx in boxes]


def measure(content, geometry):
    """per box and channel, |eval32 - ref64| of the SSIM: the floor of the fp32 formulation (0 where the box has no window)"""
    import metrics_restatement as M
    A, Bp = pages(content)
    out = []
    for p, bx in flat_boxes(geometry):
        ref, got = M.ref64(A[p], Bp[p], bx)["ssim"], M.eval32(A[p], Bp[p], bx)
        out.append([0.0 if np.isnan(r) else abs(float(g) - float(r)) for g, r in zip(got, ref)])
    return out


if __name__ == "__main__":                          # regenerate metrics_floors.py: python tests/metrics_cases.py > tests/metrics_floors.py
    print('"""Measured error of the fp32 formulation of the SSIM (metrics_restatement.eval32) against float64 (ref64), per case, box and channel, on the\n'
          'CPU: the bound of test_metrics_gpu.py is metrics_restatement.bound(floor); test_metrics_host.py measures the figures again.\n'
          'Regenerate: python tests/metrics_cases.py > tests/metrics_floors.py"""')
    print("FLOORS = {")
    for name, content, geometry in CASES:
        print(f'    "{name}": [')
        for row in measure(content, geometry):
            print("        [" + ", ".join(f"{v:.3e}" for v in row) + "],")
        print("    ],")
    print("}")
