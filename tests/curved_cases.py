"""The pages, polygons and frames shared by tests/test_prepost_curved_host.py and tests/test_prepost_curved_gpu.py, and the ctypes tables
built from them.  Three small pages, nine polygons in one launch, n in {2, 3, 4, 7, 17}.  A polygon is 2n points: the top points as
read, then the bottom points backwards; a frame is (ci2, cj2, crop_scale) in the straightened strip's pixel-index space."""
import math

S = 64
SIZES = (32, 64)                                      # the crop sizes the kernels are compared at
PAGES = [(160, 200), (120, 150), (100, 180)]          # h x w

CENTRE = None                                         # the frame's centre = the strip's centre (rw - 1, rh - 1)


def arc(cx, cy, r_in, r_out, deg0, deg1, n):
    """an annular sector as 2n points: the outer arc from deg0 to deg1 (y down: increasing angles run clockwise), the inner arc back"""
    ang = [math.radians(deg0 + (deg1 - deg0) * k / (n - 1)) for k in range(n)]
    top = [(int(round(cx + r_out * math.cos(a))), int(round(cy + r_out * math.sin(a)))) for a in ang]
    bot = [(int(round(cx + r_in * math.cos(a))), int(round(cy + r_in * math.sin(a)))) for a in ang]
    return top + bot[::-1]


def box(x1, y1, x2, y2):
    return [(x1, y1), (x2, y1), (x2, y2), (x1, y2)]


# per page: name, points, crop_scale, centre (ci2, cj2) or CENTRE
ITEMS = [
    [("arc90", arc(100, 150, 60, 80, 225, 315, 7), 128, CENTRE),                                         # n = 7: 90 degrees in six cells
     ("overlap", [(70, 66), (130, 72), (128, 90), (68, 84)], 80, CENTRE),                               # n = 2, over arc90's crown: the later one decides
     ("s_bend", [(10, 20), (40, 10), (70, 26), (100, 14), (101, 32), (70, 44), (40, 28), (11, 38)], 110, CENTRE),      # n = 4
     ("border", [(0, 0), (30, 0), (60, 4), (60, 16), (30, 12), (0, 12)], 90, CENTRE)],                  # n = 3, on the page's corner
    [("arc270", arc(75, 60, 30, 50, 135, 405, 17), 200, CENTRE),                                        # n = 17: 270 degrees in sixteen cells
     ("downwards", [(146, 10), (148, 50), (146, 100), (132, 100), (134, 50), (132, 10)], 100, CENTRE)],  # n = 3, read top to bottom
    [("two_rows", [(10, 10), (40, 11), (70, 10), (70, 11), (40, 12), (10, 11)], 64, CENTRE),             # rh = 2
     ("one_column", [(20, 40), (60, 40), (61, 40), (100, 44), (100, 62), (61, 58), (60, 58), (20, 58)], 96, CENTRE),   # n = 4, w_1 = 1
     ("overhang", [(120, 80), (175, 84), (175, 96), (120, 92)], 100, CENTRE)],                          # n = 2, a parallelogram: a 100-pixel window at a 100-row page's corner
]
FLAT = [(p, it) for p, items in enumerate(ITEMS) for it in items]
N = len(FLAT)
CELLS = sum(len(it[1]) // 2 - 1 for _, it in FLAT)

# a parallelogram, its top edge (60, 80) long, whole and cut at whole-number cell lengths
PARA = [(20, 10), (80, 90), (68, 99), (8, 19)]
PARA_CUT = [(20, 10), (38, 34), (56, 58), (80, 90), (68, 99), (44, 67), (26, 43), (8, 19)]
PARA_PAGE = (120, 100)

# refused polygons (on page 0)
ODD = [(10, 10), (40, 10), (40, 30), (25, 32), (10, 30)]
FAN = [(10, 10), (40, 10), (70, 10), (70, 30), (40, 10), (10, 30)]              # a repeated point: cell 0 is the triangle's fan, not convex
CONCAVE = [(10, 10), (40, 30), (70, 10), (70, 20), (40, 25), (10, 20)]          # the bottom of cell 1 crosses over its top
COUNTER = [(10, 30), (40, 30), (40, 10), (10, 10)]                              # counter-clockwise
FLAT_STRIP = [(20, 20), (120, 20), (120, 20), (20, 21)]                         # mean segment length 1 / 2: rh = rn(0.5) + 1 = 1
OUTSIDE = [(150, 20), (200, 20), (200, 40), (150, 40)]                          # x = 200 on a 200-column page


def strip_size(points):
    import curved_restatement as CR
    rw, rh, _ = CR.strip(points)
    return rw, rh


def frame_of(points, crop_scale, centre=CENTRE):
    rw, rh = strip_size(points)
    ci2, cj2 = (rw - 1, rh - 1) if centre is None else centre
    return (ci2, cj2, crop_scale)


def lists():
    """(polygons, frames) as the prepost functions take them: P lists each"""
    polygons = [[it[1] for it in items] for items in ITEMS]
    frames = [[frame_of(it[1], it[2], it[3]) for it in items] for items in ITEMS]
    return polygons, frames


def tables(sizes, polygons, frames, original=64, out=128):
    """ctypes tables with dummy addresses: (dmx_edit_page * P, dmx_edit_curved * B, dmx_curved_piece * NP)"""
    from diffute_amd import _cabi
    B = sum(len(q) for q in polygons)
    NP = sum(len(c) - 2 for q in polygons for c in q)
    pt, ct, xt = (_cabi.EditPage * len(sizes))(), (_cabi.EditCurved * max(B, 1))(), (_cabi.CurvedPiece * max(NP, 1))()
    lo = 0
    for p, ((h, w), qs, fs) in enumerate(zip(sizes, polygons, frames)):
        pt[p].original, pt[p].out, pt[p].H, pt[p].W, pt[p].item_lo, pt[p].item_hi = original, out, h, w, lo, lo + len(qs)
        for it, c, f in zip(ct[lo:lo + len(qs)], qs, fs):
            for k, (x, y) in enumerate(c[:34]):                         # (a longer polygon is refused by its count)
                it.x[k], it.y[k] = int(x), int(y)
            it.count, it.page = len(c), p
            if f is not None:
                it.ci2, it.cj2, it.crop_scale = f
        lo += len(qs)
    return pt, ct, xt


# ---- straightening: the page's value is a linear ramp in the distance r from RAMP_CENTRE, the region arc90's band in M = 6 cells
RAMP_PAGE, RAMP_CENTRE, RAMP_SLOPE = (160, 200), (100, 150), 2.0
RAMP_R_IN, RAMP_R_OUT, RAMP_DEG, RAMP_M = 60, 80, (225, 315), 6
RAMP_ARC = arc(RAMP_CENTRE[0], RAMP_CENTRE[1], RAMP_R_IN, RAMP_R_OUT, RAMP_DEG[0], RAMP_DEG[1], RAMP_M + 1)
RAMP_QUAD = [RAMP_ARC[0], RAMP_ARC[RAMP_M], RAMP_ARC[RAMP_M + 1], RAMP_ARC[2 * RAMP_M + 1]]       # the same band as ONE quad


def ramp_page():
    """uint8 [h][w][3]: rint(RAMP_SLOPE * r), the same in all channels (below 255 all over the band)"""
    import numpy as np
    h, w = RAMP_PAGE
    Y, X = np.mgrid[0:h, 0:w]
    v = np.clip(np.rint(RAMP_SLOPE * np.hypot(X - RAMP_CENTRE[0], Y - RAMP_CENTRE[1])), 0, 255).astype(np.uint8)
    return np.ascontiguousarray(np.repeat(v[:, :, None], 3, 2))


def ramp_bound(cells):
    """the largest spread of a strip row, in grey levels, when the band is cut into `cells` cells: a row is a chord of its circle and dips
    towards the centre by at most the sagitta R_out (1 - cos(theta / 2 cells)); a polygon point rounded to a pixel lies up to 0.71 pixels
    off its circle; the ramp's slope turns pixels into levels; rounding the page to bytes and the strip's own rounding add one level"""
    theta = math.radians(RAMP_DEG[1] - RAMP_DEG[0])
    return (RAMP_R_OUT * (1.0 - math.cos(theta / (2 * cells))) + 0.71) * RAMP_SLOPE + 1.0


def row_spread(strip):
    """per row of a strip [rh][rw][3]: max - min of channel 0"""
    s = strip[:, :, 0].astype(int)
    return s.max(1) - s.min(1)
