"""The pages, quads and frames shared by tests/test_prepost_quad_host.py and tests/test_prepost_quad_gpu.py, and the ctypes tables built
from them.  Three small pages at S = 64; two are wider than the paste's 256-column tile."""
import math

S = 64
PAGES = [(150, 300), (97, 131), (70, 260)]            # h x w


def tilted(cx, cy, length, height, degrees):
    """the corners TL, TR, BR, BL of a length x height line centred at (cx, cy) whose baseline is turned by `degrees` (y down), rounded"""
    t = math.radians(degrees)
    ux, uy, vx, vy = math.cos(t), math.sin(t), -math.sin(t), math.cos(t)
    return [(int(round(cx + sx * length / 2 * ux + sy * height / 2 * vx)), int(round(cy + sx * length / 2 * uy + sy * height / 2 * vy)))
            for sx, sy in ((-1, -1), (1, -1), (1, 1), (-1, 1))]


def box_quad(x1, y1, x2, y2):
    return [(x1, y1), (x2, y1), (x2, y2), (x1, y2)]


# per page: name, corners, frame (cx2, cy2, crop_scale, ux, uy) or None = prepost.frame_for plans it
ITEMS = [
    [("axis_copy", box_quad(20, 20, 50, 32), (2 * 15 + S - 1, 2 * 10 + S - 1, S, 1, 0)),        # crop_scale = S on a half-pixel: page[10:74, 15:79]
     ("skew_7", tilted(150, 75, 120, 14, 7), None),
     ("skew_30_overlap", tilted(170, 80, 100, 16, 30), None),                               # overlaps skew_7: the later one decides
     ("skew_m15_tile_edge", tilted(250, 100, 80, 12, -15), None)],                          # both sides of column 256
    [("rot_90", [(80, 10), (80, 70), (68, 70), (68, 10)], (2 * 74, 2 * 40, S, 0, 120)),        # read top to bottom
     ("overhang", [(2, 80), (60, 84), (59, 95), (1, 91)], (2 * 30, 2 * 87, 100, 116, 8))],    # a 100-pixel frame on a 97-row page: clamped taps
    [("rot_180", [(100, 50), (20, 50), (20, 30), (100, 30)], None),                          # upside down
     ("thin", [(10, 3), (110, 9), (110, 10), (10, 4)], None),                                # one pixel between its long edges
     ("larger_than_frame", tilted(200, 35, 100, 40, 10), (2 * 200, 2 * 35, 48, 98, 18))],     # the frame covers the middle of the quad only
]
FLAT = [(p, it) for p, items in enumerate(ITEMS) for it in items]
N = len(FLAT)


def lists():
    """(quads, frames) as the prepost functions take them: P lists each; the open frames planned by prepost.frame_for"""
    from diffute_amd import prepost
    quads = [[it[1] for it in items] for items in ITEMS]
    frames = [[it[2] if it[2] is not None else prepost.frame_for(it[1], *PAGES[p]) for it in items] for p, items in enumerate(ITEMS)]
    return quads, frames


def tables(sizes, quads, frames, original=64, out=128):
    """ctypes tables with dummy addresses: sizes [(h, w)], quads / frames P lists -> (dmx_edit_page * P, dmx_edit_quad * B)"""
    from diffute_amd import _cabi
    P, B = len(sizes), sum(len(q) for q in quads)
    pt, qt = (_cabi.EditPage * max(P, 1))(), (_cabi.EditQuad * max(B, 1))()
    lo = 0
    for p, ((h, w), qs, fs) in enumerate(zip(sizes, quads, frames)):
        pt[p].original, pt[p].out, pt[p].union_mask = original, out, 0
        pt[p].H, pt[p].W, pt[p].item_lo, pt[p].item_hi = h, w, lo, lo + len(qs)
        for it, c, f in zip(qt[lo:lo + len(qs)], qs, fs):
            for k in range(4):
                it.x[k], it.y[k] = c[k]
            it.cx2, it.cy2, it.crop_scale, it.ux, it.uy = f
            it.page = p
        lo += len(qs)
    return pt, qt
