"""The pages, quads and projective frames shared by tests/test_prepost_persp_host.py and tests/test_prepost_persp_gpu.py, and the ctypes
tables built from them.  The three small pages of tests/quad_cases.py at S = 64; a projective frame is (ci2, cj2, crop_scale): the
window's centre in half-pixels of the strip's pixel-index space and its side in strip pixels."""
import quad_cases as QC

S = QC.S
PAGES = QC.PAGES                                      # (150, 300), (97, 131), (70, 260): h x w
box_quad = QC.box_quad

CENTRE = None                                         # the frame's centre = the strip's centre (rw - 1, rh - 1)

# per page: name, corners TL TR BR BL, crop_scale, centre (ci2, cj2) or CENTRE
ITEMS = [
    [("trap_right", [(60, 40), (200, 48), (200, 72), (60, 84)], 160, CENTRE),               # the right edge at 24 / 44 of the left one
     ("keystone_down", [(100, 100), (180, 100), (190, 130), (90, 130)], 96, CENTRE),
     ("general_tile_edge", [(215, 20), (290, 28), (288, 46), (212, 44)], 90, CENTRE),       # both sides of column 256
     ("axis_copy", box_quad(20, 20, 50, 32), S, (2 * (15 - 20) + S - 1, 2 * (10 - 20) + S - 1)),   # the crop is page[10:74, 15:79]
     ("overlap", [(150, 50), (230, 44), (232, 66), (150, 70)], 100, CENTRE)],               # overlaps trap_right: the later one decides
    [("rot90_persp", [(90, 10), (90, 80), (70, 74), (66, 12)], 80, CENTRE),                 # read top to bottom
     ("overhang", [(2, 78), (60, 84), (59, 95), (1, 93)], 100, CENTRE)],                    # a 100-pixel window on a 97-row page: clamped taps
    [("parallelogram", [(20, 20), (120, 30), (125, 50), (25, 40)], 110, CENTRE),            # affine: t6 = t7 = 0
     ("thin", [(140, 3), (250, 9), (250, 11), (140, 7)], 112, CENTRE)],
]
FLAT = [(p, it) for p, items in enumerate(ITEMS) for it in items]
N = len(FLAT)

# the quad whose vanishing line lies close: refused at crop_scale 240 (the horizon crosses the window) and at 150 (the ratio of the
# denominators over the window lies between 4 and infinity); accepted at 64
HORIZON_QUAD = [(20, 10), (200, 40), (200, 48), (20, 80)]
# left edge 120, right edge 45 on a 1100 x 1300 page: its strip (301 x 83) is within the cap, a 512-pixel window on it is not, a 384-pixel one is
STEEP_QUAD = [(300, 400), (600, 437), (600, 482), (300, 520)]
FLAT_STRIP_QUAD = [(20, 20), (120, 20), (120, 20), (20, 21)]      # |v| = 1: rh = rn(1 / 2) + 1 = 1


def strip_size(corners):
    import persp_restatement as PR
    return PR.strip_size(corners)


def frame_of(corners, crop_scale, centre=CENTRE):
    rw, rh = strip_size(corners)
    ci2, cj2 = (rw - 1, rh - 1) if centre is None else centre
    return (ci2, cj2, crop_scale)


def lists():
    """(quads, frames) as the prepost functions take them with perspective=True: P lists each"""
    quads = [[it[1] for it in items] for items in ITEMS]
    frames = [[frame_of(it[1], it[2], it[3]) for it in items] for items in ITEMS]
    return quads, frames


def tables(sizes, quads, frames, original=64, out=128):
    """ctypes tables with dummy addresses: (dmx_edit_page * P, dmx_edit_quad * B, dmx_quad_persp * B); the similarity frames of the quad
    table are the placeholders prepost uses where no frame is read"""
    from diffute_amd import _cabi
    sim = [[(2 * c[0][0], 2 * c[0][1], 1, 1, 0) for c in qs] for qs in quads]
    pt, qt = QC.tables(sizes, quads, sim, original, out)
    B = sum(len(q) for q in quads)
    xt = (_cabi.QuadPersp * max(B, 1))()
    for e, f in zip(xt, [f for fs in frames for f in fs]):
        if f is not None:
            e.ci2, e.cj2, e.crop_scale = f
    return pt, qt, xt
