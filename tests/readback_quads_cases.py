"""The quads of the quad read-back tests: the pages and items of tests/quad_cases.py and tests/persp_cases.py (S = 64,
pages 150x300 / 97x131 / 70x260) plus the items that stage adds - appended to their pages, so the earlier items keep their places."""
import persp_cases as PC
import quad_cases as QC

S, PAGES, K = QC.S, QC.PAGES, 2
box_quad, tilted = QC.box_quad, QC.tilted

# name, corners, frame or None (planned).  The overlapping pair (skew_7 / skew_30_overlap; trap_right / overlap), the clamped crop taps
# (overhang) and the frame that covers the middle of its quad only (larger_than_frame) are among the base items.
SIM_ADDED = [
    [("rw_is_32", box_quad(10, 60, 41, 66), None),                                           # strip 32 x 7: no horizontal pass at 32 x 32
     ("rh_is_32", box_quad(60, 110, 75, 141), None),                                         # strip 16 x 32: no vertical pass, narrower than the output
     ("touches_border", [(0, 100), (50, 96), (51, 108), (1, 112)], None)],                   # strip taps left of column 0 are clamped
    [("near_vertical", tilted(110, 48, 70, 12, 85), None),
     ("off_its_crop", tilted(40, 40, 70, 16, 20), (2 * 40, 2 * 40, 24, 94, 34))],            # a 24-pixel frame on a 70-pixel line: original bytes beyond it
    [("rw_40_rh_24", box_quad(130, 40, 169, 63), None)],                                     # both passes skipped at 24 x 40
]
PERSP_ADDED = [
    [("rw_is_32", box_quad(10, 100, 41, 106), None),
     ("rh_is_32", box_quad(250, 80, 265, 111), None),
     ("touches_border", [(0, 104), (60, 108), (60, 124), (0, 130)], None)],
    [("near_vertical", [(112, 14), (118, 84), (106, 82), (102, 16)], None),
     ("off_its_crop", [(5, 20), (75, 24), (75, 36), (5, 44)], 30)],                          # a 30-pixel window on a 71-pixel strip
    [("rw_40_rh_24", box_quad(130, 40, 169, 63), None)],
]

# the overlapping pair of page 0 as (earlier, later) indices into the flat table
SIM_OVERLAP, PERSP_OVERLAP = (1, 2), (0, 4)


def sim_lists():
    """(names, quads, frames): P lists each, frames planned where open"""
    from diffute_amd import prepost
    items = [base + add for base, add in zip(QC.ITEMS, SIM_ADDED)]
    quads = [[it[1] for it in page] for page in items]
    frames = [[it[2] if it[2] is not None else prepost.frame_for(it[1], *PAGES[p]) for it in page] for p, page in enumerate(items)]
    return [[it[0] for it in page] for page in items], quads, frames


def persp_lists():
    """(names, quads, projective frames): the base items' frames as tests/persp_cases.py has them, the added ones planned (None) or a window
    of the given side about the strip's centre"""
    from diffute_amd import prepost
    base_q, base_f = PC.lists()
    names = [[it[0] for it in page] + [a[0] for a in add] for page, add in zip(PC.ITEMS, PERSP_ADDED)]
    quads = [q + [a[1] for a in add] for q, add in zip(base_q, PERSP_ADDED)]
    frames = [f + [prepost.persp_frame_for(a[1], *PAGES[p], S) if a[2] is None else PC.frame_of(a[1], a[2]) for a in add]
              for p, (f, add) in enumerate(zip(base_f, PERSP_ADDED))]
    return names, quads, frames


def lists(perspective):
    return persp_lists() if perspective else sim_lists()
