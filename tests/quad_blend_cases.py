"""The pages, quads, blends and choice tables shared by tests/test_quad_blend_host.py and tests/test_quad_blend_gpu.py.  Thirteen quads on the
three small pages of tests/quad_cases.py (150 x 300, 97 x 131, 70 x 260; two are wider than the paste's 256-column tile) at S = 64:
axis-aligned, tilted 7 degrees, an overlapping pair with the later one on top, a trapezoid with its right edge at 0.8 of its left, a quad
whose grown bounding box leaves the page, a line read top to bottom, a quad partly off its crop, a line upside down whose end lies off its
crop over an earlier quad (the deviation from the plain paste), a quad one pixel
between its long edges, a tilted quad across column 256 and - in the similarity frame only: its homography does not exist - a quad with a
degenerate corner.  Every geometry serves both frames; a case is (frame, blend, choice table or None)."""
import collections

import numpy as np

import persp_cases as PC
import quad_cases as QC
import quad_blend_restatement as QB
import quad_restatement as QR
import persp_restatement as PR

S = QC.S
PAGES = QC.PAGES
K = 3

# per page: name, corners TL TR BR BL, the similarity frame or None (prepost.frame_for plans it), the projective frame's (crop_scale,
# centre) or None (prepost.persp_frame_for plans it); "no_persp": the quad is left out of the projective cases
ITEMS = [
    [("axis", QC.box_quad(20, 20, 50, 32), None, None),
     ("skew_7", QC.tilted(150, 75, 120, 14, 7), None, None),
     ("overlap_on_top", QC.tilted(170, 80, 100, 16, 30), None, None),                              # overlaps skew_7; the item the choice table skips
     ("trapezoid_08", [(200, 20), (280, 22), (280, 38), (200, 40)], None, None),                  # right edge 16, left edge 20; both sides of column 256
     ("leaves_page", QC.tilted(30, 140, 50, 10, -5), None, None)],                                # grown by grow (+ ring) it leaves the page's corner
    [("top_to_bottom", [(80, 10), (80, 70), (68, 70), (68, 10)], None, None),
     ("partly_off_crop", QC.tilted(36, 82, 60, 12, 8), (2 * 36, 2 * 82, 40, 99, 14), (40, None))],  # a 40-pixel frame on a 60-pixel line
    [("under_the_end", QC.tilted(92, 42, 30, 12, 20), None, None),                                # under the end of upside_down, where that line is off its crop
     ("upside_down", [(100, 50), (20, 50), (20, 30), (100, 30)], None, None),                      # an 80-pixel line in a 70-pixel frame
     ("thin", [(10, 3), (110, 9), (110, 10), (10, 4)], None, None),                               # one pixel between its long edges
     ("tile_edge", QC.tilted(236, 35, 40, 14, -15), None, None),
     ("degenerate_corner", [(130, 20), (170, 20), (170, 40), (170, 40)], None, "no_persp"),       # BR == BL: an edge of length 0
     ("over_upside_down", QC.tilted(60, 45, 50, 12, 20), None, None)],                            # on top of upside_down
]

BLENDS = collections.OrderedDict([
    ("feather_wide", QB.Blend(feather=9)),                                      # grow = 0: the ramp inside; 9 > half of every quad's height
    ("grow_ge_feather", QB.Blend(feather=3, grow=4)),
    ("match_only", QB.Blend(match_color=True)),
    ("feather_grow_match", QB.Blend(feather=3, grow=4, match_color=True, ring=5, max_shift=12)),
    ("grow_lt_feather", QB.Blend(feather=5, grow=2, match_color=True, ring=3)),
])
SKIPPED = "overlap_on_top"
# the quads every pixel of which lies on the quad's own crop, in both frames: on them QuadBlend() is the plain quad paste (the tests
# assert the premise before they assert the equality)
ON_CROP = ("axis", "skew_7", "overlap_on_top", "trapezoid_08", "top_to_bottom", "under_the_end", "degenerate_corner", "over_upside_down")


def geometry(persp, keep=None):
    """(names, quads, frames) of one frame kind: P lists each, the open frames planned by prepost; keep: the names to keep, or None"""
    from diffute_amd import prepost
    names, quads, frames = [], [], []
    for p, items in enumerate(ITEMS):
        h, w = PAGES[p]
        kept = [it for it in items if not (persp and it[3] == "no_persp") and (keep is None or it[0] in keep)]
        names.append([it[0] for it in kept]); quads.append([it[1] for it in kept])
        if persp:
            frames.append([PC.frame_of(it[1], it[3][0], it[3][1]) if it[3] is not None else prepost.persp_frame_for(it[1], h, w, S) for it in kept])
        else:
            frames.append([it[2] if it[2] is not None else prepost.frame_for(it[1], h, w) for it in kept])
    return names, quads, frames


def prepared(persp, quads, frames, sizes=PAGES, S=S):
    """the prepared integers of every item, page-major: [(q dict, pm dict or None)] from the tables the host-only prepare entries fill"""
    from diffute_amd import _cabi
    lib, P, B = _cabi.lib(), len(sizes), sum(len(q) for q in quads)
    if persp:
        pt, qt, xt = PC.tables(sizes, quads, frames)
        _cabi.check(lib.dmx_edit_quads_prepare(pt, P, qt, B, S), "edit_quads_prepare")
        _cabi.check(lib.dmx_edit_quads_persp_prepare(pt, P, qt, xt, B, S), "edit_quads_persp_prepare")
        return [(QR.from_table(q), PR.from_table(x)) for q, x in zip(qt, xt)]
    pt, qt = QC.tables(sizes, quads, frames)
    _cabi.check(lib.dmx_edit_quads_prepare(pt, P, qt, B, S), "edit_quads_prepare")
    return [(QR.from_table(q), None) for q in qt]


def pages():
    """the three pages: a slope and a tone per page under noise, so that a patch is off in tone against its surroundings"""
    rs = np.random.RandomState(20261021)
    out = []
    for p, (h, w) in enumerate(PAGES):
        yy, xx = np.mgrid[0:h, 0:w]
        base = 90 + 30 * p + (xx * 60) // w + (yy * 40) // h
        out.append(np.clip(base[:, :, None] + np.array([0, 12, -9])[None, None, :] + rs.randint(-20, 21, (h, w, 3)), 0, 255).astype(np.uint8))
    return out


def rows(n):
    """decoder outputs [n][K][3][S][S]: noise about a tone of their own per item and candidate, some values beyond [-1, 1]"""
    rs = np.random.RandomState(7)
    tone = rs.uniform(-0.5, 0.7, (n, K, 3, 1, 1))
    return (tone + rs.standard_normal((n, K, 3, S, S)) * 0.35).clip(-1.3, 1.3).astype(np.float32)


class Case:
    """one frame kind, one blend, and with `choice` a table over K = 3 candidates (the skipped item -1); without it candidate 0"""

    def __init__(self, name, persp, blend, choice, keep=None):
        self.name, self.persp, self.blend = name, persp, blend
        self.names, self.quads, self.frames = geometry(persp, keep)
        self.N = sum(len(q) for q in self.quads)
        self.pages = pages()
        self.rows = rows(self.N)                                                  # [N][K][3][S][S]
        flat = [n for ns in self.names for n in ns]
        self.choice = None if not choice else [-1 if n == SKIPPED else (b * 2 + 1) % K for b, n in enumerate(flat)]
        self.items = prepared(persp, self.quads, self.frames)

    def row(self, b, table=None):
        """the decoder row of item b: candidate 0, or the table's (clamped to K - 1; None = skipped)"""
        table = self.choice if table is None else table
        if table is None:
            return self.rows[b, 0]
        return None if table[b] < 0 else self.rows[b, min(table[b], K - 1)]

    def page_items(self, p, table=None):
        lo = sum(len(q) for q in self.quads[:p])
        return [self.items[b] + (self.row(b, table),) for b in range(lo, lo + len(self.quads[p]))]

    def expected(self, fault=None, table=None):
        """[(out, mask, stats or None)] per page from the restatement"""
        return [QB.paste_page(self.pages[p], self.page_items(p, table), S, self.blend, fault) for p in range(len(self.pages))]


def cases():
    out = []
    for persp in (False, True):
        kind = "persp" if persp else "sim"
        for bname, blend in BLENDS.items():
            out.append(Case(f"{kind}-{bname}", persp, blend, False))
        out.append(Case(f"{kind}-choice_k3", persp, BLENDS["feather_grow_match"], True))
    return out


def on_crop_cases():
    """the quads of ON_CROP with everything off, per frame kind: what must equal the plain quad paste"""
    return [Case(("persp" if persp else "sim") + "-all_off", persp, QB.Blend(), False, ON_CROP) for persp in (False, True)]


def rot90_case(c):
    """(pages, quads, frames) of a case turned by a quarter (np.rot90): the similarity frames turn along, the projective ones live in
    strip space and stay"""
    tp = [QR.rot90_page(p) for p in c.pages]
    tq = [[QR.rot90_corners(q, w) for q in qs] for qs, (h, w) in zip(c.quads, PAGES)]
    tf = c.frames if c.persp else [[QR.rot90_frame(f, w) for f in fs] for fs, (h, w) in zip(c.frames, PAGES)]
    return tp, tq, tf
