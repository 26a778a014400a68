"""numpy / Python-int restatement of csrc/prepost_persp.h, written from its header comment: quadrilateral text regions seen through the
homography that takes the quad to its upright rw x rh strip.

Two halves, kept apart.  The HOST half (`host_maps`, `accept`) is Python ints only - exact, no float anywhere - and gives what
dmx_edit_quads_persp_prepare must fill into a dmx_quad_persp.  The KERNELS' half (`coords`, `preprocess`, `rectify`, `paste_page`) consumes
prepared maps as dicts, from `host_maps` or from `from_table` (what the entry did fill), in numpy int64 - or, with ints=object, in Python
ints, to show that nothing wraps.  Taps, the single rounding, the predicate and the paste rule are tests/quad_restatement.py's: only
where the coordinates come from is restated here.  `faults` switches on deliberate mistakes, one name each:
  floor - floor instead of round-to-nearest, ties away        unrounded_centre - coefficients about the exact centre, not the rounded one
  u_over_rw - u = i / rw instead of i / (rw - 1)               transposed_adjugate - the page -> crop matrix transposed
  cap_ignored - `accept` does not look at max D / min D        one_step - rdiv(n << 16, D) in one 64-bit division (wraps)"""
import numpy as np

import quad_restatement as QR

I64 = np.int64
Q = 43                        # the denominator's scale: t8 = 2^Q
ONE = 1 << Q
CAP = 4                       # max D <= CAP * min D over a window
D_MAX = 1 << 45               # D < D_MAX = 4 * 2^Q: (r1 << 17) + D stays below 2^63
N_MAX = 1 << 58               # A = |t0| gx + |t1| gy + |t2| < N_MAX bounds every |n| and every partial sum of it
ERR_SHIFT = 18                # ((gx + gy + 1) * (min D + A)) << ERR_SHIFT <= (min D)^2: the coefficients' rounding moves a coordinate by < 1/8 of 2^-16


class Refused(ValueError):
    pass


# ---------------------------------------------------------------------------------------------------------------- the host half: Python ints
def rdiv(a, b, faults=()):
    """a / b rounded to nearest, ties away from zero; b > 0"""
    a, b = int(a), int(b)
    assert b > 0
    if "floor" in faults:
        return a // b
    m = (2 * abs(a) + b) // (2 * b)
    return -m if a < 0 else m


def strip_size(corners):
    """(rw, rh) of csrc/prepost_quad.h's rectify section"""
    d = QR.derive(corners, (0, 0, 1, 1, 0), 1)
    return d["rw"], d["rh"]


def unit_square_to_quad(corners):
    """the homography (u, v) in [0, 1]^2 -> page with (0,0) (1,0) (1,1) (0,1) -> TL TR BR BL, multiplied through by its denominator"""
    (x0, y0), (x1, y1), (x2, y2), (x3, y3) = [(int(x), int(y)) for x, y in corners]
    dx1, dx2, sx = x1 - x2, x3 - x2, x0 - x1 + x2 - x3
    dy1, dy2, sy = y1 - y2, y3 - y2, y0 - y1 + y2 - y3
    den = dx1 * dy2 - dy1 * dx2
    g, h = sx * dy2 - sy * dx2, dx1 * sy - dy1 * sx
    return [[(x1 - x0) * den + g * x1, (x3 - x0) * den + h * x3, x0 * den],
            [(y1 - y0) * den + g * y1, (y3 - y0) * den + h * y3, y0 * den],
            [g, h, den]]


def mul3(A, B):
    return [[sum(A[r][k] * B[k][c] for k in range(3)) for c in range(3)] for r in range(3)]


def adj3(M, faults=()):
    a, b, c, d, e, f, g, h, i = (M[r][k] for r in range(3) for k in range(3))
    A = [[e * i - f * h, c * h - b * i, b * f - c * e],
         [f * g - d * i, a * i - c * g, c * d - a * f],
         [d * h - e * g, b * g - a * h, a * e - b * d]]
    if "transposed_adjugate" in faults:
        A = [[A[k][r] for k in range(3)] for r in range(3)]
    return A


def strip_to_page(corners, rw, rh, faults=()):
    """G: strip pixel-index space (i, j, 1) -> page, u = i / (rw - 1), v = j / (rh - 1)"""
    a1, b1 = (rw, rh) if "u_over_rw" in faults else (rw - 1, rh - 1)
    return mul3(unit_square_to_quad(corners), [[b1, 0, 0], [0, a1, 0], [0, 0, a1 * b1]])


def relative(M, faults=()):
    """a 3 x 3 integer homography (grid -> target) as the table holds it: the Q16 image of the grid's centre and t0..t8 about it"""
    M = [list(r) for r in M]
    if M[2][2] < 0:
        M = [[-v for v in r] for r in M]
    m8 = M[2][2]
    if m8 == 0:
        raise Refused("the denominator vanishes at the centre")
    c16 = [rdiv(M[0][2] << 16, m8, faults), rdiv(M[1][2] << 16, m8, faults)]
    t = []
    for r in range(2):
        if "unrounded_centre" in faults:
            t += [rdiv((M[r][k] * m8 - M[r][2] * M[2][k]) << Q, m8 * m8, faults) for k in range(3)]
        else:
            t += [rdiv(((M[r][k] << 16) - c16[r] * M[2][k]) << (Q - 16), m8, faults) for k in range(3)]
    t += [rdiv(M[2][0] << Q, m8, faults), rdiv(M[2][1] << Q, m8, faults), ONE]
    return dict(c16=c16, t=t)


def host_maps(corners, rw, rh, frame, S, faults=()):
    """-> dict(ci2, cj2, crop_scale, cx2, cy2, crop, paste, strip): the prepared integers of one dmx_quad_persp"""
    ci2, cj2, cs = (int(v) for v in frame)
    G = strip_to_page(corners, rw, rh, faults)
    M = mul3(G, [[cs, 0, S * ci2], [0, cs, S * cj2], [0, 0, 2 * S]])
    crop = relative(M, faults)
    strip = relative(mul3(G, [[1, 0, rw - 1], [0, 1, rh - 1], [0, 0, 2]]), faults)
    cx2, cy2 = rdiv(crop["c16"][0], 32768, faults), rdiv(crop["c16"][1], 32768, faults)
    # page half-pixels about (cx2, cy2) -> grid (p, q, w) -> crop pixel index U = (p / w + S - 1) / 2
    A = adj3(mul3([[2, 0, -cx2], [0, 2, -cy2], [0, 0, 1]], M), faults)
    K = mul3([[1, 0, S - 1], [0, 1, S - 1], [0, 0, 2]], A)
    return dict(ci2=ci2, cj2=cj2, crop_scale=cs, cx2=cx2, cy2=cy2, crop=crop, paste=relative(K, faults), strip=strip)


def _window(what, m, pts, gx, gy, cap, faults=()):
    t = m["t"]
    D = [t[6] * p + t[7] * q + t[8] for p, q in pts]
    if min(D) <= 0:
        raise Refused(f"{what}: the denominator is not positive at all four corners (the horizon crosses it)")
    if cap and "cap_ignored" not in faults and max(D) > CAP * min(D):
        raise Refused(f"{what}: max D > {CAP} * min D (beyond the cap)")
    if max(D) >= D_MAX:
        raise Refused(f"{what}: the denominator leaves the budget")
    for r in (0, 3):
        A = abs(t[r]) * gx + abs(t[r + 1]) * gy + abs(t[r + 2])
        if A >= N_MAX or ((gx + gy + 1) * (min(D) + A)) << ERR_SHIFT > min(D) * min(D):
            raise Refused(f"{what}: the numerator leaves the budget")


def accept(maps, corners, rw, rh, S, faults=()):
    """what dmx_edit_quads_persp_prepare refuses about one item's maps (after the frame itself): raises Refused"""
    if rw < 2 or rh < 2:
        raise Refused("the strip is thinner than 2 pixels")
    g = S - 1
    _window("crop window", maps["crop"], [(-g, -g), (g, -g), (g, g), (-g, g)], g, g, True, faults)
    gi, gj = rw - 1, rh - 1
    _window("strip", maps["strip"], [(-gi, -gj), (gi, -gj), (gi, gj), (-gi, gj)], gi, gj, True, faults)
    pts = [(2 * int(x) - maps["cx2"], 2 * int(y) - maps["cy2"]) for x, y in corners]
    _window("page -> crop", maps["paste"], pts, max(abs(p) for p, _ in pts), max(abs(q) for _, q in pts), False, faults)


def exact_point(M, p, q):
    """the exact image of grid point (p, q) under the integer homography M, as Fractions"""
    from fractions import Fraction
    w = M[2][0] * p + M[2][1] * q + M[2][2]
    return Fraction(M[0][0] * p + M[0][1] * q + M[0][2], w), Fraction(M[1][0] * p + M[1][1] * q + M[1][2], w)


def exact_matrices(corners, rw, rh, frame, S, cx2, cy2):
    """the three exact integer homographies (crop grid -> page, page half-pixels about (cx2, cy2) -> crop pixel index, strip grid -> page)"""
    ci2, cj2, cs = (int(v) for v in frame)
    G = strip_to_page(corners, rw, rh)
    M = mul3(G, [[cs, 0, S * ci2], [0, cs, S * cj2], [0, 0, 2 * S]])
    K = mul3([[1, 0, S - 1], [0, 1, S - 1], [0, 0, 2]], adj3(mul3([[2, 0, -cx2], [0, 2, -cy2], [0, 0, 1]], M)))
    return M, K, mul3(G, [[1, 0, rw - 1], [0, 1, rh - 1], [0, 0, 2]])


# ---------------------------------------------------------------------------------------------------------------- the kernels' half
MAP_NAMES = ("crop", "paste", "strip")


def from_table(entry):
    """a ctypes dmx_quad_persp -> the dict `host_maps` gives"""
    d = {k: int(getattr(entry, k)) for k in ("ci2", "cj2", "crop_scale", "cx2", "cy2")}
    for k in MAP_NAMES:
        m = getattr(entry, k)
        d[k] = dict(c16=[int(v) for v in m.c16], t=[int(v) for v in m.t])
    return d


def _div16(n, D, ints, faults=()):
    """rdiv(n << 16, D) as the kernels do it: two steps, nothing leaves 64 bits"""
    an = np.abs(n)
    neg = n < 0
    if "one_step" in faults:
        m = ((an << 17) + D) // (2 * D)
    else:
        q1 = an // D
        r1 = an - q1 * D
        if "floor" in faults:
            q2 = (r1 << 16) // D
            m = (q1 << 16) + q2
            up = neg & ((r1 << 16) - q2 * D != 0)
            return np.where(neg, -m - np.where(up, 1, 0), m)
        m = (q1 << 16) + ((r1 << 17) + D) // (2 * D)
    return np.where(neg, -m, m)


def coords(m, p, q, ints=I64, faults=()):
    """(X16, Y16) of grid points (p, q) (arrays) under one prepared map; ints: np.int64 (the kernels) or object (Python ints)"""
    if ints is object:
        p, q = np.asarray(p).astype(object), np.asarray(q).astype(object)
        t, c = [int(v) for v in m["t"]], [int(v) for v in m["c16"]]
    else:
        p, q = np.asarray(p, I64), np.asarray(q, I64)
        t, c = [I64(v) for v in m["t"]], [I64(v) for v in m["c16"]]
    D = t[6] * p + t[7] * q + t[8]
    return c[0] + _div16(t[0] * p + t[1] * q + t[2], D, ints, faults), c[1] + _div16(t[3] * p + t[4] * q + t[5], D, ints, faults)


def crop_grid(S):
    py, px = np.meshgrid(2 * np.arange(S, dtype=I64) + 1 - S, 2 * np.arange(S, dtype=I64) + 1 - S, indexing="ij")
    return px, py


def strip_grid(rw, rh):
    py, px = np.meshgrid(2 * np.arange(rh, dtype=I64) + 1 - rh, 2 * np.arange(rw, dtype=I64) + 1 - rw, indexing="ij")
    return px, py


def _i64(a):
    return np.asarray(a).astype(I64)


def preprocess(page, q, pm, S, ints=I64, faults=()):
    """q: the quad's prepared dict (quad_restatement), pm: its projective maps -> the dict quad_restatement.preprocess gives"""
    H, W, _ = page.shape
    X16, Y16 = (_i64(v) for v in coords(pm["crop"], *crop_grid(S), ints=ints, faults=faults))
    tx, ty = QR._taps(X16, W), QR._taps(Y16, H)
    pg = page.astype(I64)
    img = np.stack([QR._sample(lambda yi, xi: pg[yi, xi, ch], tx, ty) for ch in range(3)], -1)
    msk = np.stack([QR._sample(lambda yi, xi: np.where(QR.inside(q, xi, yi), 0, pg[yi, xi, ch]), tx, ty) for ch in range(3)], -1)
    mask = QR._sample(lambda yi, xi: QR.inside(q, xi, yi).astype(I64), tx, ty).astype(np.uint8)
    img, msk = img.astype(np.uint8), msk.astype(np.uint8)
    return dict(image=QR.normalize(img), masked_image=QR.normalize(msk), mask=mask, mask_latent=mask[::8, ::8].astype(np.float32), image_u8=img,
                masked_u8=msk)


def rectify(page, q, pm, ints=I64, faults=()):
    """-> uint8 [rh][rw][3]"""
    H, W, _ = page.shape
    X16, Y16 = (_i64(v) for v in coords(pm["strip"], *strip_grid(q["rw"], q["rh"]), ints=ints, faults=faults))
    tx, ty = QR._taps(X16, W), QR._taps(Y16, H)
    pg = page.astype(I64)
    return np.stack([QR._sample(lambda yi, xi: pg[yi, xi, ch], tx, ty) for ch in range(3)], -1).astype(np.uint8)


def crop_coords(pm, X, Y, ints=I64, faults=()):
    """(U16, V16) of page pixels (X, Y)"""
    return coords(pm["paste"], 2 * np.asarray(X, I64) - pm["cx2"], 2 * np.asarray(Y, I64) - pm["cy2"], ints=ints, faults=faults)


def paste_page(page, qs, pms, vaes, S, ints=I64, faults=()):
    """quad_restatement.paste_page with the crop coordinates of the projective maps: -> dict(out, union, pasted, hit)"""
    H, W, _ = page.shape
    Y, X = np.meshgrid(np.arange(H, dtype=I64), np.arange(W, dtype=I64), indexing="ij")
    hit = np.full((H, W), -1, np.int64)
    for b, q in enumerate(qs):
        hit[QR.inside(q, X, Y)] = b
    out, pasted = page.copy(), np.zeros((H, W), bool)
    top = (I64(S) << 16) - 32768
    for b, pm in enumerate(pms):
        sel = hit == b
        if not sel.any():
            continue
        U16, V16 = (_i64(v) for v in crop_coords(pm, X[sel], Y[sel], ints=ints, faults=faults))
        on = (U16 >= -32768) & (U16 < top) & (V16 >= -32768) & (V16 < top)
        ok = np.zeros((H, W), bool)
        ok[sel] = on
        out[ok] = np.clip(np.rint(QR.paste_value(vaes[b], S, U16[on], V16[on])), 0, 255).astype(np.uint8)
        pasted |= ok
    return dict(out=out, union=(hit >= 0).astype(np.uint8), pasted=pasted, hit=hit)
