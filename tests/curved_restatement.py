"""Python-int / numpy restatement of csrc/prepost_curved.h, written from its header comment: curved text regions - polygons of 2n points -
straightened by piecewise-affine maps.

Two halves, kept apart.  The HOST half (`strip`, `piece_matrix`, `host_item`, `accept`) gives what dmx_edit_curved_prepare must fill into a
dmx_edit_curved and its dmx_curved_piece entries: the strip's size in float64 in the stated order of operations, everything else in Python
ints.  The KERNELS' half (`piece_of`, `preprocess`, `rectify`, `paste_page`) consumes prepared items as dicts, from `host_item` or from
`from_table` (what the entry did fill), in numpy int64.  A map is tests/persp_restatement.py's (relative, coords), taps, the single
rounding, the quad predicate and the paste value are tests/quad_restatement.py's: only the region and which map a pixel takes are restated
here.  `faults` switches on deliberate mistakes, one name each:
  floor - floor instead of round-to-nearest, ties away          other_diagonal - cells cut from T_k to B_k+1
  bbox_cell - the paste picks a pixel's cell by the cells' page bounding boxes, the crop and the strip by the boxes' columns
  homography - one homography per cell instead of two affine pieces
  rh_summed - rh from the summed vectors B_k - T_k instead of their mean length
  cell_left_out - the predicate forgets the last cell"""
from fractions import Fraction

import numpy as np

import persp_restatement as PR
import quad_restatement as QR

I64 = np.int64
MAX_PAIRS = 17
SIZE_MAX = 1 << 20
Refused = PR.Refused


# ---------------------------------------------------------------------------------------------------------------- the host half
def pairs(points):
    """[(x, y)] * 2n -> (n, T, B): T_k = p[k], B_k = p[2n - 1 - k]"""
    p = [(int(x), int(y)) for x, y in points]
    if len(p) % 2:
        raise Refused("an odd point count")
    n = len(p) // 2
    if not 2 <= n <= MAX_PAIRS:
        raise Refused(f"{n} point pairs")
    return n, p[:n], [p[2 * n - 1 - k] for k in range(n)]


def cell_corners(points, k):
    n, T, B = pairs(points)
    return [T[k], T[k + 1], B[k + 1], B[k]]


def cell_dicts(points):
    """the cells as quad_restatement.inside takes them"""
    n = len(points) // 2
    out = []
    for k in range(n - 1):
        c = cell_corners(points, k)
        x, y = [v[0] for v in c], [v[1] for v in c]
        out.append(dict(x=x, y=y, ex=[x[(a + 1) % 4] - x[a] for a in range(4)], ey=[y[(a + 1) % 4] - y[a] for a in range(4)],
                        bx1=min(x), by1=min(y), bx2=max(x), by2=max(y)))
    return out


def check_cells(points, H, W):
    """what the prepare entry refuses about the polygon itself: raises Refused naming the cell"""
    n, T, B = pairs(points)
    for k in range(n - 1):
        c = cell_corners(points, k)
        area2 = 0
        for a in range(4):
            (x0, y0), (x1, y1), (x2, y2) = c[a], c[(a + 1) % 4], c[(a + 2) % 4]
            if (x1 - x0) * (y2 - y1) - (y1 - y0) * (x2 - x1) < 0:
                raise Refused(f"cell {k} turns the wrong way")
            area2 += x0 * y1 - x1 * y0
        if area2 <= 0:
            raise Refused(f"cell {k} has no area")
        if any(not (0 <= x < W and 0 <= y < H) for x, y in c):
            raise Refused(f"cell {k}: a point lies outside the page")


def strip(points, faults=()):
    """-> (rw, rh, c): float64, in the header's order of operations"""
    n, T, B = pairs(points)
    M = n - 1
    f64 = np.float64
    c = [0]
    for k in range(M):
        ux = (T[k + 1][0] - T[k][0]) + (B[k + 1][0] - B[k][0])
        uy = (T[k + 1][1] - T[k][1]) + (B[k + 1][1] - B[k][1])
        c.append(c[-1] + max(1, QR.rn(np.sqrt(f64(ux * ux + uy * uy)) / 2.0)))
    if "rh_summed" in faults:
        sx, sy = sum(B[k][0] - T[k][0] for k in range(n)), sum(B[k][1] - T[k][1] for k in range(n))
        rh = QR.rn(np.sqrt(f64(sx * sx + sy * sy)) / f64(M + 1)) + 1
    else:
        total = f64(0.0)
        for k in range(n):
            dx, dy = B[k][0] - T[k][0], B[k][1] - T[k][1]
            total = total + np.sqrt(f64(dx * dx + dy * dy))
        rh = QR.rn(total / f64(M + 1)) + 1
    return c[M] + 1, rh, c


def piece_matrix(points, c, rh, piece, faults=()):
    """the exact integer matrix strip pixel-index space (i, j, 1) -> page of one piece, times w h"""
    n, T, B = pairs(points)
    k = piece >> 1
    w, h, ck = c[k + 1] - c[k], rh - 1, c[k]
    if "homography" in faults:                              # the cell's own homography, moved to its columns
        U = PR.unit_square_to_quad(cell_corners(points, k))
        return PR.mul3(PR.mul3(U, [[h, 0, 0], [0, w, 0], [0, 0, w * h]]), [[1, 0, -ck], [0, 1, 0], [0, 0, 1]])
    rows = []
    for a in range(2):
        t0, t1, b1, b0 = T[k][a], T[k + 1][a], B[k + 1][a], B[k][a]
        if "other_diagonal" in faults:                      # pieces (T_k, T_k+1, B_k+1) and (T_k, B_k+1, B_k)
            if piece & 1 == 0:
                ax, bx = (t1 - t0) * h, (b1 - t1) * w
                rows.append([ax, bx, t1 * w * h - ax * (ck + w)])
            else:
                ax, bx = (b1 - b0) * h, (b0 - t0) * w
                rows.append([ax, bx, t0 * w * h - ax * ck])
        elif piece & 1 == 0:
            ax, bx = (t1 - t0) * h, (b0 - t0) * w
            rows.append([ax, bx, t0 * w * h - ax * ck])
        else:
            ax, bx = (b1 - b0) * h, (b1 - t1) * w
            rows.append([ax, bx, b1 * w * h - ax * (ck + w) - bx * h])
    return rows + [[0, 0, w * h]]


def piece_maps(G, rw, rh, frame, S, faults=()):
    """the prepared integers of one piece, or with S = 0 its strip map alone: tests/persp_restatement.host_maps with G given"""
    strip_map = PR.relative(PR.mul3(G, [[1, 0, rw - 1], [0, 1, rh - 1], [0, 0, 2]]), faults)
    if S == 0:
        zero = dict(c16=[0, 0], t=[0] * 9)
        return dict(cx2=0, cy2=0, crop=zero, paste=dict(zero), strip=strip_map)
    ci2, cj2, cs = (int(v) for v in frame)
    M = PR.mul3(G, [[cs, 0, S * ci2], [0, cs, S * cj2], [0, 0, 2 * S]])
    crop = PR.relative(M, faults)
    cx2, cy2 = PR.rdiv(crop["c16"][0], 32768, faults), PR.rdiv(crop["c16"][1], 32768, faults)
    K = PR.mul3([[1, 0, S - 1], [0, 1, S - 1], [0, 0, 2]], PR.adj3(PR.mul3([[2, 0, -cx2], [0, 2, -cy2], [0, 0, 1]], M)))
    return dict(cx2=cx2, cy2=cy2, crop=crop, paste=PR.relative(K, faults), strip=strip_map)


def exact_matrices(G, rw, rh, frame, S, cx2, cy2):
    """the three exact integer matrices of one piece (crop grid -> page, page half-pixels about (cx2, cy2) -> crop pixel index, strip
    grid -> page), for tests/persp_restatement.exact_point"""
    ci2, cj2, cs = (int(v) for v in frame)
    M = PR.mul3(G, [[cs, 0, S * ci2], [0, cs, S * cj2], [0, 0, 2 * S]])
    K = PR.mul3([[1, 0, S - 1], [0, 1, S - 1], [0, 0, 2]], PR.adj3(PR.mul3([[2, 0, -cx2], [0, 2, -cy2], [0, 0, 1]], M)))
    return dict(crop=M, paste=K, strip=PR.mul3(G, [[1, 0, rw - 1], [0, 1, rh - 1], [0, 0, 2]]))


def host_item(points, frame, S, faults=()):
    """-> the dict of one prepared item: x, y, count, ci2, cj2, crop_scale, rw, rh, c (17 columns), bx1 .. by2, pieces (a list of
    piece_maps), cells (for the predicate).  No offsets: they depend on the table."""
    n, T, B = pairs(points)
    rw, rh, c = strip(points, faults)
    x, y = [int(p[0]) for p in points], [int(p[1]) for p in points]
    ci2, cj2, cs = (int(v) for v in frame)
    pieces = [piece_maps(piece_matrix(points, c, rh, piece, faults), rw, rh, frame, S, faults) for piece in range(2 * (n - 1))]
    return dict(x=x + [0] * (34 - 2 * n), y=y + [0] * (34 - 2 * n), count=2 * n, ci2=ci2, cj2=cj2, crop_scale=cs, rw=rw, rh=rh,
                c=c + [0] * (MAX_PAIRS - n), bx1=min(x), by1=min(y), bx2=max(x), by2=max(y), pieces=pieces, cells=cell_dicts(points), n=n)


def accept(item, S):
    """what dmx_edit_curved_prepare refuses about one item beyond its polygon: raises Refused"""
    rw, rh, n = item["rw"], item["rh"], item["n"]
    if rh < 2:
        raise Refused("the strip is thinner than 2 pixels")
    if rw > SIZE_MAX or rh > SIZE_MAX:
        raise Refused("the strip is too large")
    if S >= 1:
        if item["crop_scale"] == 0:
            raise Refused("no frame")
        if not 1 <= item["crop_scale"] <= 65535 or abs(item["ci2"]) > 1 << 20 or abs(item["cj2"]) > 1 << 20:
            raise Refused("the frame")
    g, gi, gj = S - 1, rw - 1, rh - 1
    for piece, m in enumerate(item["pieces"]):
        if S >= 1:
            PR._window(f"piece {piece}: crop window", m["crop"], [(-g, -g), (g, -g), (g, g), (-g, g)], g, g, True)
            cell = item["cells"][piece >> 1]
            pts = [(2 * x - m["cx2"], 2 * y - m["cy2"]) for x, y in zip(cell["x"], cell["y"])]
            PR._window(f"piece {piece}: page -> crop", m["paste"], pts, max(abs(p) for p, _ in pts), max(abs(q) for _, q in pts), False)
        PR._window(f"piece {piece}: strip", m["strip"], [(-gi, -gj), (gi, -gj), (gi, gj), (-gi, gj)], gi, gj, True)


ITEM_FIELDS = ("x", "y", "count", "ci2", "cj2", "crop_scale", "rw", "rh", "c", "bx1", "by1", "bx2", "by2")
TABLE_FIELDS = ("page", "piece_lo", "pieces", "rect_block_lo", "rect_blocks", "rect_off")


def from_table(entry, piece_table):
    """a ctypes dmx_edit_curved and the dmx_curved_piece table -> the dict `host_item` gives, plus the table's offsets"""
    d = {}
    for k in ITEM_FIELDS + TABLE_FIELDS:
        v = getattr(entry, k)
        d[k] = int(v) if isinstance(v, int) else [int(t) for t in v]
    d["piece_count"] = d.pop("pieces")
    n = d["count"] // 2
    d["n"] = n
    d["pieces"] = []
    for piece in range(d["piece_count"]):
        e = piece_table[d["piece_lo"] + piece]
        m = dict(cx2=int(e.cx2), cy2=int(e.cy2))
        for name in PR.MAP_NAMES:
            t = getattr(e, name)
            m[name] = dict(c16=[int(v) for v in t.c16], t=[int(v) for v in t.t])
        d["pieces"].append(m)
    d["cells"] = cell_dicts(list(zip(d["x"][:2 * n], d["y"][:2 * n])))
    return d


# ---------------------------------------------------------------------------------------------------------------- the kernels' half
def inside(item, X, Y, faults=()):
    """the region's predicate: some cell covers the pixel"""
    X, Y = np.asarray(X, I64), np.asarray(Y, I64)
    cells = item["cells"][:-1] if "cell_left_out" in faults and len(item["cells"]) > 1 else item["cells"]
    ok = np.zeros(np.broadcast(X, Y).shape, bool)
    for q in cells:
        ok |= QR.inside(q, X, Y)
    return ok


def piece_of(item, I, J, den, faults=()):
    """the piece of the strip positions (I / den, J / den) (int64 arrays): the column band, then the side of the diagonal"""
    I, J = np.asarray(I, I64), np.asarray(J, I64)
    c, M, h = item["c"], item["n"] - 1, I64(item["rh"] - 1)
    den = I64(den)
    k = np.zeros(np.broadcast(I, J).shape, I64)
    for m in range(1, M):
        if "bbox_cell" in faults:                           # the box of cell m - 1 holds its right edge: the shared column goes left
            k += (I > den * I64(c[m])).astype(I64)
        else:
            k += (I >= den * I64(c[m])).astype(I64)
    ck = np.asarray(c, I64)[k]
    w = np.asarray(c, I64)[k + 1] - ck
    if "other_diagonal" in faults:                          # the diagonal from (c_k, 0) to (c_k + w, rh - 1): piece 2k above it
        upper = J * w <= (I - den * ck) * h
    else:
        upper = (I - den * ck) * h + J * w <= den * w * h
    return 2 * k + np.where(upper, 0, 1)


def _by_piece(item, name, piece, p, q, faults=()):
    """the coordinates of grid points (p, q), each under the map `name` of its own piece"""
    A, B = np.zeros(piece.shape, I64), np.zeros(piece.shape, I64)
    for g in np.unique(piece):
        sel = piece == g
        a, b = PR.coords(item["pieces"][int(g)][name], p[sel], q[sel], faults=faults)
        A[sel], B[sel] = a, b
    return A, B


def crop_coords(item, S, faults=()):
    """(X16, Y16, piece) int64 [S][S] of the crop pixels (row dy, column dx)"""
    px, py = PR.crop_grid(S)
    piece = piece_of(item, I64(S) * item["ci2"] + I64(item["crop_scale"]) * px, I64(S) * item["cj2"] + I64(item["crop_scale"]) * py, 2 * S, faults)
    return _by_piece(item, "crop", piece, px, py, faults) + (piece,)


def strip_coords(item, faults=()):
    rw, rh = item["rw"], item["rh"]
    px, py = PR.strip_grid(rw, rh)
    j, i = np.meshgrid(np.arange(rh, dtype=I64), np.arange(rw, dtype=I64), indexing="ij")
    piece = piece_of(item, i, j, 1, faults)
    return _by_piece(item, "strip", piece, px, py, faults) + (piece,)


def preprocess(page, item, S, faults=()):
    """-> the dict quad_restatement.preprocess gives"""
    H, W, _ = page.shape
    X16, Y16, _ = crop_coords(item, S, faults)
    tx, ty = QR._taps(X16, W), QR._taps(Y16, H)
    pg = page.astype(I64)
    img = np.stack([QR._sample(lambda yi, xi: pg[yi, xi, ch], tx, ty) for ch in range(3)], -1)
    msk = np.stack([QR._sample(lambda yi, xi: np.where(inside(item, xi, yi, faults), 0, pg[yi, xi, ch]), tx, ty) for ch in range(3)], -1)
    mask = QR._sample(lambda yi, xi: inside(item, xi, yi, faults).astype(I64), tx, ty).astype(np.uint8)
    img, msk = img.astype(np.uint8), msk.astype(np.uint8)
    return dict(image=QR.normalize(img), masked_image=QR.normalize(msk), mask=mask, mask_latent=mask[::8, ::8].astype(np.float32), image_u8=img,
                masked_u8=msk)


def rectify(page, item, faults=()):
    """-> uint8 [rh][rw][3]"""
    H, W, _ = page.shape
    X16, Y16, _ = strip_coords(item, faults)
    tx, ty = QR._taps(X16, W), QR._taps(Y16, H)
    pg = page.astype(I64)
    return np.stack([QR._sample(lambda yi, xi: pg[yi, xi, ch], tx, ty) for ch in range(3)], -1).astype(np.uint8)


def page_pieces(item, X, Y, faults=()):
    """per page pixel: the piece of the FIRST cell of the item that covers it, or -1"""
    X, Y = np.asarray(X, I64), np.asarray(Y, I64)
    piece = np.full(np.broadcast(X, Y).shape, -1, I64)
    cells = item["cells"][:-1] if "cell_left_out" in faults and len(item["cells"]) > 1 else item["cells"]
    for k, q in enumerate(cells):
        if "bbox_cell" in faults:
            cov = (X >= q["bx1"]) & (X <= q["bx2"]) & (Y >= q["by1"]) & (Y <= q["by2"]) & inside(item, X, Y)
        else:
            cov = QR.inside(q, X, Y)
        if "other_diagonal" in faults:                      # the diagonal from corner 0 to corner 2: piece 2k on its corner-1 side
            E = I64(q["x"][2] - q["x"][0]) * (Y - q["y"][0]) - I64(q["y"][2] - q["y"][0]) * (X - q["x"][0])
            odd = E > 0
        else:
            E = I64(q["x"][3] - q["x"][1]) * (Y - q["y"][1]) - I64(q["y"][3] - q["y"][1]) * (X - q["x"][1])
            odd = E < 0
        new = cov & (piece < 0)
        piece[new] = (2 * k + odd.astype(I64))[new]
    return piece


def paste_page(page, items, vaes, S, faults=()):
    """One page, its items in table order and their decoder outputs ([3][S][S] each) -> dict(out, union, pasted, hit, piece)"""
    H, W, _ = page.shape
    Y, X = np.meshgrid(np.arange(H, dtype=I64), np.arange(W, dtype=I64), indexing="ij")
    hit, piece = np.full((H, W), -1, np.int64), np.full((H, W), -1, np.int64)
    for b, item in enumerate(items):
        pc = page_pieces(item, X, Y, faults)
        hit[pc >= 0] = b
        piece[pc >= 0] = pc[pc >= 0]
    out, pasted = page.copy(), np.zeros((H, W), bool)
    top = (I64(S) << 16) - 32768
    for b, item in enumerate(items):
        for g in np.unique(piece[hit == b]):
            sel = (hit == b) & (piece == g)
            m = item["pieces"][int(g)]
            U16, V16 = (np.asarray(v).astype(I64) for v in
                        PR.coords(m["paste"], 2 * X[sel] - m["cx2"], 2 * Y[sel] - m["cy2"], faults=faults))
            on = (U16 >= -32768) & (U16 < top) & (V16 >= -32768) & (V16 < top)
            ok = np.zeros((H, W), bool)
            ok[sel] = on
            out[ok] = np.clip(np.rint(QR.paste_value(vaes[b], S, U16[on], V16[on])), 0, 255).astype(np.uint8)
            pasted |= ok
    return dict(out=out, union=(hit >= 0).astype(np.uint8), pasted=pasted, hit=hit, piece=piece)


def exact_point(M, p, q):
    return PR.exact_point(M, p, q)


BOUND = Fraction(1, 2) + Fraction(1, 8) * (1 + Fraction(1, 1 << 18))      # csrc/prepost_persp.h: 0.6251 units of 2^-16
