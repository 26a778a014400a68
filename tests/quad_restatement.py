"""numpy restatement of csrc/prepost_quad.h, written from its header comment: quadrilateral text regions with oriented crops.

It consumes the PREPARED integers of a dmx_edit_quad - as a dict, from `derive` (the closed form in float64, what dmx_edit_quads_prepare
must fill) or from `from_table` (what it did fill) - and computes the u8 paths in int64 and the paste in float32 (the kernel's
arithmetic, bit for bit) or float64 (for error bounds).  `faults` switches on deliberate mistakes, one name each, for the tests that show
the properties checked here can fail:
  transposed - b and c of the matrices swapped      flip_v - the sign of the matrix' second column flipped
  drop_half - 2d - S instead of 2d + 1 - S          exclusive - edges excluded (E > 0)
  reversed - the winding reversed (E <= 0)          first_wins - the FIRST covering item decides
  two_pass - the horizontal pass rounded to a byte before the vertical one        truncated - fractions cut to 8 bits"""
import numpy as np

I64 = np.int64


def rn(v):
    return int(np.rint(v))                       # round half to even


def derive(corners, frame, S):
    """corners: 4 x (x, y) TL TR BR BL; frame: (cx2, cy2, crop_scale, ux, uy) -> the dict of prepared integers (no offsets)"""
    x = [int(c[0]) for c in corners]; y = [int(c[1]) for c in corners]
    cx2, cy2, cs, ux, uy = (int(v) for v in frame)
    n = np.sqrt(np.float64(ux * ux + uy * uy))
    f64 = np.float64
    a, c = rn((f64(cs) * ux * 32768.0) / (n * S)), rn((f64(cs) * uy * 32768.0) / (n * S))
    ia, ib = rn((f64(S) * ux * 32768.0) / (n * cs)), rn((f64(S) * uy * 32768.0) / (n * cs))
    rux, ruy = (x[1] - x[0]) + (x[2] - x[3]), (y[1] - y[0]) + (y[2] - y[3])
    rvx, rvy = (x[3] - x[0]) + (x[2] - x[1]), (y[3] - y[0]) + (y[2] - y[1])
    nu, nv = np.sqrt(f64(rux * rux + ruy * ruy)), np.sqrt(f64(rvx * rvx + rvy * rvy))
    ra, rc = rn((f64(rux) * 32768.0) / nu), rn((f64(ruy) * 32768.0) / nu)
    return dict(x=x, y=y, cx2=cx2, cy2=cy2, crop_scale=cs, ux=ux, uy=uy, fwd=[a, -c, c, a], inv=[ia, ib, -ib, ia],
                ex=[x[(k + 1) % 4] - x[k] for k in range(4)], ey=[y[(k + 1) % 4] - y[k] for k in range(4)],
                bx1=min(x), by1=min(y), bx2=max(x), by2=max(y), rect=[ra, -rc, rc, ra], sx4=sum(x), sy4=sum(y),
                rw=rn(nu / 2.0) + 1, rh=rn(nv / 2.0) + 1)


FIELDS = ("x", "y", "cx2", "cy2", "crop_scale", "ux", "uy", "fwd", "inv", "ex", "ey", "bx1", "by1", "bx2", "by2", "rect", "sx4", "sy4", "rw", "rh")


def from_table(entry):
    """a ctypes dmx_edit_quad -> the dict `derive` gives (plus page, rect_off, rect_block_lo, rect_blocks)"""
    d = {}
    for k in FIELDS + ("page", "rect_off", "rect_block_lo", "rect_blocks"):
        v = getattr(entry, k)
        d[k] = int(v) if isinstance(v, int) else [int(t) for t in v]
    return d


def inside(q, X, Y, faults=()):
    """the predicate at integer pixel coordinates (arrays): all four edge functions >= 0, in int64"""
    X, Y = np.asarray(X, I64), np.asarray(Y, I64)
    ok = np.ones(np.broadcast(X, Y).shape, bool)
    for k in range(4):
        E = I64(q["ex"][k]) * (Y - q["y"][k]) - I64(q["ey"][k]) * (X - q["x"][k])
        ok &= (E <= 0) if "reversed" in faults else ((E > 0) if "exclusive" in faults else (E >= 0))
    return ok


def _matrix(m, faults):
    a, b, c, d = (I64(v) for v in m)
    if "transposed" in faults:
        b, c = c, b
    if "flip_v" in faults:
        b, d = -b, -d
    return a, b, c, d


def _taps(c16, n, faults=()):
    fl = c16 >> 16
    f = c16 & 65535
    if "truncated" in faults:
        f = f & ~I64(255)
    return np.clip(fl, 0, n - 1), np.clip(fl + 1, 0, n - 1), 65536 - f, f


def _round32(acc):
    return (acc + (I64(1) << 31)) >> 32


def _sample(vals, tx, ty, faults=()):
    """vals(yi, xi) -> int64 array of tap values; the single-rounding bilinear byte"""
    x0, x1, wx0, wx1 = tx
    y0, y1, wy0, wy1 = ty
    if "two_pass" in faults:
        r0 = (wx0 * vals(y0, x0) + wx1 * vals(y0, x1) + 32768) >> 16
        r1 = (wx0 * vals(y1, x0) + wx1 * vals(y1, x1) + 32768) >> 16
        return (wy0 * r0 + wy1 * r1 + 32768) >> 16
    return _round32(wy0 * wx0 * vals(y0, x0) + wy0 * wx1 * vals(y0, x1) + wy1 * wx0 * vals(y1, x0) + wy1 * wx1 * vals(y1, x1))


def frame_coords(q, S, faults=()):
    """(X16, Y16) int64 [S][S] of the crop pixels (row dy, column dx)"""
    a, b, c, d = _matrix(q["fwd"], faults)
    h = 0 if "drop_half" in faults else 1
    py, px = np.meshgrid(2 * np.arange(S, dtype=I64) + h - S, 2 * np.arange(S, dtype=I64) + h - S, indexing="ij")
    return (I64(q["cx2"]) << 15) + a * px + b * py, (I64(q["cy2"]) << 15) + c * px + d * py


def normalize(u8):
    """HWC bytes -> CHW fp32 in [-1, 1]: (x - 127.5) * (1 / 127.5) in fp32"""
    inv = np.float32(1.0) / np.float32(127.5)
    return np.ascontiguousarray(((u8.astype(np.float32) - np.float32(127.5)) * inv).transpose(2, 0, 1))


def preprocess(page, q, S, faults=()):
    """-> dict(image, masked_image: fp32 [3][S][S]; mask: uint8 [S][S]; mask_latent: fp32 [S/8][S/8]; image_u8, masked_u8: uint8 [S][S][3])"""
    H, W, _ = page.shape
    X16, Y16 = frame_coords(q, S, faults)
    tx, ty = _taps(X16, W, faults), _taps(Y16, H, faults)
    pg = page.astype(I64)
    img = np.stack([_sample(lambda yi, xi: pg[yi, xi, ch], tx, ty, faults) for ch in range(3)], -1)
    msk = np.stack([_sample(lambda yi, xi: np.where(inside(q, xi, yi, faults), 0, pg[yi, xi, ch]), tx, ty, faults) for ch in range(3)], -1)
    mask = _sample(lambda yi, xi: inside(q, xi, yi, faults).astype(I64), tx, ty, faults).astype(np.uint8)
    img, msk = img.astype(np.uint8), msk.astype(np.uint8)
    return dict(image=normalize(img), masked_image=normalize(msk), mask=mask, mask_latent=mask[::8, ::8].astype(np.float32), image_u8=img, masked_u8=msk)


def rectify(page, q, faults=()):
    """-> uint8 [rh][rw][3]"""
    H, W, _ = page.shape
    a, b, c, d = _matrix(q["rect"], faults)
    h = 0 if "drop_half" in faults else 1
    py, px = np.meshgrid(2 * np.arange(q["rh"], dtype=I64) + h - q["rh"], 2 * np.arange(q["rw"], dtype=I64) + h - q["rw"], indexing="ij")
    X16, Y16 = (I64(q["sx4"]) << 14) + a * px + b * py, (I64(q["sy4"]) << 14) + c * px + d * py
    tx, ty = _taps(X16, W, faults), _taps(Y16, H, faults)
    pg = page.astype(I64)
    return np.stack([_sample(lambda yi, xi: pg[yi, xi, ch], tx, ty, faults) for ch in range(3)], -1).astype(np.uint8)


def crop_coords(q, S, X, Y, faults=()):
    """(U16, V16) of page pixels (X, Y)"""
    ia, ib, ic, id_ = _matrix(q["inv"], faults)
    qx, qy = 2 * np.asarray(X, I64) - q["cx2"], 2 * np.asarray(Y, I64) - q["cy2"]
    base = I64(S - 1) << 15
    return base + ia * qx + ib * qy, base + ic * qx + id_ * qy


def paste_value(vae, S, U16, V16, dtype=np.float32):
    """the unrounded pasted value [n][3] in `dtype` at crop coordinates (U16, V16) [n]: post_src at the taps, horizontal then vertical"""
    t = dtype
    src = (vae.astype(t) / t(2) + t(0.5)) * t(255)
    x0, x1, wx0, wx1 = _taps(U16, S)
    y0, y1, wy0, wy1 = _taps(V16, S)
    fx0, fx1, fy0, fy1 = (w.astype(t) / t(65536) for w in (wx0, wx1, wy0, wy1))
    r0 = src[:, y0, x0] * fx0 + src[:, y0, x1] * fx1
    r1 = src[:, y1, x0] * fx0 + src[:, y1, x1] * fx1
    return (r0 * fy0 + r1 * fy1).T


def paste_page(page, qs, vaes, S, dtype=np.float32, faults=()):
    """One page, its items `qs` in table order and their decoder outputs `vaes` ([3][S][S] each) -> dict(out: uint8 [H][W][3]; union:
    uint8 [H][W]; pasted: bool [H][W]; hit: int [H][W], the deciding item or -1; value: `dtype` [H][W][3], the unrounded value where
    pasted; clamped: bool [H][W], a tap of the pasted value was moved onto the crop's border)"""
    H, W, _ = page.shape
    Y, X = np.meshgrid(np.arange(H, dtype=I64), np.arange(W, dtype=I64), indexing="ij")
    hit = np.full((H, W), -1, np.int64)
    for b, q in enumerate(qs):
        cov = inside(q, X, Y, faults)
        if "first_wins" in faults:
            cov &= hit < 0
        hit[cov] = b
    out, pasted = page.copy(), np.zeros((H, W), bool)
    value, clamped = np.zeros((H, W, 3), dtype), np.zeros((H, W), bool)
    top = (I64(S) << 16) - 32768
    for b, q in enumerate(qs):
        U16, V16 = crop_coords(q, S, X, Y, faults)
        ok = (hit == b) & (U16 >= -32768) & (U16 < top) & (V16 >= -32768) & (V16 < top)
        if not ok.any():
            continue
        v = paste_value(vaes[b], S, U16[ok], V16[ok], dtype)
        value[ok] = v
        out[ok] = np.clip(np.rint(v), 0, 255).astype(np.uint8)
        pasted |= ok
        clamped[ok] = (U16[ok] < 0) | (U16[ok] > (I64(S - 1) << 16)) | (V16[ok] < 0) | (V16[ok] > (I64(S - 1) << 16))
    return dict(out=out, union=(hit >= 0).astype(np.uint8), pasted=pasted, hit=hit, value=value, clamped=clamped)


# ---- a page, its quads and frames turned by 90 degrees (np.rot90, counter-clockwise): pixel (X, Y) of a page of width W goes to (Y, W - 1 - X)
def rot90_page(page):
    return np.ascontiguousarray(np.rot90(page))


def rot90_corners(corners, W):
    return [(int(y), W - 1 - int(x)) for x, y in corners]


def rot90_frame(frame, W):
    cx2, cy2, cs, ux, uy = frame
    return (cy2, 2 * (W - 1) - cx2, cs, uy, -ux)
