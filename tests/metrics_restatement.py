"""What diffute_amd.metrics computes, restated in numpy (no torch, no scipy, no GPU).

ref64: the definition, in float64 - per channel the exact SSE and the mean SSIM of Wang et al. 2004 as scikit-image computes it with
gaussian_weights=True, sigma=1.5, use_sample_covariance=False, data_range=255 on the slice [y1:y2, x1:x2]: an 11-tap Gaussian (radius
int(3.5 * 1.5 + 0.5) = 5), the mean over the (h - 10) (w - 10) window centres whose window lies inside the box (scikit-image filters with a
reflected border and crops 5: the same numbers; test_metrics_host.py pins this against scipy.ndimage.gaussian_filter).  NaN where
min(h, w) < 11.

eval32: the kernel's formulation (csrc/metrics.hip), in float32 - tiles of TILE x TILE window centres counted from the box's corner, the
moments of a tile about an integer pivot (the rounded mean of `a` over the pixels the tile reads), the weights rounded to fp32, every
sum k = 0 .. 10 in order without contraction, one SSIM value per window in fp32, the mean over the box in fp64, rounded to fp32.  `fault`
injects one mistake.
Its distance from ref64 per box and channel is the FLOOR recorded in metrics_floors.py; the bound of the GPU test is bound(floor)."""
import numpy as np

TILE, WIN, R = 16, 11, 5
FAULTS = ("unpivoted", "sample_covariance", "sigma_1", "uniform_7x7", "k2_0.01", "data_range_1", "reflect_no_crop", "inclusive_corner",
          "window_reads_outside")


def weights64(sigma=1.5):
    g = [float(np.exp(-(float(i - R) ** 2) / (2.0 * sigma * sigma))) for i in range(WIN)]
    s = 0.0
    for v in g:
        s += v
    return np.array([v / s for v in g], dtype=np.float64)


def weights32():
    return weights64().astype(np.float32)


def _filter_valid(x, w):
    """the separable window as a valid convolution: along x, then along y; taps added in order"""
    h, wd = x.shape
    oh, ow = h - (WIN - 1), wd - (WIN - 1)
    acc = np.zeros((h, ow), dtype=x.dtype)
    for k in range(WIN):
        acc = acc + w[k] * x[:, k:k + ow]
    out = np.zeros((oh, ow), dtype=x.dtype)
    for k in range(WIN):
        out = out + w[k] * acc[k:k + oh, :]
    return out


def ssim_map(x, y, w, dtype, pivot=0, c1=(0.01 * 255.0) ** 2, c2=(0.03 * 255.0) ** 2, cov_norm=1.0):
    """x, y: integer arrays [h][w], h, w >= 11 -> the SSIM of every window inside them, [h - 10][w - 10] in `dtype`"""
    f = dtype
    xd, yd = (x.astype(np.int64) - pivot).astype(f), (y.astype(np.int64) - pivot).astype(f)
    w = w.astype(f)
    mx, my = _filter_valid(xd, w), _filter_valid(yd, w)
    sxx, syy, sxy = _filter_valid(xd * xd, w), _filter_valid(yd * yd, w), _filter_valid(xd * yd, w)
    vx, vy, vxy = sxx - mx * mx, syy - my * my, sxy - mx * my
    if cov_norm != 1.0:
        vx, vy, vxy = f(cov_norm) * vx, f(cov_norm) * vy, f(cov_norm) * vxy
    ux, uy = mx + f(pivot), my + f(pivot)
    a1, a2 = f(2) * ux * uy + f(c1), f(2) * vxy + f(c2)
    b1, b2 = ux * ux + uy * uy + f(c1), vx + vy + f(c2)
    out = (a1 * a2) / (b1 * b2)
    assert out.dtype == f
    return out


def sse(a, b, box):
    x1, y1, x2, y2 = box
    d = a[y1:y2, x1:x2].astype(np.int64) - b[y1:y2, x1:x2].astype(np.int64)
    return (d * d).sum((0, 1))


def ref64(a, b, box):
    """a, b: uint8 [H][W][3]; box (x1, y1, x2, y2) -> dict(n, sse int64 [3], ssim float64 [3])"""
    x1, y1, x2, y2 = box
    assert 0 <= x1 < x2 <= a.shape[1] and 0 <= y1 < y2 <= a.shape[0] and a.shape == b.shape
    sa, sb = a[y1:y2, x1:x2], b[y1:y2, x1:x2]
    ssim = np.full(3, np.nan)
    if min(sa.shape[:2]) >= WIN:
        w = weights64()
        ssim = np.array([ssim_map(sa[..., c], sb[..., c], w, np.float64).mean() for c in range(3)])
    return dict(n=(x2 - x1) * (y2 - y1), sse=sse(a, b, box), ssim=ssim)


def derived(n, sse3):
    """(mse, psnr) of one box as metrics.derive defines them"""
    mse = float(sse3.sum()) / (3.0 * n)
    return mse, (float("inf") if sse3.sum() == 0 else 10.0 * np.log10(255.0 ** 2 / mse))


def _tiled32(sa, sb, w, pivoted=True, **kw):
    """mean over the windows of one channel of a slice, tile by tile as the kernel goes"""
    h, wd = sa.shape
    oh, ow = h - (WIN - 1), wd - (WIN - 1)
    total = 0.0
    for ty in range(0, oh, TILE):
        for tx in range(0, ow, TILE):
            ra, rb = sa[ty:ty + TILE + WIN - 1, tx:tx + TILE + WIN - 1], sb[ty:ty + TILE + WIN - 1, tx:tx + TILE + WIN - 1]
            s = ssim_map(ra, rb, w, np.float32, pivot=(int(ra.sum()) + ra.size // 2) // ra.size if pivoted else 0, **kw)
            total += float(s.astype(np.float64).sum())
    return np.float32(total / (oh * ow))


def eval32(a, b, box, fault=None):
    """the kernel's formulation -> ssim float32 [3] (NaN where the box is too small); fault: None or one of FAULTS"""
    assert fault is None or fault in FAULTS
    H, W = a.shape[:2]
    x1, y1, x2, y2 = box
    if fault == "inclusive_corner":
        x2, y2 = min(x2 + 1, W), min(y2 + 1, H)
    if fault == "window_reads_outside":                       # every centre whose window touches the box, page pixels around it read
        x1, y1, x2, y2 = max(x1 - R, 0), max(y1 - R, 0), min(x2 + R, W), min(y2 + R, H)
    sa, sb = a[y1:y2, x1:x2], b[y1:y2, x1:x2]
    if fault == "reflect_no_crop":                            # scipy's `reflect` is numpy's `symmetric`
        sa, sb = (np.pad(s, ((R, R), (R, R), (0, 0)), mode="symmetric") for s in (sa, sb))
    if min(sa.shape[:2]) < WIN:
        return np.full(3, np.nan, dtype=np.float32)
    w, kw = weights32(), {}
    if fault == "sigma_1":
        w = weights64(1.0).astype(np.float32)
    if fault == "uniform_7x7":
        w = np.array([0, 0] + [1.0 / 7] * 7 + [0, 0], dtype=np.float32)
    if fault == "sample_covariance":
        kw["cov_norm"] = WIN * WIN / (WIN * WIN - 1.0)
    if fault == "k2_0.01":
        kw["c2"] = (0.01 * 255.0) ** 2
    if fault == "data_range_1":
        kw["c1"], kw["c2"] = 0.01 ** 2, 0.03 ** 2
    return np.array([_tiled32(sa[..., c], sb[..., c], w, pivoted=fault != "unpivoted", **kw) for c in range(3)], dtype=np.float32)


def bound(floor):
    """4 x floor: the kernel's summation order inside the window and across tiles differs from numpy's; 2^-22: the final mean and its
    rounding to fp32 at values near 1"""
    return 4.0 * floor + 2.0 ** -22


def ssim_ok(got, ref, floor):
    """one box, one channel"""
    if np.isnan(ref):
        return bool(np.isnan(got))
    return bool(abs(float(got) - float(ref)) <= bound(floor))


def outside_ref(a, b, boxes):
    """(changed, sse) over the pixels of one page that no box covers"""
    out = np.ones(a.shape[:2], dtype=bool)
    for x1, y1, x2, y2 in boxes:
        out[y1:y2, x1:x2] = False
    d = a.astype(np.int64) - b.astype(np.int64)
    return int(((d != 0).any(2) & out).sum()), int((d * d).sum(2)[out].sum())
