"""Test-local restatement of Pillow's 8-bit resample (src/libImaging/Resample.c as published: precompute_coeffs,
normalize_coeffs_8bpc, ImagingResampleHorizontal_8bpc / Vertical_8bpc, ImagingResampleInner) and of the float arithmetic that
transformers' numpy image path (image_transforms.rescale / normalize) applies afterwards.  Pure numpy and Python floats, the C written
out literally one output index at a time (not through the product's vectorised table builder), so the product's tables and kernel are
checked against the published algorithm in its operation order."""
import math

import numpy as np

BILINEAR, BICUBIC = 2, 3
PRECISION_BITS = 32 - 8 - 2


def bilinear_filter(x):
    if x < 0.0:
        x = -x
    if x < 1.0:
        return 1.0 - x
    return 0.0


def bicubic_filter(x):
    a = -0.5
    if x < 0.0:
        x = -x
    if x < 1.0:
        return ((a + 2.0) * x - (a + 3.0)) * x * x + 1
    if x < 2.0:
        return (((x - 5) * x + 8) * x - 4) * a
    return 0.0


FILTERS = {BILINEAR: (bilinear_filter, 1.0), BICUBIC: (bicubic_filter, 2.0)}


def precompute_coeffs(in_size, out_size, resample):
    """-> ksize, bounds [(xmin, count)], kk [out][ksize] int (already through normalize_coeffs_8bpc)"""
    filt, filter_support = FILTERS[resample]
    filterscale = scale = float(in_size) / out_size
    if filterscale < 1.0:
        filterscale = 1.0
    support = filter_support * filterscale
    ksize = int(math.ceil(support)) * 2 + 1
    bounds, kk = [], []
    for xx in range(out_size):
        center = (xx + 0.5) * scale
        ww = 0.0
        ss = 1.0 / filterscale
        xmin = int(center - support + 0.5)            # C (int): truncation toward zero, like Python's int()
        if xmin < 0:
            xmin = 0
        xmax = int(center + support + 0.5)
        if xmax > in_size:
            xmax = in_size
        xmax -= xmin
        k = [0.0] * ksize
        for x in range(xmax):
            w = filt((x + xmin - center + 0.5) * ss)
            k[x] = w
            ww += w
        for x in range(xmax):
            if ww != 0.0:
                k[x] /= ww
        bounds.append((xmin, xmax))
        kk.append([int(-0.5 + v * (1 << PRECISION_BITS)) if v < 0 else int(0.5 + v * (1 << PRECISION_BITS)) for v in k])
    return ksize, bounds, kk


def clip8(v):
    """clip8(in) = clip8_lookups[in >> PRECISION_BITS]: arithmetic shift, then clamp to a byte"""
    return np.clip(v >> PRECISION_BITS, 0, 255).astype(np.uint8)


def resample_axis(img, out_size, resample, axis):
    """one pass over `axis` of a uint8 [H][W][C] image"""
    in_size = img.shape[axis]
    _, bounds, kk = precompute_coeffs(in_size, out_size, resample)
    src = np.moveaxis(img, axis, 0).astype(np.int64)
    out = np.empty((out_size,) + src.shape[1:], dtype=np.uint8)
    for xx, (xmin, n) in enumerate(bounds):
        ss = np.full(src.shape[1:], 1 << (PRECISION_BITS - 1), dtype=np.int64)
        for x in range(n):
            ss = ss + src[xmin + x] * kk[xx][x]
        assert np.abs(ss).max() < 2 ** 31, "Pillow accumulates in a 32-bit int"
        out[xx] = clip8(ss)
    return np.moveaxis(out, 0, axis)


def resize(img, size, resample=BILINEAR):
    """Image.resize((width, height), resample) of a uint8 [H][W][C] image: horizontal pass first, its result stored as bytes, then the
    vertical pass; a pass whose input and output size are equal is skipped."""
    assert img.dtype == np.uint8 and img.ndim == 3
    height, width = size
    out = img
    if out.shape[1] != width:
        out = resample_axis(out, width, resample, 1)
    if out.shape[0] != height:
        out = resample_axis(out, height, resample, 0)
    return np.ascontiguousarray(out)


def rescale_normalize(chw, do_rescale=True, rescale_factor=1 / 255, do_normalize=True, image_mean=(0.5, 0.5, 0.5),
                      image_std=(0.5, 0.5, 0.5)):
    """transformers' numpy path on a uint8 [C][H][W] image: rescale = upcast to float64, multiply, downcast to float32;
    normalize = (x - mean) / std in float32 with mean and std cast to float32 (a uint8 input is cast to float32 first)."""
    x = chw
    if do_rescale:
        x = (x.astype(np.float64) * rescale_factor).astype(np.float32)
    if do_normalize:
        if not np.issubdtype(x.dtype, np.floating):
            x = x.astype(np.float32)
        mean = np.array(image_mean, dtype=x.dtype)
        std = np.array(image_std, dtype=x.dtype)
        x = ((x.T - mean) / std).T
    return x.astype(np.float32)


def pixel_values(img_hwc, size=(384, 384), resample=BILINEAR, **norm):
    """-> (resized uint8 [3][h][w], pixel_values float32 [3][h][w])"""
    r = resize(img_hwc, size, resample).transpose(2, 0, 1)
    return r, rescale_normalize(r, **norm)
