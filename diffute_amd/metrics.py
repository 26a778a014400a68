"""Comparing two versions of a set of pages on the device (csrc/metrics.hip): per text box MSE / PSNR / SSIM - what the scene-text-editing
literature reports, on exactly the edited box - and per page what changed OUTSIDE all boxes, the check of the paste kernels' promise that
a pixel no box covers is copied.

    m = diffute_amd.metrics.box_metrics_pages(pages_a, pages_b, locations)      # BoxMetrics of device tensors, one row per box, page-major
    o = diffute_amd.metrics.outside_diff_pages(originals, edited, locations)    # o.changed[p] == 0: the edit stayed inside its boxes

Pages are contiguous uint8 CUDA [h][w][3] tensors on one device, the two versions of a page of equal size; boxes are (x1, y1, x2, y2) and name
the slice [y1:y2, x1:x2] (exclusive upper corner, non-empty, inside the page: the read-back's convention, prepost.check_readback_boxes).
SSIM is scikit-image's structural_similarity(gaussian_weights=True, sigma=1.5, use_sample_covariance=False, data_range=255) per channel
on the slice.  Nothing here synchronises: the tables travel in one pinned staging buffer and one asynchronous copy, the results stay on the
device."""
import collections
import ctypes

import torch

from . import _cabi
from .prepost import check_readback_boxes_pages

# n: int64 [N] pixels of the box; sse: int64 [N,3] exact sum of (a - b)^2 per channel; ssim_rgb: fp32 [N,3] mean SSIM per channel (NaN where
# min(h, w) < 11); mse: fp64 [N] = sse.sum(1) / (3 n); psnr: fp64 [N] = 10 log10(255^2 / mse), inf where the SSE is 0; ssim: fp64 [N], the
# mean of the three channels (NaN where the box is too small)
BoxMetrics = collections.namedtuple("BoxMetrics", "n sse ssim_rgb mse psnr ssim")
# changed: int64 [P] pixels outside every box of the page whose bytes differ; sse: int64 [P] the sum of (a - b)^2 over them
OutsideDiff = collections.namedtuple("OutsideDiff", "changed sse")
_Tables = collections.namedtuple("_Tables", "pages boxes stage dbuf off_boxes off_n P B dev")


def _check_pairs(images_a, images_b, locations):
    """the arguments of every function here -> (pages a, pages b, the boxes flattened page-major, the pages' box counts, the device);
    ValueErrors name the page and the box"""
    images_a, images_b, locations = list(images_a), list(images_b), [list(l) for l in locations]
    P = len(images_a)
    if P == 0:
        raise ValueError("no pages: at least one pair of pages is needed")
    if len(images_b) != P or len(locations) != P:
        raise ValueError(f"{P} pages a, {len(images_b)} pages b, {len(locations)} lists of boxes: the lengths must agree")
    for p in range(P):
        for name, t in ((f"images_a[{p}]", images_a[p]), (f"images_b[{p}]", images_b[p])):
            if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.uint8 and t.is_contiguous()):
                raise ValueError(f"page {p}: {name} must be a contiguous uint8 CUDA tensor")
            if t.dim() != 3 or t.shape[2] != 3 or t.shape[0] < 1 or t.shape[1] < 1:
                raise ValueError(f"page {p}: {name} must be HWC with 3 channels")
            if t.device != images_a[0].device:
                raise ValueError(f"page {p}: {name} lives on {t.device}, images_a[0] on {images_a[0].device}: pages on several devices are not supported")
        if images_a[p].shape != images_b[p].shape:
            raise ValueError(f"page {p}: the two versions differ in size: {tuple(images_a[p].shape)} and {tuple(images_b[p].shape)}")
        for b, loc in enumerate(locations[p]):
            if len(loc) < 4:
                raise ValueError(f"page {p}: box {b}: expected (x1, y1, x2, y2)")
    flat = [loc for locs in locations for loc in locs]
    counts = [len(locs) for locs in locations]
    check_readback_boxes_pages(flat, counts, [t.shape[:2] for t in images_a])
    return images_a, images_b, flat, counts, images_a[0].device


def _upload(images_a, images_b, flat, counts, dev):
    """dmx_metric_page | dmx_metric_box | the boxes' pixel counts (int64), filled and validated in ONE pinned staging buffer, then ONE
    asynchronous copy on the current stream.  The entries read the host tables, the kernels the device copies."""
    P, B = len(images_a), len(flat)
    n_pages, n_boxes = P * ctypes.sizeof(_cabi.MetricPage), B * ctypes.sizeof(_cabi.MetricBox)
    stage = torch.empty(n_pages + n_boxes + 8 * B, dtype=torch.uint8, pin_memory=True)
    st = stage.numpy()
    pages = (_cabi.MetricPage * P).from_buffer(st[:n_pages])
    boxes = (_cabi.MetricBox * B).from_buffer(st[n_pages:n_pages + n_boxes]) if B else None
    n = st[n_pages + n_boxes:].view("int64")
    lo = 0
    for p, (pg, a, b, cnt) in enumerate(zip(pages, images_a, images_b, counts)):
        pg.a, pg.b, pg.H, pg.W, pg.box_lo, pg.box_hi = a.data_ptr(), b.data_ptr(), int(a.shape[0]), int(a.shape[1]), lo, lo + cnt
        for i in range(lo, lo + cnt):
            bx = boxes[i]
            bx.page = p
            bx.x1, bx.y1, bx.x2, bx.y2 = (int(v) for v in flat[i][:4])
            n[i] = (bx.x2 - bx.x1) * (bx.y2 - bx.y1)
        lo += cnt
    _cabi.check(_cabi.lib().dmx_metric_tables_prepare(pages, P, boxes, B), "metric_tables_prepare")
    with torch.cuda.device(dev):
        dbuf = torch.empty(stage.numel(), dtype=torch.uint8, device=dev)
        dbuf.copy_(stage, non_blocking=True)
    return _Tables(pages, boxes, stage, dbuf, n_pages, n_pages + n_boxes, P, B, dev)


def _box_metrics_raw(t, sse=None, ssim=None, lib=None, workspace=None):
    """the kernel's outputs for the tables `t`: (sse int64 [B,3], ssim fp32 [B,3]), written into the given tensors if any"""
    lib = _cabi.lib() if lib is None else lib
    base = t.dbuf.data_ptr()
    with torch.cuda.device(t.dev):
        sse = torch.empty(t.B, 3, dtype=torch.int64, device=t.dev) if sse is None else sse
        ssim = torch.empty(t.B, 3, dtype=torch.float32, device=t.dev) if ssim is None else ssim
        if workspace is None:
            workspace = torch.empty(max(int(lib.dmx_box_metrics_workspace_bytes(t.boxes, t.B)), 8), dtype=torch.uint8, device=t.dev)
        _cabi.check(lib.dmx_box_metrics_pages(t.pages, base, t.P, t.boxes, base + t.off_boxes, t.B, _cabi.ptr(sse), _cabi.ptr(ssim), _cabi.ptr(workspace),
                                              workspace.numel(), _cabi.current_stream()), "box_metrics_pages", lib)
    return sse, ssim


def _outside_diff_raw(t, out=None, lib=None):
    """the kernel's output for the tables `t`: int64 [P,2] = (changed, sse) per page, written into `out` if given"""
    lib = _cabi.lib() if lib is None else lib
    base = t.dbuf.data_ptr()
    with torch.cuda.device(t.dev):
        out = torch.empty(t.P, 2, dtype=torch.int64, device=t.dev) if out is None else out
        _cabi.check(lib.dmx_page_outside_diff(t.pages, base, t.P, t.boxes, (base + t.off_boxes) if t.B else None, t.B, _cabi.ptr(out),
                                              _cabi.current_stream()), "page_outside_diff", lib)
    return out


def derive(n, sse, ssim_rgb):
    """BoxMetrics from the kernel's outputs: torch arithmetic on whatever device they live on"""
    total = sse.sum(1).to(torch.float64)
    mse = total / (3 * n).to(torch.float64)
    psnr = torch.where(total == 0, torch.full_like(mse, float("inf")), 10.0 * torch.log10(255.0 ** 2 / mse))
    return BoxMetrics(n, sse, ssim_rgb, mse, psnr, ssim_rgb.to(torch.float64).mean(1))


def box_metrics_pages(images_a, images_b, locations):
    """MSE / PSNR / SSIM of every box between two versions of P pages, in one pass on the device.  images_a / images_b: P contiguous uint8
    CUDA [h_p][w_p][3] tensors on one device, the pair of a page of equal size; locations: P lists of boxes (x1, y1, x2, y2), a page's list
    may be empty.  Returns BoxMetrics with N rows, N the total box count, page-major as in edit_pages.  A box's row does not depend on
    the other boxes: it is bit-equal measured alone or in any batch."""
    a, b, flat, counts, dev = _check_pairs(images_a, images_b, locations)
    if not flat:
        raise ValueError("no boxes: box metrics need at least one")
    t = _upload(a, b, flat, counts, dev)
    sse, ssim = _box_metrics_raw(t)
    return derive(t.dbuf[t.off_n:].view(torch.int64), sse, ssim)


def box_metrics(image_a, image_b, locations):
    """box_metrics_pages for one page: the same path, the same bits"""
    return box_metrics_pages([image_a], [image_b], [locations])


def outside_diff_pages(images_a, images_b, locations):
    """Per page, what differs between the two versions OUTSIDE all of that page's boxes: OutsideDiff(changed int64 [P] - pixels whose three
    bytes are not all equal -, sse int64 [P] - the sum of (a - b)^2 over them).  Arguments as for box_metrics_pages; a page without boxes
    counts all its pixels.  After an edit, `changed` must be 0 everywhere: a pixel no box covers is copied."""
    a, b, flat, counts, dev = _check_pairs(images_a, images_b, locations)
    out = _outside_diff_raw(_upload(a, b, flat, counts, dev))
    return OutsideDiff(out[:, 0], out[:, 1])


def outside_diff(image_a, image_b, locations):
    """outside_diff_pages for one page: the same path, the same bits"""
    return outside_diff_pages([image_a], [image_b], [locations])
