"""On-device pre/post-processing around the denoise loop: the host mirror of the notebook's helper
functions (app.ipynb:370-383 mask, :674-720 crop ladder / origin, :722-745 resize + normalise, :776-779 latent mask,
:825-846 paste-back) over the HIP kernels in csrc/prepost.hip.  The uint8 image is uploaded once; the three network inputs
come out of one kernel and the result is pasted back by another - no PIL / cv2 / albumentations and no second PCIe hop."""
import collections
import ctypes

import numpy as np
import torch

from . import _cabi


def crop_scale_for(location, h, w):
    """crop-size ladder (app.ipynb:674-695)"""
    char_height = int(location[3] - location[1]); char_lenth = int(location[2] - location[0])
    short_side = min(h, w)
    crop_lenth = 6 * char_height
    for bound in (128, 256, 384, 512, 640, 784, 1000):
        if 6 * char_height < bound:
            crop_lenth = max(bound, char_lenth)
            break
    return min(crop_lenth, short_side) if char_lenth < crop_lenth else short_side


def crop_origin(location, crop_scale, w, rng=np.random):
    """crop origin (app.ipynb:701-720), including the reference's use of the image WIDTH in the y branch"""
    x1, y1, x2, y2 = (int(v) for v in location[:4])

    def pick(a1, a2):
        if a2 - a1 < crop_scale:
            if a2 - crop_scale > 0:
                return a2 - crop_scale
            return a1 if a1 + crop_scale < w else 0
        return int(rng.randint(a1, max(0, a2 - crop_scale - 1)))
    return pick(x1, x2), pick(y1, y2)


def _u8(t, name):
    if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.uint8 and t.is_contiguous()):
        raise TypeError(f"{name}: expected a contiguous uint8 CUDA tensor")
    return t


def generate_mask(h, w, location, device):
    """generate_mask (app.ipynb:370-378) on the device: uint8 [h][w], 1 inside the inclusive box"""
    mask = torch.empty(h, w, dtype=torch.uint8, device=device)
    x0, y0, x1, y1 = (int(v) for v in location[:4])
    _cabi.check(_cabi.lib().dmx_mask_rasterize(_cabi.ptr(mask), h, w, x0, y0, x1, y1, _cabi.current_stream()), "mask_rasterize")
    return mask


def preprocess(instance_image, location, x_s, y_s, crop_scale, size=512):
    """instance_image: uint8 CUDA tensor [h][w][3].  Returns dict(image, masked_image: fp32 [1,3,S,S] in [-1,1];
    mask: uint8 [1,1,S,S]; mask_latent: fp32 [1,1,S/8,S/8]; mask_full: uint8 [h][w])."""
    img = _u8(instance_image, "instance_image")
    h, w, c = img.shape
    if c != 3:
        raise ValueError("instance_image must be HWC with 3 channels")
    dev = img.device
    mask_full = generate_mask(h, w, location, dev)
    S = int(size)
    image = torch.empty(1, 3, S, S, dtype=torch.float32, device=dev)
    masked = torch.empty(1, 3, S, S, dtype=torch.float32, device=dev)
    mask = torch.empty(1, 1, S, S, dtype=torch.uint8, device=dev)
    mask_lat = torch.empty(1, 1, S // 8, S // 8, dtype=torch.float32, device=dev)
    _cabi.check(_cabi.lib().dmx_preprocess_crop(_cabi.ptr(img), _cabi.ptr(mask_full), h, w, int(x_s), int(y_s), int(crop_scale), S,
                                               _cabi.ptr(image), _cabi.ptr(masked), _cabi.ptr(mask), _cabi.ptr(mask_lat),
                                               _cabi.current_stream()), "preprocess_crop")
    return dict(image=image, masked_image=masked, mask=mask, mask_latent=mask_lat, mask_full=mask_full)


def postprocess(image_vae, instance_image, location, x_s, y_s, crop_scale):
    """image_vae: fp32 CUDA [1,3,S,S] (or [3,S,S]) decoder output in [-1,1]; returns the uint8 [h][w][3] result with the
    text box replaced (app.ipynb:825-846)."""
    img = _u8(instance_image, "instance_image")
    h, w, _ = img.shape
    v = image_vae.reshape(-1, image_vae.shape[-2], image_vae.shape[-1])
    if v.shape[0] != 3 or v.shape[1] != v.shape[2]:
        raise ValueError("image_vae must be one square 3-channel image")
    v = v.to(torch.float32).contiguous()
    out = torch.empty_like(img)
    x1, y1, x2, y2 = (int(t) for t in location[:4])
    _cabi.check(_cabi.lib().dmx_postprocess_paste(_cabi.ptr(v), int(v.shape[-1]), _cabi.ptr(img), _cabi.ptr(out), h, w, int(x_s), int(y_s),
                                                 int(crop_scale), x1, y1, x2, y2, _cabi.current_stream()), "postprocess_paste")
    return out


# ------------------------------------------------------------------------------------------------ several boxes per launch, on one page or on several
def plan_edits(locations, h, w, rng=np.random):
    """crop_scale_for + crop_origin for every box of one h x w image: [(x_s, y_s, crop_scale), ...].  Boxes that need a random origin draw
    from `rng` in box order, so a seeded rng gives what one text_editing() call per box would draw."""
    plans = []
    for loc in locations:
        crop_scale = crop_scale_for(loc, h, w)
        x_s, y_s = crop_origin(loc, crop_scale, w, rng)
        plans.append((x_s, y_s, crop_scale))
    return plans


def plan_pages(locations, sizes, rng=np.random):
    """plan_edits page after page on ONE rng stream: locations is a list of P lists of boxes, sizes the pages' (h, w).  Returns P lists
    of (x_s, y_s, crop_scale); a seeded rng draws exactly what one text_editing() call per box, page after page, would draw."""
    locations, sizes = list(locations), list(sizes)
    if len(locations) != len(sizes):
        raise ValueError(f"{len(locations)} lists of boxes, {len(sizes)} page sizes: the lengths must agree")
    return [plan_edits(locs, int(h), int(w), rng) for locs, (h, w) in zip(locations, sizes)]


# "the boxes of this call", whichever form the caller used: images - the page tensors, on the device dev; locations / origins /
# crop_scales - one entry per box, flattened page-major; counts - the pages' box counts; paged - the caller passed lists of pages, so
# the *_pages entries run and lists come back (a one-page call holds one image and runs the one-page entries).
_Boxes = collections.namedtuple("_Boxes", "images dev locations origins crop_scales counts paged")


def _check_items(locations, origins, crop_scales):
    """the list half of the batched functions' arguments, checked before anything touches a tensor"""
    locations, origins, crop_scales = list(locations), list(origins), list(crop_scales)
    B = len(locations)
    if B == 0:
        raise ValueError("no boxes: the batched pre/post-processing needs at least one")
    if B > _cabi.EDIT_MAX_ITEMS:
        raise ValueError(f"{B} boxes in one launch, at most {_cabi.EDIT_MAX_ITEMS}")
    if len(origins) != B or len(crop_scales) != B:
        raise ValueError(f"{B} boxes, {len(origins)} origins, {len(crop_scales)} crop scales: the lengths must agree")
    return locations, origins, crop_scales


def _check_pages(images, locations, origins, crop_scales):
    """the list half of the *_pages functions' arguments, checked before anything touches a tensor.  Returns (images, the three lists
    flattened page-major, the pages' box counts)."""
    images, locations, origins, crop_scales = list(images), list(locations), list(origins), list(crop_scales)
    P = len(images)
    if P == 0:
        raise ValueError("no pages: the paged pre/post-processing needs at least one")
    if P > _cabi.EDIT_MAX_ITEMS:
        raise ValueError(f"{P} pages in one launch, at most {_cabi.EDIT_MAX_ITEMS}")
    if len(locations) != P or len(origins) != P or len(crop_scales) != P:
        raise ValueError(f"{P} pages, {len(locations)} lists of boxes, {len(origins)} of origins, {len(crop_scales)} of crop scales: the lengths must agree")
    flat, counts = ([], [], []), []
    for p in range(P):
        locs, orgs, crops = list(locations[p]), list(origins[p]), list(crop_scales[p])
        if not locs:
            raise ValueError(f"page {p}: no boxes; every page needs at least one")
        if len(orgs) != len(locs) or len(crops) != len(locs):
            raise ValueError(f"page {p}: {len(locs)} boxes, {len(orgs)} origins, {len(crops)} crop scales: the lengths must agree")
        flat[0].extend(locs); flat[1].extend(orgs); flat[2].extend(crops)
        counts.append(len(locs))
    if len(flat[0]) > _cabi.EDIT_MAX_ITEMS:
        raise ValueError(f"{len(flat[0])} boxes in one launch, at most {_cabi.EDIT_MAX_ITEMS}")
    return (images,) + flat + (counts,)


def _check_page_images(images):
    """P contiguous uint8 CUDA [h][w][3] tensors on one device -> that device"""
    for p, img in enumerate(images):
        _u8(img, f"images[{p}]")
        if img.dim() != 3 or img.shape[2] != 3:
            raise ValueError(f"images[{p}] must be HWC with 3 channels")
        if img.device != images[0].device:
            raise ValueError(f"images[{p}] lives on {img.device}, images[0] on {images[0].device}: pages on several devices are not supported")
    return images[0].device


def _resizing_processor(processor, what):
    """the image processor of a read-back - a ViTImageProcessor, or the one inside a TrOCRProcessor -, refused unless it resizes; like the
    lists it is checked before any tensor is looked at"""
    ip = getattr(processor, "image_processor", processor)
    if not ip.do_resize:
        raise ValueError(f"{what}: the processor must resize (do_resize=True): boxes have no common size")
    return ip


def _one_page(instance_image, locations, origins, crop_scales):
    """the boxes of a one-page call: the lists are checked before the tensor is looked at"""
    locations, origins, crop_scales = _check_items(locations, origins, crop_scales)
    img = _u8(instance_image, "instance_image")
    if img.dim() != 3 or img.shape[2] != 3:
        raise ValueError("instance_image must be HWC with 3 channels")
    return _Boxes([img], img.device, locations, origins, crop_scales, [len(locations)], False)


def _paged(images, locations, origins, crop_scales):
    """the boxes of a paged call: the lists are checked before any tensor is looked at"""
    images, locations, origins, crop_scales, counts = _check_pages(images, locations, origins, crop_scales)
    return _Boxes(images, _check_page_images(images), locations, origins, crop_scales, counts, True)


def _upload(bx, S, out=None, union=None, extra=()):
    """the tables of one launch - dmx_edit_item | dmx_edit_page (a paged call only; out / union: its pages' output tensors) | `extra`
    (numpy arrays) - filled and validated in ONE pinned staging buffer, then ONE asynchronous copy on the current stream.  Returns (host
    items, host pages or None, the pinned storage, the device buffer, the byte offsets of the pages and of every extra array in it):
    the entries read the host tables, the kernels the device copies."""
    B, P = len(bx.locations), len(bx.images) if bx.paged else 0
    n_items, n_pages = B * ctypes.sizeof(_cabi.EditItem), P * ctypes.sizeof(_cabi.EditPage)
    offs, total = [], n_items + n_pages
    for a in extra:
        offs.append(total); total += a.nbytes
    stage = torch.empty(total, dtype=torch.uint8, pin_memory=True)
    st = stage.numpy()
    host = (_cabi.EditItem * B).from_buffer(st[:n_items])
    for it, loc, (x_s, y_s), crop_scale in zip(host, bx.locations, bx.origins, bx.crop_scales):
        it.x1, it.y1, it.x2, it.y2 = (int(v) for v in loc[:4])
        it.x_s, it.y_s, it.crop_scale = int(x_s), int(y_s), int(crop_scale)
    if bx.paged:
        pages = (_cabi.EditPage * P).from_buffer(st[n_items:n_items + n_pages])
        lo = 0
        for p, (pg, img, n) in enumerate(zip(pages, bx.images, bx.counts)):
            pg.original = img.data_ptr()
            pg.out = out[p].data_ptr() if out is not None else 0
            pg.union_mask = union[p].data_ptr() if union is not None else 0
            pg.H, pg.W, pg.item_lo, pg.item_hi = int(img.shape[0]), int(img.shape[1]), lo, lo + n
            lo += n
        _cabi.check(_cabi.lib().dmx_edit_pages_prepare(pages, P, host, B, S), "edit_pages_prepare")
    else:
        pages = None
        _cabi.check(_cabi.lib().dmx_edit_items_prepare(host, B, int(bx.images[0].shape[0]), int(bx.images[0].shape[1]), S), "edit_items_prepare")
    for a, o in zip(extra, offs):
        st[o:o + a.nbytes] = np.ascontiguousarray(a).reshape(-1).view(np.uint8)
    with torch.cuda.device(bx.dev):
        dbuf = torch.empty(total, dtype=torch.uint8, device=bx.dev)
        dbuf.copy_(stage, non_blocking=True)                          # the one H2D copy
    return host, pages, stage, dbuf, [n_items] + offs


def _upload_pages(images, locations, origins, crop_scales, counts, S, dev, out=None, union=None, extra=()):
    """_upload of a paged call from its parts.  The tests build real tables through this function (tests/test_prepost_pages_gpu.py):
    arguments and the returned tuple stay as they are."""
    return _upload(_Boxes(images, dev, locations, origins, crop_scales, counts, True), S, out, union, extra)


def _check_vae(image_vae, B, candidates):
    """the decoder outputs of B boxes - [B,3,S,S], or with `candidates` [B,K,3,S,S] - -> (S, K); nothing is converted or copied here"""
    if not (isinstance(image_vae, torch.Tensor) and image_vae.is_cuda):
        raise TypeError("image_vae: expected a CUDA tensor")
    s = image_vae.shape
    if image_vae.dim() != (5 if candidates else 4) or s[0] != B or s[-3] != 3 or s[-2] != s[-1]:
        raise ValueError(f"image_vae must be [{B},K,3,S,S]: K square 3-channel candidates per box" if candidates else
                         f"image_vae must be [{B},3,S,S]: one square 3-channel image per box")
    K = int(s[1]) if candidates else 1
    if not 1 <= K <= _cabi.SELECT_MAX_CANDIDATES:
        raise ValueError(f"{K} candidates per box, expected 1 .. {_cabi.SELECT_MAX_CANDIDATES}")
    return int(s[-1]), K


def _check_page_outputs(out, images):
    """the optional `out` list of the paged pastes: P contiguous uint8 tensors of the pages' shapes on their device, sharing no memory with
    the pages or with one another (one launch reads every page and writes every output)"""
    out = list(out)
    if len(out) != len(images):
        raise ValueError(f"{len(images)} pages, {len(out)} output tensors: the lengths must agree")
    spans = [(t.data_ptr(), t.data_ptr() + t.numel(), f"images[{p}]") for p, t in enumerate(images)]
    for p, (o, img) in enumerate(zip(out, images)):
        if not (isinstance(o, torch.Tensor) and o.is_cuda and o.dtype == torch.uint8 and o.is_contiguous() and o.device == img.device
                and o.shape == img.shape):
            raise ValueError(f"out[{p}] must be a contiguous uint8 tensor {tuple(img.shape)} on {img.device}")
        lo, hi = o.data_ptr(), o.data_ptr() + o.numel()
        for a, z, name in spans:
            if lo < z and a < hi:
                raise ValueError(f"out[{p}] shares memory with {name}")
        spans.append((lo, hi, f"out[{p}]"))
    return out


def _page_outputs(images, dev, out, return_mask):
    """what a paste over `images` writes, as lists: (the output pages - `out` if given, checked -, the union masks or None)"""
    if out is not None:
        out = _check_page_outputs(out, images)
    with torch.cuda.device(dev):
        out = [torch.empty_like(img) for img in images] if out is None else out
        union = [torch.empty(img.shape[0], img.shape[1], dtype=torch.uint8, device=dev) for img in images] if return_mask else None
    return out, union


def _paste_outputs(bx, out, return_mask):
    """_page_outputs of the boxes' pages: lists for a paged call, the one page's tensors otherwise"""
    out, union = _page_outputs(bx.images, bx.dev, out, return_mask)
    return (out, union) if bx.paged else (out[0], None if union is None else union[0])


def _crop_outputs(B, S, dev):
    """what a crop of B regions writes, in the order the C entries take it (call it on the device)"""
    return dict(image=torch.empty(B, 3, S, S, dtype=torch.float32, device=dev), masked_image=torch.empty(B, 3, S, S, dtype=torch.float32, device=dev),
                mask=torch.empty(B, 1, S, S, dtype=torch.uint8, device=dev), mask_latent=torch.empty(B, 1, S // 8, S // 8, dtype=torch.float32, device=dev))


def _check_readback_outputs(out, out_resized, rows, S_h, S_w, dev):
    """the optional preallocated outputs of a read-back: contiguous [rows,3,S_h,S_w] on dev, fp32 and uint8"""
    for name, t, dt in (("out", out, torch.float32), ("out_resized", out_resized, torch.uint8)):
        if t is not None and not (isinstance(t, torch.Tensor) and t.device == dev and t.dtype == dt and t.is_contiguous()
                                  and tuple(t.shape) == (rows, 3, S_h, S_w)):
            raise ValueError(f"{name} must be a contiguous {dt} tensor [{rows},3,{S_h},{S_w}] on {dev}")


def _call_boxes(name, bx, tables, head, *tail, outs=(), choice=()):
    """dmx_<name>(*head, the page part, the item table - host and device -, B, *tail, stream) on the current stream, `tables` being what
    _upload returned.  The page part of a one-page call is `img, *outs, *choice, H, W` - outs: the (out, union) a paste writes; choice: the
    select paste's, which the C signature has there.  A paged call runs dmx_<name>_pages (for dmx_<name>_batch) and its page part is
    `*choice, pages_host, pages_device, P`: the outputs travel in the page table."""
    host, pages, _, dbuf, offs = tables
    base, img, lib = dbuf.data_ptr(), bx.images[0], _cabi.lib()
    if bx.paged:
        name, page = name.removesuffix("_batch") + "_pages", (*choice, pages, base + offs[0], len(bx.images))
    else:
        page = (_cabi.ptr(img), *map(_cabi.ptr, outs), *choice, img.shape[0], img.shape[1])
    _cabi.check(getattr(lib, "dmx_" + name)(*head, *page, host, base, len(host), *tail, _cabi.current_stream()), name, lib)


def _preprocess(bx, size):
    B, S = len(bx.locations), int(size)
    tables = _upload(bx, S)
    with torch.cuda.device(bx.dev):
        pre = _crop_outputs(B, S, bx.dev)
        _call_boxes("preprocess_crop_batch", bx, tables, (), S, *map(_cabi.ptr, pre.values()))
    return pre


class PasteBlend:
    """How the batched pastes put a generated patch onto the page (include/diffute_hip.h dmx_paste_blend; integers throughout):
    feather - the width f of the linear ramp at the edge of the paste rectangle: the weight of the patch is min(d + 1, f + 1) / (f + 1)
              at distance d from the rectangle's edge (0 on the edge), so f = 0 is a hard edge;
    grow - the paste rectangle is the box grown by g pixels on every side (clipped to the crop).  With grow >= feather the whole box is
              fully generated and the ramp lies around it - the setting for tight OCR boxes; with grow = 0 the ramp lies INSIDE the box;
    match_color - shift every channel of the patch by the mean difference between the original page and the patch over a ring of
              `ring` pixels around the paste rectangle, at most `max_shift` levels (a mean shift of bytes: no gain, no gamma).
    PasteBlend() - all off - pastes what blend=None pastes, bit for bit.  For boxes only: quads take a QuadBlend, whose ramp is measured
    perpendicular to the quad's edges (edit_quads refuses a PasteBlend)."""
    __slots__ = ("feather", "grow", "match_color", "ring", "max_shift")

    def __init__(self, feather=0, grow=0, match_color=False, ring=8, max_shift=32):
        cap = _cabi.PASTE_BLEND_MAX
        for name, v, lo, hi in (("feather", feather, 0, cap), ("grow", grow, 0, cap), ("ring", ring, 1, cap), ("max_shift", max_shift, 0, 255)):
            if isinstance(v, bool) or not isinstance(v, (int, np.integer)):
                raise TypeError(f"PasteBlend: {name} must be an integer, got {v!r}")
            if not lo <= v <= hi:
                raise ValueError(f"PasteBlend: {name} = {v}, expected {lo} .. {hi}")
        if not isinstance(match_color, (bool, np.bool_)):
            raise TypeError(f"PasteBlend: match_color must be a bool, got {match_color!r}")
        self.feather, self.grow, self.match_color, self.ring, self.max_shift = int(feather), int(grow), bool(match_color), int(ring), int(max_shift)

    def __repr__(self):
        return (f"PasteBlend(feather={self.feather}, grow={self.grow}, match_color={self.match_color}, ring={self.ring}, "
                f"max_shift={self.max_shift})")

    def grown(self, locations, h=None, w=None):
        """the boxes grown by `grow` - every paste rectangle lies inside its grown box - as [(x1, y1, x2, y2)], clipped to an h x w page if
        the size is given: what metrics.outside_diff takes to show that nothing outside the paste rectangles changed"""
        g, out = self.grow, []
        for loc in locations:
            x1, y1, x2, y2 = (int(v) for v in loc[:4])
            x1, y1, x2, y2 = x1 - g, y1 - g, x2 + g, y2 + g
            if w is not None:
                x1, x2 = max(x1, 0), min(x2, int(w))
            if h is not None:
                y1, y2 = max(y1, 0), min(y2, int(h))
            out.append((x1, y1, x2, y2))
        return out

    def _struct(self):
        return _cabi.PasteBlend(self.feather, self.grow, self.ring, self.max_shift, int(self.match_color))


def _check_blend(blend):
    if not isinstance(blend, PasteBlend):
        raise TypeError(f"blend: expected a PasteBlend or None, got {type(blend).__name__}")
    return blend


def _check_scores_tensor(scores):
    if not (isinstance(scores, torch.Tensor) and scores.is_cuda):
        raise TypeError("scores: expected a CUDA tensor")


def _check_scores(scores, B, K, threshold):
    """scores [B,K] on the device and the threshold -> the threshold as the C entries take it (None: -inf)"""
    _check_scores_tensor(scores)
    if tuple(scores.shape) != (B, K):
        raise ValueError(f"scores must be [{B},{K}], got {tuple(scores.shape)}")
    thr = float("-inf") if threshold is None else float(threshold)
    if thr != thr:
        raise ValueError("threshold is NaN")
    return thr


def _choose(lib, scores, B, K, thr, dev):
    """choice int32 [B] on the device from scores [B,K], by the rule of the select pastes (dmx_select_choices: a launch of its own)"""
    sc = scores.to(torch.float32).contiguous()
    choice = torch.empty(B, dtype=torch.int32, device=dev)
    _cabi.check(lib.dmx_select_choices(_cabi.ptr(sc), B, K, thr, _cabi.ptr(choice), _cabi.current_stream()), "select_choices", lib)
    return choice


def _color_stats(bx, tables, v, S, K, choice, bs):
    """stats int64 [B,4] on the device: one launch, one block per item"""
    stats = torch.empty(len(bx.locations), 4, dtype=torch.int64, device=bx.dev)
    _call_boxes("paste_color_stats", bx, tables, (_cabi.ptr(v), S), ctypes.byref(bs), _cabi.ptr(choice), K, _cabi.ptr(stats))
    return stats


def _blend_paste(bx, image_vae, blend, return_mask, out, scores=None, threshold=None):
    """the blended pastes: [choose ->] [stats ->] paste, every launch on the current stream, nothing read on the host.  scores given:
    image_vae is [B,K,3,S,S] and (out, choice[, union]) comes back, as from the select pastes"""
    blend = _check_blend(blend)
    B, select = len(bx.locations), scores is not None
    S, K = _check_vae(image_vae, B, select)
    thr = _check_scores(scores, B, K, threshold) if select else None
    out, union = _paste_outputs(bx, out, return_mask)
    v = image_vae.to(torch.float32).contiguous()
    tables, bs = _upload(bx, S, out, union), blend._struct()
    with torch.cuda.device(bx.dev):
        choice = _choose(_cabi.lib(), scores, B, K, thr, bx.dev) if select else None
        stats = _color_stats(bx, tables, v, S, K, choice, bs) if blend.match_color else None
        _call_boxes("postprocess_paste_blend", bx, tables, (_cabi.ptr(v), S), ctypes.byref(bs), _cabi.ptr(stats), _cabi.ptr(choice), K, outs=(out, union))
    if select:
        return (out, choice, union) if return_mask else (out, choice)
    return (out, union) if return_mask else out


def _stats_only(bx, image_vae, blend, choice):
    blend = _check_blend(blend)
    B = len(bx.locations)
    S, K = _check_vae(image_vae, B, choice is not None)
    _check_choice(choice, B)
    v = image_vae.to(torch.float32).contiguous()
    tables = _upload(bx, S)
    with torch.cuda.device(bx.dev):
        return _color_stats(bx, tables, v, S, K, choice, blend._struct())


def _paste(bx, image_vae, return_mask, out):
    S, _ = _check_vae(image_vae, len(bx.locations), False)
    out, union = _paste_outputs(bx, out, return_mask)
    v = image_vae.to(torch.float32).contiguous()
    tables = _upload(bx, S, out, union)
    with torch.cuda.device(bx.dev):
        _call_boxes("postprocess_paste_batch", bx, tables, (_cabi.ptr(v), S), outs=(out, union))
    return (out, union) if return_mask else out


def check_readback_boxes(locations, h, w):
    """what the read-back needs of the boxes beyond the batched paste's checks: the slice [y1:y2, x1:x2] is non-empty and inside the image"""
    for b, loc in enumerate(locations):
        x1, y1, x2, y2 = (int(v) for v in loc[:4])
        if x2 <= x1 or y2 <= y1:
            raise ValueError(f"box {b}: ({x1}, {y1}, {x2}, {y2}) is empty; the OCR read-back needs at least one pixel")
        if x1 < 0 or y1 < 0 or x2 > w or y2 > h:
            raise ValueError(f"box {b}: ({x1}, {y1}, {x2}, {y2}) lies outside the {w}x{h} image")


def check_readback_boxes_pages(locations, counts, sizes):
    """check_readback_boxes page by page: locations flattened page-major, counts the pages' box counts, sizes their (h, w)"""
    lo = 0
    for p, (n, (h, w)) in enumerate(zip(counts, sizes)):
        try:
            check_readback_boxes(locations[lo:lo + n], int(h), int(w))
        except ValueError as e:
            raise ValueError(f"page {p}: {e}") from None
        lo += n


def _readback_tables(locations, ip, cap, what="box"):
    """per box the two resample tables of (box width -> S_w) and (box height -> S_h), deduplicated: (passes [B][4] int32, the concatenated
    int32 tables, max_taps).  A pass with equal sizes is skipped (offset -1), as Pillow does.  what: how the error names a region (the
    quad read-back passes the pseudo-boxes (0, 0, rw, rh) of its strips)."""
    from . import processing
    S_h, S_w = ip.size["height"], ip.size["width"]
    passes = np.zeros((len(locations), 4), dtype=np.int32)
    tables, table_off, n_ints, max_taps = [], {}, 0, 0
    for b, loc in enumerate(locations):
        x1, y1, x2, y2 = (int(v) for v in loc[:4])
        for col, (n_in, n_out) in ((0, (x2 - x1, S_w)), (2, (y2 - y1, S_h))):
            if n_in == n_out:
                passes[b, col], passes[b, col + 1] = -1, 0
                continue
            taps = processing._taps(n_in, n_out, ip.resample)
            if taps > cap:
                raise ValueError(f"{what} {b}: resizing {n_in} -> {n_out} needs {taps} taps per output pixel, more than the kernel's cap of {cap} "
                                 "(downscale ratio at most 31 for bilinear, 15 for bicubic)")
            k = (n_in, n_out, ip.resample)
            if k not in table_off:
                t = processing.resample_table(*k)
                table_off[k] = n_ints; tables.append(t); n_ints += t.size
            passes[b, col], passes[b, col + 1] = table_off[k], taps
            max_taps = max(max_taps, taps)
    return passes, (np.concatenate(tables) if tables else np.zeros(0, dtype=np.int32)), max_taps


def _readback(bx, image_vae, ip, return_resized, out, out_resized):
    B, img = len(bx.locations), bx.images[0]
    S, K = _check_vae(image_vae, B, True)
    if bx.paged:
        check_readback_boxes_pages(bx.locations, bx.counts, [i.shape[:2] for i in bx.images])
    else:
        check_readback_boxes(bx.locations, img.shape[0], img.shape[1])
    S_h, S_w = ip.size["height"], ip.size["width"]
    _check_readback_outputs(out, out_resized, B * K, S_h, S_w, bx.dev)
    passes, tables, max_taps = _readback_tables(bx.locations, ip, int(_cabi.lib().dmx_glyph_max_taps()))
    v = image_vae.to(torch.float32).contiguous()
    up = _upload(bx, S, extra=(passes, ip._norm, tables))
    _, _, stage, dbuf, (_, off_pass, off_norm, off_tab) = up
    host_passes = (_cabi.ReadbackPass * B).from_buffer(stage.numpy()[off_pass:off_norm])
    base = dbuf.data_ptr()
    with torch.cuda.device(bx.dev):
        if out is None:
            out = torch.empty(B * K, 3, S_h, S_w, dtype=torch.float32, device=bx.dev)
        res = out_resized
        if res is None and return_resized:
            res = torch.empty(B * K, 3, S_h, S_w, dtype=torch.uint8, device=bx.dev)
        _call_boxes("readback_pixel_values", bx, up, (_cabi.ptr(v), S), K, base + off_tab, int(tables.size), base + off_norm, host_passes,
                    base + off_pass, max_taps, S_h, S_w, _cabi.ptr(out), _cabi.ptr(res))
    return (out, res) if (return_resized or out_resized is not None) else out


def _select_paste(bx, image_vae, scores, threshold, return_mask, out):
    B = len(bx.locations)
    _check_scores_tensor(scores)                                       # (before image_vae is looked at, the rest after)
    S, K = _check_vae(image_vae, B, True)
    thr = _check_scores(scores, B, K, threshold)
    out, union = _paste_outputs(bx, out, return_mask)
    v, sc = image_vae.to(torch.float32).contiguous(), scores.to(torch.float32).contiguous()
    tables = _upload(bx, S, out, union)
    with torch.cuda.device(bx.dev):
        choice = torch.empty(B, dtype=torch.int32, device=bx.dev)
        _call_boxes("postprocess_paste_select", bx, tables, (_cabi.ptr(v), S, _cabi.ptr(sc), thr), K, outs=(out, union), choice=(_cabi.ptr(choice),))
    return (out, choice, union) if return_mask else (out, choice)


# ---- the public functions: each builds the description of its boxes and calls the body above; a one-page function runs the one-page
# entry of the C-ABI and returns tensors, a paged one the *_pages entry and returns lists
def preprocess_batch(instance_image, locations, origins, crop_scales, size=512):
    """B boxes of one image in one launch.  instance_image: uint8 CUDA tensor [h][w][3]; locations: B boxes (x1, y1, x2, y2); origins: B
    crop origins (x_s, y_s); crop_scales: B crop sides (plan_edits gives the last two).  Returns dict(image, masked_image: fp32
    [B,3,S,S] in [-1,1]; mask: uint8 [B,1,S,S]; mask_latent: fp32 [B,1,S/8,S/8]); row b equals preprocess() of box b, whose mask holds
    that box alone.  No [h][w] mask is built."""
    return _preprocess(_one_page(instance_image, locations, origins, crop_scales), size)


def preprocess_pages(images, locations, origins, crop_scales, size=512):
    """preprocess_batch for boxes on SEVERAL pages, in one launch.  images: P contiguous uint8 CUDA [h_p][w_p][3] tensors on one device;
    locations / origins / crop_scales: P lists, one entry per box of that page (plan_pages gives the last two).  Returns the
    preprocess_batch dict with N rows, N the total box count, page-major (page 0's boxes in order, then page 1's): row b equals
    preprocess() of box b on its own page."""
    return _preprocess(_paged(images, locations, origins, crop_scales), size)


def postprocess_batch(image_vae, instance_image, locations, origins, crop_scales, return_mask=False, blend=None):
    """image_vae: fp32 CUDA [B,3,S,S] decoder outputs in [-1,1], one per box; returns the uint8 [h][w][3] image that B chained
    postprocess() calls in box order leave (a later box wins where boxes overlap), in one launch.  return_mask=True also returns the
    union of the boxes as uint8 [h][w] in {0, 1} (the app shows mask * 255).
    blend: None - the hard paste above -, or a PasteBlend: feathered edge and / or colour match ([stats ->] blended paste, one launch
    each; the chain of single blended pastes in box order).  The mask is then the union of the PASTE RECTANGLES (half-open, the boxes
    grown by blend.grow and clipped to their crops): the result equals the original wherever it is 0."""
    bx = _one_page(instance_image, locations, origins, crop_scales)
    return _paste(bx, image_vae, return_mask, None) if blend is None else _blend_paste(bx, image_vae, blend, return_mask, None)


def postprocess_pages(image_vae, images, locations, origins, crop_scales, return_mask=False, out=None, blend=None):
    """postprocess_batch for boxes on several pages, in one launch.  image_vae: fp32 CUDA [N,3,S,S] decoder outputs, page-major; the
    other arguments as for preprocess_pages.  Returns the list of P uint8 [h_p][w_p][3] pages - page p is postprocess_batch of its own
    boxes (a later box wins where boxes overlap) -, with return_mask=True also the list of P union masks uint8 [h_p][w_p].  out
    (optional): a list of P preallocated contiguous uint8 tensors of the pages' shapes, distinct from `images`, to write into.
    blend: as for postprocess_batch."""
    bx = _paged(images, locations, origins, crop_scales)
    return _paste(bx, image_vae, return_mask, out) if blend is None else _blend_paste(bx, image_vae, blend, return_mask, out)


def paste_color_stats(image_vae, instance_image, locations, origins, crop_scales, blend, choice=None):
    """The colour statistics a blended paste with blend.match_color uses, int64 CUDA [B,4]: per box n - the pixels of the ring of
    blend.ring pixels around its paste rectangle, inside its crop - and D_r, D_g, D_b - the sums over the ring of (original - generated
    byte), clamped to +- blend.max_shift * n.  Read from the ORIGINAL page and the box's own decoder output: a box's numbers do not depend
    on the other boxes.  image_vae: [B,3,S,S], or with choice (int32 CUDA [B], -1 = skipped: zeros) [B,K,3,S,S]."""
    return _stats_only(_one_page(instance_image, locations, origins, crop_scales), image_vae, blend, choice)


def paste_color_stats_pages(image_vae, images, locations, origins, crop_scales, blend, choice=None):
    """paste_color_stats for boxes on several pages: int64 CUDA [N,4], page-major, every box against its own page"""
    return _stats_only(_paged(images, locations, origins, crop_scales), image_vae, blend, choice)


def readback_pixel_values(image_vae, instance_image, locations, origins, crop_scales, processor, return_resized=False, out=None, out_resized=None):
    """The OCR model's input for K candidates of each of B boxes, in ONE launch: image_vae fp32 CUDA [B,K,3,S,S] decoder outputs ->
    pixel_values fp32 [B*K,3,S_h,S_w], box-major.  Row (b, k) is bit for bit `processor(postprocess(image_vae[b, k], instance_image,
    box b)[y1:y2, x1:x2])` - the reference's read-back (app.ipynb:842-846) - without the page, the slice or the processor call.
    processor: a ViTImageProcessor or TrOCRProcessor with do_resize; its tables travel in one pinned staging buffer, one H2D copy.
    return_resized=True also returns the uint8 [B*K,3,S_h,S_w] bytes before rescale / normalise.  out / out_resized (optional): contiguous
    CUDA tensors of those shapes to write into."""
    ip = _resizing_processor(processor, "readback_pixel_values")
    return _readback(_one_page(instance_image, locations, origins, crop_scales), image_vae, ip, return_resized, out, out_resized)


def readback_pixel_values_pages(image_vae, images, locations, origins, crop_scales, processor, return_resized=False, out=None, out_resized=None):
    """readback_pixel_values for boxes on several pages, in one launch: image_vae fp32 CUDA [N,K,3,S,S], page-major -> pixel_values fp32
    [N*K,3,S_h,S_w]; row (b, k) is the read-back of candidate k of box b on its own page.  The items, the pages and the processor's
    tables travel in one pinned staging buffer, one H2D copy.  return_resized / out / out_resized as for readback_pixel_values."""
    ip = _resizing_processor(processor, "readback_pixel_values_pages")
    return _readback(_paged(images, locations, origins, crop_scales), image_vae, ip, return_resized, out, out_resized)


def postprocess_select_batch(image_vae, scores, instance_image, locations, origins, crop_scales, threshold=None, return_mask=False, blend=None):
    """Choose and paste in ONE launch, without reading the scores on the host.  image_vae: fp32 CUDA [B,K,3,S,S]; scores: fp32 CUDA [B,K].
    choice[b] = arg-max over k of scores[b] (lowest k on a tie; a NaN never wins; 0 when every score is NaN), or -1 when the best score
    is below `threshold` (None: no threshold) - that box then keeps the original pixels.  Returns (out, choice): the uint8 [h][w][3] page
    postprocess_batch gives for the chosen rows over the boxes that were kept, and choice int32 [B] on the device; with return_mask=True
    also the union of ALL boxes as uint8 [h][w].
    blend: None, or a PasteBlend: choose -> [stats ->] blended paste of the chosen rows, one launch each and still no score read on the
    host; the mask is then the union of the paste rectangles of all boxes (postprocess_batch)."""
    bx = _one_page(instance_image, locations, origins, crop_scales)
    if blend is None:
        return _select_paste(bx, image_vae, scores, threshold, return_mask, None)
    return _blend_paste(bx, image_vae, blend, return_mask, None, scores, threshold)


def postprocess_select_pages(image_vae, scores, images, locations, origins, crop_scales, threshold=None, return_mask=False, out=None, blend=None):
    """postprocess_select_batch for boxes on several pages, in one launch: image_vae fp32 CUDA [N,K,3,S,S], scores fp32 CUDA [N,K], both
    page-major.  Returns (pages, choice): the list of P uint8 pages, page p being what postprocess_select_batch gives for its own boxes,
    and choice int32 [N] on the device, by the same rule; with return_mask=True also the list of P union masks.  out as for
    postprocess_pages.  blend: as for postprocess_select_batch."""
    bx = _paged(images, locations, origins, crop_scales)
    if blend is None:
        return _select_paste(bx, image_vae, scores, threshold, return_mask, out)
    return _blend_paste(bx, image_vae, blend, return_mask, out, scores, threshold)


# ------------------------------------------------------------------------------------------------ quadrilateral regions, oriented crops
# (csrc/prepost_quad.hip; the arithmetic is stated in csrc/prepost_quad.h).  A quad is four corners (x, y) - top-left, top-right,
# bottom-right, bottom-left of the text as read, clockwise with y down -, a frame is (cx2, cy2, crop_scale, ux, uy): the crop's centre in
# half-pixels of pixel-index space, its side in page pixels and the direction of its x axis.
def _corners(quad):
    """a quad as given - 4 x (x, y) or 8 numbers - -> [[x, y]] * 4 of ints"""
    c = np.asarray(quad).reshape(-1)
    if c.size != 8:
        raise ValueError(f"a quad is four corners (x, y): TL, TR, BR, BL; got {c.size} numbers")
    return [[int(c[2 * k]), int(c[2 * k + 1])] for k in range(4)]


def _rn(v):
    return int(np.rint(v))                                             # round half to even, as the C side's rint


def quad_baseline(quad):
    """u = (TR - TL) + (BR - BL): the direction of the text, top and bottom edge averaged (twice their mean)"""
    (x0, y0), (x1, y1), (x2, y2), (x3, y3) = _corners(quad)
    return (x1 - x0) + (x2 - x3), (y1 - y0) + (y2 - y3)


def frame_for(quad, h, w):
    """The oriented crop of one quad on an h x w page -> (cx2, cy2, crop_scale, ux, uy), integers, no rng.  (ux, uy) is the quad's
    baseline u.  crop_scale is the ladder crop_scale_for applied to the quad's OWN length and height (rn of the mean length of its top and
    bottom edge / of its left and right edge), as if the line lay upright.  The centre is the quad's centre (rn of the corner sum / 2, in
    half-pixels), moved along each page axis by the smallest translation that brings the frame's bounding box - half-extent
    crop_scale * (|ux| + |uy|) / (2 |u|) on both axes - inside the page; where the box is larger than the page along an axis the frame
    is centred on the page along that axis."""
    c = _corners(quad)
    ux, uy = quad_baseline(c)
    if ux == 0 and uy == 0:
        raise ValueError("the quad has no baseline: (TR - TL) + (BR - BL) is (0, 0)")
    dist = lambda a, b: float(np.sqrt(float((c[a][0] - c[b][0]) ** 2 + (c[a][1] - c[b][1]) ** 2)))
    length, height = _rn((dist(1, 0) + dist(2, 3)) / 2.0), _rn((dist(3, 0) + dist(2, 1)) / 2.0)
    crop_scale = max(1, int(crop_scale_for((0, 0, length, height), h, w)))
    ext2 = int(np.ceil(crop_scale * (abs(ux) + abs(uy)) / float(np.sqrt(float(ux * ux + uy * uy)))))       # the box's side, = 2 half-extents in half-pixels
    centre = []
    for axis, n in ((0, w), (1, h)):
        c2 = _rn(sum(p[axis] for p in c) / 2.0)
        lo, hi = ext2 - 1, 2 * n - 1 - ext2                            # the box [c2/2 - ext/2, c2/2 + ext/2] inside [-1/2, n - 1/2]
        centre.append(min(max(c2, lo), hi) if lo <= hi else n - 1)
    return centre[0], centre[1], crop_scale, ux, uy


def persp_frame_accepted(quad, h, w, frame, size=512):
    """None if the C side (host-only: dmx_edit_quads_prepare, dmx_edit_quads_persp_prepare) accepts the projective frame (ci2, cj2,
    crop_scale) of `quad` on an h x w page at crop size `size`, else its message"""
    c = _corners(quad)
    pages, host, persp = (_cabi.EditPage * 1)(), (_cabi.EditQuad * 1)(), (_cabi.QuadPersp * 1)()
    pages[0].original, pages[0].H, pages[0].W, pages[0].item_lo, pages[0].item_hi = 64, int(h), int(w), 0, 1
    for k in range(4):
        host[0].x[k], host[0].y[k] = c[k]
    host[0].cx2, host[0].cy2, host[0].crop_scale, host[0].ux, host[0].uy = 2 * c[0][0], 2 * c[0][1], 1, 1, 0
    persp[0].ci2, persp[0].cj2, persp[0].crop_scale = (int(v) for v in frame)
    lib = _cabi.lib()
    if lib.dmx_edit_quads_prepare(pages, 1, host, 1, int(size)) != 0 or lib.dmx_edit_quads_persp_prepare(pages, 1, host, persp, 1, int(size)) != 0:
        return lib.dmx_last_error().decode()
    return None


def strip_size(quad):
    """(rw, rh) of the quad's upright strip: rn of half the summed opposite edges, plus 1 (csrc/prepost_quad.h, the rectify section)"""
    c = _corners(quad)
    ux, uy = quad_baseline(c)
    vx, vy = (c[3][0] - c[0][0]) + (c[2][0] - c[1][0]), (c[3][1] - c[0][1]) + (c[2][1] - c[1][1])
    return _rn(np.sqrt(float(ux * ux + uy * uy)) / 2.0) + 1, _rn(np.sqrt(float(vx * vx + vy * vy)) / 2.0) + 1


_LADDER = (128, 256, 384, 512, 640, 784, 1000)


def persp_frame_for(quad, h, w, size=512):
    """The projective frame of one quad on an h x w page -> (ci2, cj2, crop_scale), integers, no rng (csrc/prepost_persp.h): the window
    the network sees is a square of side crop_scale in the pixels of the quad's upright rw x rh STRIP, carried to the page by the
    homography that takes the strip to the quad.  The centre is the strip's centre, (rw - 1, rh - 1) half-pixels.  crop_scale is the
    ladder crop_scale_for applied to (rw, rh) as frame_for applies it to length and height; where the C side refuses that window - the
    homography's denominator changes by more than 4x over it, or its horizon crosses it - it is stepped down: the ladder's rungs below
    it that are still longer than the strip, then the strip's own length rw.  ValueError, naming the quad, if that is refused too.
    Limit: the centre is NOT moved to keep the window on the page; where the window overhangs, clamped taps replicate the border."""
    c = _corners(quad)
    rw, rh = strip_size(c)
    first = max(1, int(crop_scale_for((0, 0, rw, rh), h, w)))
    tries = [first] + [b for b in reversed(_LADDER) if rw < b < first] + ([rw] if rw < first else [])
    why = None
    for crop_scale in tries:
        why = persp_frame_accepted(c, h, w, (rw - 1, rh - 1, crop_scale), size)
        if why is None:
            return rw - 1, rh - 1, crop_scale
    raise ValueError(f"no projective frame for the quad {c} on a {w}x{h} page: windows of {tries} strip pixels are all refused; the last: {why}")


def plan_quads(quads_per_page, sizes, perspective=False, size=512):
    """frame_for for every quad of every page: quads_per_page is a list of P lists of quads, sizes the pages' (h, w).  Returns P lists of
    frames.  Deterministic: nothing is drawn.  perspective=True: persp_frame_for instead - projective frames (ci2, cj2, crop_scale), for
    crops of `size`."""
    quads_per_page, sizes = list(quads_per_page), list(sizes)
    if len(quads_per_page) != len(sizes):
        raise ValueError(f"{len(quads_per_page)} lists of quads, {len(sizes)} page sizes: the lengths must agree")
    if perspective:
        return [[persp_frame_for(q, int(h), int(w), size) for q in quads] for quads, (h, w) in zip(quads_per_page, sizes)]
    return [[frame_for(q, int(h), int(w)) for q in quads] for quads, (h, w) in zip(quads_per_page, sizes)]


_Quads = collections.namedtuple("_Quads", "images dev quads frames counts persp", defaults=(None,))


def _check_quads(images, quads, frames, perspective=False):
    """the list half of the quad functions' arguments, checked before any tensor is looked at; frames None (rectify_quads): placeholders.
    perspective: the frames are projective, (ci2, cj2, crop_scale) - they go to `persp`, and `frames` holds the placeholders"""
    images, quads = list(images), [list(q) for q in quads]
    P = len(images)
    if P == 0:
        raise ValueError("no pages: the quad pre/post-processing needs at least one")
    if P > _cabi.EDIT_MAX_ITEMS:
        raise ValueError(f"{P} pages in one launch, at most {_cabi.EDIT_MAX_ITEMS}")
    if len(quads) != P:
        raise ValueError(f"{P} pages, {len(quads)} lists of quads: the lengths must agree")
    if frames is not None:
        frames = [list(f) for f in frames]
        if len(frames) != P:
            raise ValueError(f"{P} pages, {len(frames)} lists of frames: the lengths must agree")
    flat_q, flat_f, counts = [], [], []
    for p in range(P):
        if not quads[p]:
            raise ValueError(f"page {p}: no quads; every page needs at least one")
        if frames is not None and len(frames[p]) != len(quads[p]):
            raise ValueError(f"page {p}: {len(quads[p])} quads, {len(frames[p])} frames: the lengths must agree")
        flat_q.extend(_corners(q) for q in quads[p])
        if frames is not None:
            for j, f in enumerate(frames[p]):
                if perspective and (f is None or len(f) != 3):
                    raise ValueError(f"page {p}: quad {j}: a projective frame is (ci2, cj2, crop_scale)")
                if not perspective and len(f) != 5:
                    raise ValueError(f"page {p}: a frame is (cx2, cy2, crop_scale, ux, uy)")
                flat_f.append(tuple(int(v) for v in f))
        counts.append(len(quads[p]))
    if len(flat_q) > _cabi.EDIT_MAX_ITEMS:
        raise ValueError(f"{len(flat_q)} quads in one launch, at most {_cabi.EDIT_MAX_ITEMS}")
    dev = _check_page_images(images)
    persp = None
    if perspective:                                                    # (frames None: the strips alone, which read no frame)
        persp, frames = (flat_f if frames is not None else []), None
    if frames is None:                                                 # the strips read no frame: any valid one, on the quad's first corner
        flat_f = [(2 * q[0][0], 2 * q[0][1], 1, 1, 0) for q in flat_q]
    return _Quads(images, dev, flat_q, flat_f, counts, persp)


_QuadTables = collections.namedtuple("_QuadTables", "host pages persp stage dbuf off xoff")


def _upload_quads(qx, S, out=None, union=None):
    """the tables of one quad launch - dmx_edit_quad | dmx_edit_page, and with projective frames (qx.persp) | dmx_quad_persp - in ONE
    pinned staging buffer, filled and validated (dmx_edit_quads_prepare, then dmx_edit_quads_persp_prepare), then ONE asynchronous copy on
    the current stream.  S = 0 (rectify_quads): the strips alone, which depend neither on the frames nor on S.  Returns a _QuadTables:
    the host tables (persp None for the similarity frame), the pinned storage, the device buffer, the byte offsets of the page table and
    of the projective table in it."""
    return _upload_quads_extra(qx, S, out, union, None)[0]


def _upload_quads_extra(qx, S, out, union, extra):
    """_upload_quads with more tables behind the quad tables, in the same pinned buffer and the same copy, in the spirit of `extra` of
    _upload.  extra: None, or a function of the PREPARED host quad table that returns numpy arrays - tables that depend on derived fields,
    as the read-back's resample tables depend on the strips' sizes.  The arrays size the buffer, so with `extra` the tables are prepared
    in plain host memory first and copied into the pinned buffer; without it they are filled in the pinned buffer directly.  Returns
    (the _QuadTables, the byte offsets of the extra arrays)."""
    B, P = len(qx.quads), len(qx.images)
    n_quads, n_pages = B * ctypes.sizeof(_cabi.EditQuad), P * ctypes.sizeof(_cabi.EditPage)
    off, xoff = n_quads, n_quads + n_pages
    n_tables = xoff + (B * ctypes.sizeof(_cabi.QuadPersp) if qx.persp is not None else 0)

    def views(st):
        return ((_cabi.EditQuad * B).from_buffer(st[:off]), (_cabi.EditPage * P).from_buffer(st[off:xoff]),
                (_cabi.QuadPersp * B).from_buffer(st[xoff:n_tables]) if qx.persp is not None else None)

    stage = torch.empty(n_tables, dtype=torch.uint8, pin_memory=True) if extra is None else None
    tab = stage.numpy() if extra is None else np.empty(n_tables, dtype=np.uint8)
    tab[:] = 0
    host, pages, persp = views(tab)
    lo = 0
    for p, (pg, img, n) in enumerate(zip(pages, qx.images, qx.counts)):
        pg.original = img.data_ptr()
        pg.out = out[p].data_ptr() if out is not None else 0
        pg.union_mask = union[p].data_ptr() if union is not None else 0
        pg.H, pg.W, pg.item_lo, pg.item_hi = int(img.shape[0]), int(img.shape[1]), lo, lo + n
        for it, c, f in zip(host[lo:lo + n], qx.quads[lo:lo + n], qx.frames[lo:lo + n]):
            for k in range(4):
                it.x[k], it.y[k] = c[k]
            it.cx2, it.cy2, it.crop_scale, it.ux, it.uy = f
            it.page = p
        lo += n
    # (the placeholder frames of the strips and of the projective entries are prepared at any valid S)
    _cabi.check(_cabi.lib().dmx_edit_quads_prepare(pages, P, host, B, max(S, 8) if qx.persp is not None or S == 0 else S), "edit_quads_prepare")
    if persp is not None:
        for e, f in zip(persp, qx.persp):
            e.ci2, e.cj2, e.crop_scale = f
        _cabi.check(_cabi.lib().dmx_edit_quads_persp_prepare(pages, P, host, persp, B, S), "edit_quads_persp_prepare")
    eoffs = []
    if extra is not None:
        arrays, total = [np.ascontiguousarray(a) for a in extra(host)], n_tables
        for a in arrays:
            total = (total + 15) // 16 * 16                            # (every array 16-byte aligned, whatever lies before it)
            eoffs.append(total); total += a.nbytes
        stage = torch.empty(total, dtype=torch.uint8, pin_memory=True)
        st = stage.numpy()
        st[:n_tables] = tab
        for a, o in zip(arrays, eoffs):
            st[o:o + a.nbytes] = a.reshape(-1).view(np.uint8)
        host, pages, persp = views(st)                                 # the entries read the host tables where the copy reads them
    with torch.cuda.device(qx.dev):
        dbuf = torch.empty(stage.numel(), dtype=torch.uint8, device=qx.dev)
        dbuf.copy_(stage, non_blocking=True)                          # the one H2D copy
    return _QuadTables(host, pages, persp, stage, dbuf, off, xoff), eoffs


def _call_quads(name, t, head, *tail):
    """dmx_<name>(*head, the tables of t - host and device, pages then quads -, B, *tail, stream) on the current stream; with projective
    frames dmx_<name>_persp, their table (host, device) spliced in behind the quads, where the C signature has it"""
    base = t.dbuf.data_ptr()
    tables = (t.pages, base + t.off, len(t.pages), t.host, base)
    if t.persp is not None:
        name, tables = name + "_persp", tables + (t.persp, base + t.xoff)
    _cabi.check(getattr(_cabi.lib(), "dmx_" + name)(*head, *tables, len(t.host), *tail, _cabi.current_stream()), name)


def _plan_persp(images, quads, frames, perspective, size):
    """the projective frames where a perspective call left them open (frames None), planned here; size: the crop size, or the decoder
    outputs whose last dimension it is"""
    if perspective and frames is None:
        S = size if isinstance(size, (int, np.integer)) else size.shape[-1]
        return plan_quads([list(q) for q in quads], [(int(i.shape[0]), int(i.shape[1])) for i in images], True, int(S))
    return frames


def preprocess_quads(images, quads, frames, size=512, perspective=False):
    """preprocess_pages for quadrilateral regions, in one launch.  images: P contiguous uint8 CUDA [h_p][w_p][3] tensors on one device;
    quads: P lists of quads (four corners TL, TR, BR, BL); frames: P lists of (cx2, cy2, crop_scale, ux, uy) (plan_quads gives them).
    Returns the dict preprocess_pages returns, N rows page-major: row b is quad b's oriented crop - the text's baseline horizontal -,
    masked_image with the quad itself blacked out before resampling, mask the quad as seen in the crop.
    perspective=True: frames are projective, (ci2, cj2, crop_scale) (plan_quads(..., perspective=True); None plans them here) - the crop
    is taken through the homography that makes the quad an upright rectangle (csrc/prepost_persp.h), so a trapezoid's text is seen
    without keystone; the same outputs."""
    S = int(size)
    qx = _check_quads(images, quads, _plan_persp(images, quads, frames, perspective, S), perspective)
    t = _upload_quads(qx, S)
    with torch.cuda.device(qx.dev):
        pre = _crop_outputs(len(qx.quads), S, qx.dev)
        _call_quads("preprocess_quads", t, (), S, *map(_cabi.ptr, pre.values()))
    return pre


class QuadBlend:
    """How the quad pastes put a generated patch onto the page (include/diffute_hip.h above dmx_paste_color_stats_quads; integers
    throughout).  A pixel's depth m is the smallest of its whole pixel steps inside the quad's four edges, measured PERPENDICULAR to each
    edge (floor(E_k / |e_k|), exactly), and inside the quad's bounding box; m >= 0 is the quad itself.
    feather - the width f of the linear ramp: the weight of the patch is min(m + grow + 1, f + 1) / (f + 1), so f = 0 is a hard edge;
    grow - the paste region is the quad with every edge moved out by g pixels, its mitres cut by the bounding box grown by g, and cut
              where it leaves the quad's crop (a hard edge there).  With grow >= feather the whole quad is fully generated and the ramp
              lies around it; with grow = 0 the ramp lies INSIDE the quad;
    match_color - shift every channel of the patch by the mean difference between the original page and the patch over the ring of
              `ring` pixels around the paste region, at most `max_shift` levels (a mean shift of bytes: no gain, no gamma).
    feather, grow <= QUAD_BLEND_MAX = 1024, 1 <= ring <= 1024.  A type of its own, not a PasteBlend: the ramp and the caps differ.
    QuadBlend() - all off - pastes what blend=None pastes, bit for bit, when every pixel of every quad lies on that quad's crop: here an
    item whose pixel is off its crop updates nothing and an earlier quad shows through, where the plain paste lets the last covering
    quad decide and leaves the original byte."""
    __slots__ = ("feather", "grow", "match_color", "ring", "max_shift")

    def __init__(self, feather=0, grow=0, match_color=False, ring=8, max_shift=32):
        cap = _cabi.QUAD_BLEND_MAX
        for name, v, lo, hi in (("feather", feather, 0, cap), ("grow", grow, 0, cap), ("ring", ring, 1, cap), ("max_shift", max_shift, 0, 255)):
            if isinstance(v, bool) or not isinstance(v, (int, np.integer)):
                raise TypeError(f"QuadBlend: {name} must be an integer, got {v!r}")
            if not lo <= v <= hi:
                raise ValueError(f"QuadBlend: {name} = {v}, expected {lo} .. {hi}")
        if not isinstance(match_color, (bool, np.bool_)):
            raise TypeError(f"QuadBlend: match_color must be a bool, got {match_color!r}")
        self.feather, self.grow, self.match_color, self.ring, self.max_shift = int(feather), int(grow), bool(match_color), int(ring), int(max_shift)

    def __repr__(self):
        return (f"QuadBlend(feather={self.feather}, grow={self.grow}, match_color={self.match_color}, ring={self.ring}, "
                f"max_shift={self.max_shift})")

    def grown(self, quads, h=None, w=None):
        """the quads' bounding boxes grown by `grow` - every paste region lies inside its grown bounding box - as half-open
        [(x1, y1, x2, y2)], clipped to an h x w page if the size is given: what metrics.outside_diff takes to show that nothing outside
        them changed"""
        g, out = self.grow, []
        for quad in quads:
            c = _corners(quad)
            x1, y1 = min(x for x, _ in c) - g, min(y for _, y in c) - g
            x2, y2 = max(x for x, _ in c) + g + 1, max(y for _, y in c) + g + 1
            if w is not None:
                x1, x2 = max(x1, 0), min(x2, int(w))
            if h is not None:
                y1, y2 = max(y1, 0), min(y2, int(h))
            out.append((x1, y1, x2, y2))
        return out

    def _struct(self):
        return _cabi.PasteBlend(self.feather, self.grow, self.ring, self.max_shift, int(self.match_color))


def _check_quad_blend(blend):
    if isinstance(blend, PasteBlend):
        raise NotImplementedError("blend: a PasteBlend is not supported for quads (its ramp is measured along the page's axes); pass a QuadBlend")
    if not isinstance(blend, QuadBlend):
        raise TypeError(f"blend: expected a QuadBlend or None, got {type(blend).__name__}")
    return blend


def _check_choice(choice, B):
    if choice is not None and not (isinstance(choice, torch.Tensor) and choice.is_cuda and choice.dtype == torch.int32 and choice.is_contiguous()
                                   and tuple(choice.shape) == (B,)):
        raise ValueError(f"choice must be a contiguous int32 CUDA tensor [{B}]")


def _blend_paste_quads(qx, image_vae, blend, return_mask, out, scores=None, threshold=None):
    """the blended quad pastes: [choose ->] [stats ->] paste, every launch on the current stream, ONE table upload, nothing read on the
    host.  scores given: image_vae is [B,K,3,S,S] and (out, choice[, union]) comes back, as from postprocess_select_quads"""
    B, select = len(qx.quads), scores is not None
    S, K = _check_vae(image_vae, B, select)
    thr = _check_scores(scores, B, K, threshold) if select else None
    out, union = _page_outputs(qx.images, qx.dev, out, return_mask)
    v = image_vae.to(torch.float32).contiguous()
    t, bs = _upload_quads(qx, S, out, union), blend._struct()
    with torch.cuda.device(qx.dev):
        choice = _choose(_cabi.lib(), scores, B, K, thr, qx.dev) if select else None
        stats = None
        if blend.match_color:
            stats = torch.empty(B, 4, dtype=torch.int64, device=qx.dev)
            _call_quads("paste_color_stats_quads", t, (_cabi.ptr(v), S), ctypes.byref(bs), _cabi.ptr(choice), K, _cabi.ptr(stats))
        _call_quads("postprocess_paste_blend_quads", t, (_cabi.ptr(v), S), ctypes.byref(bs), _cabi.ptr(stats), _cabi.ptr(choice), K)
    if select:
        return (out, choice, union) if return_mask else (out, choice)
    return (out, union) if return_mask else out


def paste_color_stats_quads(image_vae, images, quads, frames, blend, choice=None, perspective=False):
    """The colour statistics the blended quad paste would use, int64 CUDA [N,4] = (n, D_r, D_g, D_b) per quad, D already clamped to
    +- max_shift * n: over the ring of blend.ring pixels around the quad's paste region (on its crop), of the ORIGINAL page against the
    quad's own decoder row.  One launch, one block per quad: a quad's numbers are the same alone or in any batch.  images / quads /
    frames / perspective: as for postprocess_quads.  choice: None - image_vae is [N,3,S,S] -, or int32 CUDA [N] - image_vae is
    [N,K,3,S,S], quad b reads candidate choice[b], a quad with choice[b] < 0 writes zeros."""
    blend = _check_quad_blend(blend)
    if not (isinstance(image_vae, torch.Tensor) and image_vae.is_cuda):
        raise TypeError("image_vae: expected a CUDA tensor")
    qx = _check_quads(images, quads, _plan_persp(images, quads, frames, perspective, image_vae), perspective)
    B = len(qx.quads)
    S, K = _check_vae(image_vae, B, choice is not None)
    _check_choice(choice, B)
    v = image_vae.to(torch.float32).contiguous()
    t, bs = _upload_quads(qx, S), blend._struct()
    with torch.cuda.device(qx.dev):
        stats = torch.empty(B, 4, dtype=torch.int64, device=qx.dev)
        _call_quads("paste_color_stats_quads", t, (_cabi.ptr(v), S), ctypes.byref(bs), _cabi.ptr(choice), K, _cabi.ptr(stats))
    return stats


def postprocess_quads(image_vae, images, quads, frames, return_mask=False, out=None, perspective=False, blend=None):
    """postprocess_pages for quadrilateral regions, in one launch.  image_vae: fp32 CUDA [N,3,S,S] decoder outputs, page-major; the other
    arguments as for preprocess_quads.  Returns the list of P uint8 [h_p][w_p][3] pages: a pixel inside a quad (edges included) and on
    that quad's crop comes from the decoder output through the inverse of the frame - where quads overlap the later one decides -, every
    other pixel is the original's; with return_mask=True also the list of P union masks uint8 [h_p][w_p] (1 inside any quad).  out: as
    for postprocess_pages.  perspective=True: frames are projective (None plans them), and a page pixel finds its crop coordinates
    through the inverse homography; which pixels are pasted, and the union masks, follow the same rule.
    blend: None - the hard paste above, exactly today's code path -, or a QuadBlend: feathered edge and / or colour match ([stats ->]
    blended paste, one launch each, one table upload).  Every quad is blended over what the quads before it left, in table order; a pixel
    off a quad's crop is left to the earlier quads; the union masks are then 1 inside any quad GROWN by blend.grow, and the page equals
    the original wherever the mask is 0."""
    if blend is not None:
        blend = _check_quad_blend(blend)
    qx = _check_quads(images, quads, _plan_persp(images, quads, frames, perspective, image_vae), perspective)
    if blend is not None:
        return _blend_paste_quads(qx, image_vae, blend, return_mask, out)
    S, _ = _check_vae(image_vae, len(qx.quads), False)
    out, union = _page_outputs(qx.images, qx.dev, out, return_mask)
    v = image_vae.to(torch.float32).contiguous()
    t = _upload_quads(qx, S, out, union)
    with torch.cuda.device(qx.dev):
        _call_quads("postprocess_paste_quads", t, (_cabi.ptr(v), S))
    return (out, union) if return_mask else out


def rectify_quads(images, quads, perspective=False):
    """Every quad as an upright strip, in one launch: a list of N uint8 CUDA [h_b][w_b][3] tensors, page-major, views of ONE buffer -
    what TrOCRProcessor(images=...) accepts on the device, so the OCR model can read a skewed line.  The strip runs along the quad's
    baseline at scale 1 (w_b, h_b: rn of half the summed opposite edges, plus 1); an axis-aligned quad gives page[y1:y2+1, x1:x2+1].
    perspective=True: strips of the same sizes through the homography that takes the quad's corners to the strip's corners - a
    trapezoid comes out upright and without keystone (no frame is needed: the strip is the quad itself)."""
    qx = _check_quads(images, quads, None, perspective)
    t = _upload_quads(qx, 0)                                           # (the strips depend neither on the frames nor on S)
    last = t.host[len(t.host) - 1]
    total = int(last.rect_off) + int(last.rw) * int(last.rh) * 3
    with torch.cuda.device(qx.dev):
        buf = torch.empty(total, dtype=torch.uint8, device=qx.dev)
        _call_quads("rectify_quads", t, (), _cabi.ptr(buf), total)
    return [buf[int(q.rect_off):int(q.rect_off) + int(q.rw) * int(q.rh) * 3].view(int(q.rh), int(q.rw), 3) for q in t.host]


def readback_pixel_values_quads(image_vae, images, quads, frames, processor, perspective=False, return_resized=False, out=None, out_resized=None):
    """readback_pixel_values_pages for quadrilateral regions, in ONE launch: image_vae fp32 CUDA [N,K,3,S,S] (or [N*K,3,S,S]) decoder
    outputs, page-major -> pixel_values fp32 [N*K,3,S_h,S_w].  Row (b, k) is bit for bit `processor(rectify_quads(postprocess_quads(
    image_vae[b, k], quad b ALONE)))` - candidate k pasted over the original page through quad b's frame, the quad taken as an upright strip,
    the strip resized and normalised - without the pasted page, the strip or the processor call; other quads of the page play no part.
    images / quads / frames / perspective: as for postprocess_quads (perspective=True with frames=None plans them).  processor: a
    ViTImageProcessor or TrOCRProcessor with do_resize.  The quads, the pages, the projective frames, the passes and the processor's
    tables travel in one pinned staging buffer, one H2D copy.  return_resized / out / out_resized as for readback_pixel_values."""
    ip = _resizing_processor(processor, "readback_pixel_values_quads")
    if not (isinstance(image_vae, torch.Tensor) and image_vae.is_cuda):
        raise TypeError("image_vae: expected a CUDA tensor")
    frames = _plan_persp(images, quads, frames, perspective, image_vae.shape[-1])
    qx = _check_quads(images, quads, frames, perspective)
    B = len(qx.quads)
    if image_vae.dim() == 4:                                           # [N*K,3,S,S]: the rows of _candidate_rows before their reshape
        if image_vae.shape[0] % B:
            raise ValueError(f"image_vae must be [{B},K,3,S,S] or [{B}*K,3,S,S]: {image_vae.shape[0]} rows are no multiple of {B} quads")
        image_vae = image_vae.reshape(B, image_vae.shape[0] // B, *image_vae.shape[1:])
    S, K = _check_vae(image_vae, B, True)
    S_h, S_w = ip.size["height"], ip.size["width"]
    _check_readback_outputs(out, out_resized, B * K, S_h, S_w, qx.dev)
    lib = _cabi.lib()
    cap, made = int(lib.dmx_glyph_max_taps()), {}

    def tables_of(host):                                               # the strips' sizes are derived fields: (0, 0, rw, rh) stands for a box
        made["passes"], made["tables"], made["max_taps"] = _readback_tables([(0, 0, int(q.rw), int(q.rh)) for q in host], ip, cap, "quad")
        return made["passes"], ip._norm, made["tables"]

    v = image_vae.to(torch.float32).contiguous()
    t, (off_pass, off_norm, off_tab) = _upload_quads_extra(qx, S, None, None, tables_of)
    host_passes = (_cabi.ReadbackPass * B).from_buffer(t.stage.numpy()[off_pass:off_pass + made["passes"].nbytes])
    base = t.dbuf.data_ptr()
    with torch.cuda.device(qx.dev):
        if out is None:
            out = torch.empty(B * K, 3, S_h, S_w, dtype=torch.float32, device=qx.dev)
        res = out_resized
        if res is None and return_resized:
            res = torch.empty(B * K, 3, S_h, S_w, dtype=torch.uint8, device=qx.dev)
        _call_quads("readback_pixel_values_quads", t, (_cabi.ptr(v), S), K, base + off_tab, int(made["tables"].size), base + off_norm, host_passes,
                    base + off_pass, made["max_taps"], S_h, S_w, _cabi.ptr(out), _cabi.ptr(res))
    return (out, res) if (return_resized or out_resized is not None) else out


def postprocess_select_quads(image_vae, scores, images, quads, frames, threshold=None, return_mask=False, out=None, perspective=False, blend=None):
    """postprocess_select_pages for quadrilateral regions: choose and paste in ONE launch, without reading the scores on the host.
    image_vae fp32 CUDA [N,K,3,S,S], scores fp32 CUDA [N,K], both page-major; the other arguments as for postprocess_quads.  Returns
    (pages, choice): choice int32 [N] on the device by the rule of postprocess_select_batch, and the list of P pages postprocess_quads
    gives for the chosen rows.  A quad whose best score is below `threshold` (choice -1) is TRANSPARENT: it pastes nothing, and an earlier
    chosen quad under it still shows.  With return_mask=True also the list of P union masks, 1 inside ANY quad, skipped ones included.
    blend: None - exactly today's code path -, or a QuadBlend: choose (dmx_select_choices) -> [stats ->] blended paste of the chosen rows,
    one launch each, one table upload and still no score read on the host; pages and masks as postprocess_quads(blend=...) gives them
    for the chosen rows, a skipped quad updating nothing."""
    if blend is not None:
        blend = _check_quad_blend(blend)
    _check_scores_tensor(scores)
    if not (isinstance(image_vae, torch.Tensor) and image_vae.is_cuda):
        raise TypeError("image_vae: expected a CUDA tensor")
    frames = _plan_persp(images, quads, frames, perspective, image_vae.shape[-1])
    qx = _check_quads(images, quads, frames, perspective)
    if blend is not None:
        return _blend_paste_quads(qx, image_vae, blend, return_mask, out, scores, threshold)
    B = len(qx.quads)
    S, K = _check_vae(image_vae, B, True)
    thr = _check_scores(scores, B, K, threshold)
    out, union = _page_outputs(qx.images, qx.dev, out, return_mask)
    with torch.cuda.device(qx.dev):
        choice = torch.empty(B, dtype=torch.int32, device=qx.dev)
    v, sc = image_vae.to(torch.float32).contiguous(), scores.to(torch.float32).contiguous()
    t = _upload_quads(qx, S, out, union)
    with torch.cuda.device(qx.dev):
        _call_quads("postprocess_paste_select_quads", t, (_cabi.ptr(v), S, _cabi.ptr(sc), thr, _cabi.ptr(choice)), K)
    return (out, choice, union) if return_mask else (out, choice)


# ------------------------------------------------------------------------------------------------ curved regions, piecewise-affine maps
# (csrc/prepost_curved.hip; the arithmetic is stated in csrc/prepost_curved.h).  A curved region is a polygon of 2n points (x, y),
# 2 <= n <= 17, as scene-text OCR gives a curved line: the n top points left to right as read, then the n bottom points right to left,
# clockwise with y down.  A frame is the projective quads': (ci2, cj2, crop_scale), the window's centre in half-pixels of the
# straightened strip's pixel-index space and its side in strip pixels.
def _polygon(polygon):
    """a polygon as given - 2n x (x, y) or 4n numbers - -> [[x, y]] * 2n of ints"""
    c = np.asarray(polygon).reshape(-1)
    if c.size % 2 != 0 or (c.size // 2) % 2 != 0:
        raise ValueError(f"a curved region is 2n points (x, y) - n on top as read, then n on the bottom backwards; got {c.size} numbers: an odd point count")
    n = c.size // 4
    if not 2 <= n <= _cabi.CURVED_MAX_PAIRS:
        raise ValueError(f"a curved region has 2 .. {_cabi.CURVED_MAX_PAIRS} point pairs, got {n}")
    return [[int(c[2 * k]), int(c[2 * k + 1])] for k in range(2 * n)]


def strip_size_curved(polygon):
    """(rw, rh) of the polygon's straightened strip (csrc/prepost_curved.h): cell k is w_k = max(1, rn(|u_k| / 2)) columns long,
    u_k = (T_k+1 - T_k) + (B_k+1 - B_k), and rw = sum of w_k, plus 1; rh = rn(the mean length of the n segments T_k B_k) + 1.  For a
    parallelogram given as four points this is strip_size(quad)."""
    p = _polygon(polygon)
    n = len(p) // 2
    rw, total = 1, np.float64(0.0)
    for k in range(n):
        dx, dy = p[2 * n - 1 - k][0] - p[k][0], p[2 * n - 1 - k][1] - p[k][1]
        total = total + np.sqrt(np.float64(dx * dx + dy * dy))
        if k < n - 1:
            ux = (p[k + 1][0] - p[k][0]) + (p[2 * n - 2 - k][0] - p[2 * n - 1 - k][0])
            uy = (p[k + 1][1] - p[k][1]) + (p[2 * n - 2 - k][1] - p[2 * n - 1 - k][1])
            rw += max(1, _rn(np.sqrt(np.float64(ux * ux + uy * uy)) / 2.0))
    return rw, _rn(total / np.float64(n)) + 1


def curved_frame_accepted(polygon, h, w, frame, size=512):
    """None if the C side (host-only: dmx_edit_curved_prepare) accepts the frame (ci2, cj2, crop_scale) of `polygon` on an h x w page at
    crop size `size`, else its message"""
    p = _polygon(polygon)
    M = len(p) // 2 - 1
    pages, host, pieces = (_cabi.EditPage * 1)(), (_cabi.EditCurved * 1)(), (_cabi.CurvedPiece * (2 * M))()
    pages[0].original, pages[0].H, pages[0].W, pages[0].item_lo, pages[0].item_hi = 64, int(h), int(w), 0, 1
    for k, (x, y) in enumerate(p):
        host[0].x[k], host[0].y[k] = x, y
    host[0].count = len(p)
    host[0].ci2, host[0].cj2, host[0].crop_scale = (int(v) for v in frame)
    lib = _cabi.lib()
    if lib.dmx_edit_curved_prepare(pages, 1, host, pieces, 1, int(size)) != 0:
        return lib.dmx_last_error().decode()
    return None


def curved_frame_for(polygon, h, w, size=512):
    """The frame of one curved region on an h x w page -> (ci2, cj2, crop_scale), integers, no rng: the window the network sees is a
    square of side crop_scale in the pixels of the polygon's straightened rw x rh strip, centred on the strip - (rw - 1, rh - 1)
    half-pixels -, with crop_scale the ladder crop_scale_for applied to (rw, rh) as persp_frame_for applies it.  ValueError, naming the
    polygon and with the C side's reason, where dmx_edit_curved_prepare refuses the polygon or that window.
    Limit: the centre is NOT moved to keep the window on the page; where the window overhangs, clamped taps replicate the border."""
    p = _polygon(polygon)
    rw, rh = strip_size_curved(p)
    frame = (rw - 1, rh - 1, max(1, int(crop_scale_for((0, 0, rw, rh), h, w))))
    why = curved_frame_accepted(p, h, w, frame, size)
    if why is not None:
        raise ValueError(f"no frame for the curved region {p} on a {w}x{h} page: {why}")
    return frame


def plan_curved(polygons_per_page, sizes, size=512):
    """curved_frame_for for every polygon of every page: polygons_per_page is a list of P lists of polygons, sizes the pages' (h, w).
    Returns P lists of frames (ci2, cj2, crop_scale), for crops of `size`.  Deterministic: nothing is drawn."""
    polygons_per_page, sizes = list(polygons_per_page), list(sizes)
    if len(polygons_per_page) != len(sizes):
        raise ValueError(f"{len(polygons_per_page)} lists of polygons, {len(sizes)} page sizes: the lengths must agree")
    return [[curved_frame_for(q, int(h), int(w), size) for q in polys] for polys, (h, w) in zip(polygons_per_page, sizes)]


_Curved = collections.namedtuple("_Curved", "images dev polygons frames counts")


def _check_curved(images, polygons, frames):
    """the list half of the curved functions' arguments, checked before any tensor is looked at; frames None (rectify_curved): no frames"""
    images, polygons = list(images), [list(q) for q in polygons]
    P = len(images)
    if P == 0:
        raise ValueError("no pages: the curved pre/post-processing needs at least one")
    if P > _cabi.EDIT_MAX_ITEMS:
        raise ValueError(f"{P} pages in one launch, at most {_cabi.EDIT_MAX_ITEMS}")
    if len(polygons) != P:
        raise ValueError(f"{P} pages, {len(polygons)} lists of polygons: the lengths must agree")
    if frames is not None:
        frames = [list(f) for f in frames]
        if len(frames) != P:
            raise ValueError(f"{P} pages, {len(frames)} lists of frames: the lengths must agree")
    flat_q, flat_f, counts = [], [], []
    for p in range(P):
        if not polygons[p]:
            raise ValueError(f"page {p}: no polygons; every page needs at least one")
        if frames is not None and len(frames[p]) != len(polygons[p]):
            raise ValueError(f"page {p}: {len(polygons[p])} polygons, {len(frames[p])} frames: the lengths must agree")
        flat_q.extend(_polygon(q) for q in polygons[p])
        for j, f in enumerate(frames[p] if frames is not None else [(0, 0, 0)] * len(polygons[p])):
            if f is None or len(f) != 3:
                raise ValueError(f"page {p}: polygon {j}: a frame is (ci2, cj2, crop_scale)")
            flat_f.append(tuple(int(v) for v in f))
        counts.append(len(polygons[p]))
    if len(flat_q) > _cabi.EDIT_MAX_ITEMS:
        raise ValueError(f"{len(flat_q)} polygons in one launch, at most {_cabi.EDIT_MAX_ITEMS}")
    cells = sum(len(q) // 2 - 1 for q in flat_q)
    if cells > _cabi.CURVED_MAX_CELLS:
        raise ValueError(f"{cells} cells in one launch, at most {_cabi.CURVED_MAX_CELLS}")
    return _Curved(images, _check_page_images(images), flat_q, flat_f, counts)


_CurvedTables = collections.namedtuple("_CurvedTables", "host pages pieces stage dbuf off xoff")


def _upload_curved(cx, S, out=None, union=None):
    """the tables of one curved launch - dmx_edit_curved | dmx_edit_page | dmx_curved_piece - in ONE pinned staging buffer, filled and
    validated (dmx_edit_curved_prepare), then ONE asynchronous copy on the current stream.  S = 0 (rectify_curved): the strips alone,
    which depend neither on the frames nor on S.  Returns a _CurvedTables: the host tables, the pinned storage, the device buffer, the
    byte offsets of the page table and of the piece table in it."""
    B, P = len(cx.polygons), len(cx.images)
    NP = sum(len(q) - 2 for q in cx.polygons)
    off = B * ctypes.sizeof(_cabi.EditCurved)
    xoff = off + P * ctypes.sizeof(_cabi.EditPage)
    total = xoff + NP * ctypes.sizeof(_cabi.CurvedPiece)
    stage = torch.empty(total, dtype=torch.uint8, pin_memory=True)
    st = stage.numpy()
    st[:] = 0
    host, pages = (_cabi.EditCurved * B).from_buffer(st[:off]), (_cabi.EditPage * P).from_buffer(st[off:xoff])
    pieces = (_cabi.CurvedPiece * NP).from_buffer(st[xoff:total])
    lo = 0
    for p, (pg, img, n) in enumerate(zip(pages, cx.images, cx.counts)):
        pg.original = img.data_ptr()
        pg.out = out[p].data_ptr() if out is not None else 0
        pg.union_mask = union[p].data_ptr() if union is not None else 0
        pg.H, pg.W, pg.item_lo, pg.item_hi = int(img.shape[0]), int(img.shape[1]), lo, lo + n
        for it, c, f in zip(host[lo:lo + n], cx.polygons[lo:lo + n], cx.frames[lo:lo + n]):
            for k, (x, y) in enumerate(c):
                it.x[k], it.y[k] = x, y
            it.count, it.page = len(c), p
            it.ci2, it.cj2, it.crop_scale = f
        lo += n
    _cabi.check(_cabi.lib().dmx_edit_curved_prepare(pages, P, host, pieces, B, S), "edit_curved_prepare")
    with torch.cuda.device(cx.dev):
        dbuf = torch.empty(total, dtype=torch.uint8, device=cx.dev)
        dbuf.copy_(stage, non_blocking=True)                          # the one H2D copy
    return _CurvedTables(host, pages, pieces, stage, dbuf, off, xoff)


def _call_curved(name, t, head, *tail):
    """dmx_<name>(*head, the tables of t - host and device: pages, items, pieces -, B, *tail, stream) on the current stream"""
    base = t.dbuf.data_ptr()
    _cabi.check(getattr(_cabi.lib(), "dmx_" + name)(*head, t.pages, base + t.off, len(t.pages), t.host, base, t.pieces, base + t.xoff, len(t.host),
                                                    *tail, _cabi.current_stream()), name)


def _plan_curved(images, polygons, frames, size):
    """the frames where a call left them open (frames None), planned here; size: the crop size, or the decoder outputs whose last
    dimension it is"""
    if frames is not None:
        return frames
    S = size if isinstance(size, (int, np.integer)) else size.shape[-1]
    return plan_curved([list(q) for q in polygons], [(int(i.shape[0]), int(i.shape[1])) for i in images], int(S))


def _no_curved_blend(blend, who):
    if blend is not None:
        raise NotImplementedError(f"{who}: no blend for curved regions yet (blend must be None); the hard paste of the polygon is what there is")


def preprocess_curved(images, polygons, frames, size=512):
    """preprocess_quads for curved regions, in one launch.  images: P contiguous uint8 CUDA [h_p][w_p][3] tensors on one device; polygons:
    P lists of polygons (2n points: top as read, then bottom backwards); frames: P lists of (ci2, cj2, crop_scale) (plan_curved gives
    them; None plans them here).  Returns the dict preprocess_quads returns, N rows page-major: row b is polygon b's window with the line
    STRAIGHT - every crop pixel goes to the page through the affine piece of its column band of the strip -, masked_image with the
    polygon (the union of its cells) blacked out before resampling, mask the polygon as seen in the crop."""
    S = int(size)
    cx = _check_curved(images, polygons, _plan_curved(images, polygons, frames, S))
    t = _upload_curved(cx, S)
    with torch.cuda.device(cx.dev):
        pre = _crop_outputs(len(cx.polygons), S, cx.dev)
        _call_curved("preprocess_curved", t, (), S, *map(_cabi.ptr, pre.values()))
    return pre


def postprocess_curved(image_vae, images, polygons, frames, return_mask=False, out=None, blend=None):
    """postprocess_quads for curved regions, in one launch.  image_vae: fp32 CUDA [N,3,S,S] decoder outputs, page-major; the other
    arguments as for preprocess_curved.  Returns the list of P uint8 [h_p][w_p][3] pages: a pixel inside a polygon (some cell covers it,
    edges included) and on that polygon's crop comes from the decoder output through the inverse of the piece it lies in - the result is
    put back BENT; where polygons overlap the later one decides -, every other pixel is the original's; with return_mask=True also the
    list of P union masks uint8 [h_p][w_p] (1 inside any polygon).  out: as for postprocess_pages.
    blend: must be None - there is no blend for curved regions yet; anything else raises NotImplementedError."""
    _no_curved_blend(blend, "postprocess_curved")
    cx = _check_curved(images, polygons, _plan_curved(images, polygons, frames, image_vae))
    S, _ = _check_vae(image_vae, len(cx.polygons), False)
    out, union = _page_outputs(cx.images, cx.dev, out, return_mask)
    v = image_vae.to(torch.float32).contiguous()
    t = _upload_curved(cx, S, out, union)
    with torch.cuda.device(cx.dev):
        _call_curved("postprocess_paste_curved", t, (_cabi.ptr(v), S))
    return (out, union) if return_mask else out


def rectify_curved(images, polygons):
    """Every curved region as an upright, STRAIGHT strip, in one launch: a list of N uint8 CUDA [h_b][w_b][3] tensors, page-major, views
    of ONE buffer - what TrOCRProcessor(images=...) accepts on the device, so the OCR model can read a line on an arc.  (w_b, h_b) is
    strip_size_curved(polygon); an axis-aligned rectangle given as four points gives page[y1:y2+1, x1:x2+1].  No frame is needed."""
    cx = _check_curved(images, polygons, None)
    t = _upload_curved(cx, 0)                                          # (the strips depend neither on the frames nor on S)
    last = t.host[len(t.host) - 1]
    total = int(last.rect_off) + int(last.rw) * int(last.rh) * 3
    with torch.cuda.device(cx.dev):
        buf = torch.empty(total, dtype=torch.uint8, device=cx.dev)
        _call_curved("rectify_curved", t, (), _cabi.ptr(buf), total)
    return [buf[int(q.rect_off):int(q.rect_off) + int(q.rw) * int(q.rh) * 3].view(int(q.rh), int(q.rw), 3) for q in t.host]
