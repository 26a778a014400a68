"""TrOCRProcessor / ViTImageProcessor: the reference's `processor(images=ttf_imgs, return_tensors="pt").pixel_values`
(app.ipynb:773, train_diffute_v1.py:868; transformers' TrOCRProcessor, whose image half for trocr-large-printed is a ViT image
processor: PIL bilinear resize to 384x384, rescale by 1/255, normalise with mean = std = 0.5) over ONE HIP launch
(csrc/prepost.hip dmx_glyph_resize_normalize).

Everything that involves floating point happens here, in numpy, exactly as Pillow's Resample.c and transformers' numpy code do it,
and reaches the kernel as integer tables: per (in_size, out_size, filter) the tap bounds and the 2^22 fixed-point coefficients, and the
uint8 -> fp32 normalisation as a [3][256] table.  Host images, the per-image descriptors and the tables travel in one staging buffer
(one H2D copy per call); images that already live on the GPU are read in place through their strides.  No host fallback."""
import functools
import json
import os

import numpy as np
import torch

from . import _cabi

BILINEAR, BICUBIC = 2, 3                     # PIL.Image.Resampling values, as stored in preprocessor_config.json
_PRECISION_BITS = 32 - 8 - 2                 # Resample.c
_CONFIG_NAME = "preprocessor_config.json"

_DESC = np.dtype(_cabi.GlyphImage)           # include/diffute_hip.h dmx_glyph_image


def _filter_weights(x, resample):
    """Resample.c bilinear_filter / bicubic_filter (a = -0.5) on a float64 array, in the published operation order"""
    x = np.abs(x)
    if resample == BILINEAR:
        return np.where(x < 1.0, 1.0 - x, 0.0)
    a = -0.5
    return np.where(x < 1.0, ((a + 2.0) * x - (a + 3.0)) * x * x + 1, np.where(x < 2.0, (((x - 5) * x + 8) * x - 4) * a, 0.0))


def _taps(in_size, out_size, resample):
    """ksize of Resample.c precompute_coeffs: the coefficient row length"""
    filterscale = max(in_size / out_size, 1.0)
    return int(np.ceil((1.0 if resample == BILINEAR else 2.0) * filterscale)) * 2 + 1


@functools.lru_cache(maxsize=256)
def resample_table(in_size, out_size, resample):
    """precompute_coeffs + normalize_coeffs_8bpc of Resample.c in float64: int32 array = bounds [out][2] (first source index, tap
    count) followed by the fixed-point coefficients [out][ksize].  Cached: glyph heights are always 60 and the widths a small set."""
    support_unit = 1.0 if resample == BILINEAR else 2.0
    scale = in_size / out_size
    filterscale = max(scale, 1.0)
    support = support_unit * filterscale
    ksize = int(np.ceil(support)) * 2 + 1
    center = (np.arange(out_size, dtype=np.float64) + 0.5) * scale
    xmin = np.maximum((center - support + 0.5).astype(np.int64), 0)           # (int) truncates, like astype
    xmax = np.minimum((center + support + 0.5).astype(np.int64), in_size) - xmin
    ss = 1.0 / filterscale
    x = np.arange(ksize, dtype=np.float64)[None, :]
    w = _filter_weights((x + xmin[:, None] - center[:, None] + 0.5) * ss, resample)
    w = np.where(x < xmax[:, None], w, 0.0)
    ww = np.zeros(out_size, dtype=np.float64)
    for i in range(ksize):                   # Pillow sums the taps left to right; numpy's pairwise sum would round differently
        ww = ww + w[:, i]
    w = np.where(ww[:, None] != 0.0, w / np.where(ww == 0.0, 1.0, ww)[:, None], w)
    kk = np.where(w < 0, -0.5 + w * (1 << _PRECISION_BITS), 0.5 + w * (1 << _PRECISION_BITS)).astype(np.int32)
    kk = np.where(x < xmax[:, None], kk, 0).astype(np.int32)
    out = np.concatenate([np.stack([xmin, xmax], 1).astype(np.int32).reshape(-1), kk.reshape(-1)])
    out.setflags(write=False)
    return out


def normalisation_table(do_rescale, rescale_factor, do_normalize, image_mean, image_std):
    """float32 [3][256]: what transformers' numpy path makes of a resized byte - rescale is `(x.astype(float64) * scale).astype(float32)`,
    normalize is `(x - float32(mean)) / float32(std)` in float32 (without rescale it casts the byte to float32 first)."""
    v = np.arange(256, dtype=np.uint8)
    if do_rescale:
        v = (v.astype(np.float64) * rescale_factor).astype(np.float32)
    else:
        v = v.astype(np.float32)
    rows = []
    for c in range(3):
        r = v
        if do_normalize:
            r = (r - np.float32(image_mean[c])) / np.float32(image_std[c])
        rows.append(r.astype(np.float32))
    return np.stack(rows)


class BatchFeature(dict):
    """what the processor returns: `.pixel_values` and `["pixel_values"]`"""

    def __getattr__(self, k):
        try:
            return self[k]
        except KeyError:
            raise AttributeError(k)

    def to(self, *a, **kw):
        return BatchFeature({k: v.to(*a, **kw) for k, v in self.items()})


def _three(v, name):
    v = [float(v)] * 3 if isinstance(v, (int, float)) else [float(t) for t in v]
    if len(v) != 3:
        raise ValueError(f"{name} must have 3 elements, got {len(v)}")
    return v


def _as_hwc_view(img):
    """one image -> (array or tensor viewed as [H][W][3], on_gpu).  The channel axis is inferred like transformers'
    infer_channel_dimension_format for 3 channels, except that a shape that fits both layouts is refused instead of guessed."""
    if not isinstance(img, (np.ndarray, torch.Tensor)):
        if hasattr(img, "mode") and hasattr(img, "size") and hasattr(img, "tobytes"):       # PIL.Image, without importing PIL
            if img.mode != "RGB":
                raise ValueError(f"PIL images must be in RGB mode, got {img.mode!r}")
            img = np.asarray(img)
        else:
            raise TypeError(f"images must be uint8 numpy arrays, PIL images or torch uint8 tensors, got {type(img).__name__}")
    if img.dtype != (torch.uint8 if isinstance(img, torch.Tensor) else np.uint8):
        raise TypeError(f"images must be uint8, got {img.dtype}")
    if img.ndim != 3:
        raise ValueError(f"an image must have 3 dimensions (HWC or CHW), got shape {tuple(img.shape)}")
    first, last = img.shape[0] == 3, img.shape[2] == 3
    if first and last:
        raise ValueError(f"ambiguous channel axis for shape {tuple(img.shape)}: both the first and the last dimension are 3")
    if not (first or last):
        raise ValueError(f"cannot infer the channel axis of shape {tuple(img.shape)}: expected 3 channels first or last")
    if first:
        img = img.permute(1, 2, 0) if isinstance(img, torch.Tensor) else img.transpose(1, 2, 0)
    if img.shape[0] < 1 or img.shape[1] < 1:
        raise ValueError("empty image")
    return img


class ViTImageProcessor:
    """transformers' ViTImageProcessor for uint8 RGB inputs, on the GPU.  Defaults = microsoft/trocr-large-printed."""

    def __init__(self, do_resize=True, size=384, resample=BILINEAR, do_rescale=True, rescale_factor=1 / 255, do_normalize=True,
                 image_mean=(0.5, 0.5, 0.5), image_std=(0.5, 0.5, 0.5), device=None, **ignored):
        if isinstance(size, dict):
            if "height" not in size or "width" not in size:
                raise ValueError(f"size must be an int or {{'height', 'width'}}, got {size}")
            size = {"height": int(size["height"]), "width": int(size["width"])}
        else:
            size = {"height": int(size), "width": int(size)}
        if size["height"] < 1 or size["width"] < 1:
            raise ValueError(f"bad size {size}")
        if int(resample) not in (BILINEAR, BICUBIC):
            raise NotImplementedError(f"resample {resample}: only PIL BILINEAR (2) and BICUBIC (3) are implemented")
        self.do_resize, self.size, self.resample = bool(do_resize), size, int(resample)
        self.do_rescale, self.rescale_factor, self.do_normalize = bool(do_rescale), float(rescale_factor), bool(do_normalize)
        self.image_mean, self.image_std = _three(image_mean, "image_mean"), _three(image_std, "image_std")
        self.device = device
        self._norm = normalisation_table(self.do_rescale, self.rescale_factor, self.do_normalize, self.image_mean, self.image_std)

    # ---- persistence (transformers' preprocessor_config.json)
    def to_dict(self):
        return dict(image_processor_type="ViTImageProcessor", do_resize=self.do_resize, size=dict(self.size), resample=self.resample,
                    do_rescale=self.do_rescale, rescale_factor=self.rescale_factor, do_normalize=self.do_normalize,
                    image_mean=list(self.image_mean), image_std=list(self.image_std))

    @classmethod
    def from_pretrained(cls, pretrained_model_name_or_path, subfolder=None, device=None, **kw):
        d = pretrained_model_name_or_path if subfolder is None else os.path.join(pretrained_model_name_or_path, subfolder)
        with open(os.path.join(d, _CONFIG_NAME)) as f:
            cfg = json.load(f)
        keys = ("do_resize", "size", "resample", "do_rescale", "rescale_factor", "do_normalize", "image_mean", "image_std")
        return cls(device=device, **{k: cfg[k] for k in keys if k in cfg and cfg[k] is not None})

    def save_pretrained(self, save_directory):
        os.makedirs(save_directory, exist_ok=True)
        d = self.to_dict()
        d["processor_class"] = "TrOCRProcessor"
        with open(os.path.join(save_directory, _CONFIG_NAME), "w") as f:
            json.dump(d, f, indent=2, sort_keys=True)
            f.write("\n")

    # ---- the call
    def __call__(self, images=None, return_tensors="pt", device=None, return_resized=False, out=None, **unused):
        """images: one image or a list of images of mixed sizes - uint8 numpy arrays, PIL RGB images or torch uint8 tensors (host or
        GPU, HWC or CHW, any strides).  Returns BatchFeature(pixel_values = fp32 CUDA [B,3,height,width]); with return_resized=True
        also `resized`, the uint8 [B,3,height,width] image before rescale / normalise.  out (optional): a contiguous fp32 CUDA tensor
        [B,3,height,width] to write pixel_values into."""
        if images is None:
            raise ValueError("images is required")
        if return_tensors not in ("pt", None):
            raise ValueError(f"return_tensors={return_tensors!r}: only 'pt' is implemented (the result lives on the GPU)")
        if not isinstance(images, (list, tuple)):
            images = [images]
        if not images:
            raise ValueError("images is empty")
        views = [_as_hwc_view(im) for im in images]
        dev = device if device is not None else self.device
        if dev is None:
            on_gpu = [v.device for v in views if isinstance(v, torch.Tensor) and v.is_cuda]
            dev = on_gpu[0] if on_gpu else torch.device("cuda", torch.cuda.current_device())
        dev = torch.device(dev)
        if dev.type != "cuda":
            raise RuntimeError("diffute_amd: the processor runs on the GPU (cuda / ROCm device); there is no CPU path")
        if dev.index is None:
            dev = torch.device("cuda", torch.cuda.current_device())
        lib = _cabi.lib()
        cap = int(lib.dmx_glyph_max_taps())
        B = len(views)
        if self.do_resize:
            S_h, S_w = self.size["height"], self.size["width"]
        else:
            S_h, S_w = int(views[0].shape[0]), int(views[0].shape[1])
            if any((int(v.shape[0]), int(v.shape[1])) != (S_h, S_w) for v in views):
                raise ValueError("do_resize=False needs images of one size")
        # lay out the staging buffer: descriptors | normalisation table | coefficient tables (ints) | host pixels
        desc = np.zeros(B, dtype=_DESC)
        tables, table_off, n_ints, max_taps = [], {}, 0, 0
        for i, v in enumerate(views):
            H, W = int(v.shape[0]), int(v.shape[1])
            for key, (n_in, n_out) in (("h", (W, S_w)), ("v", (H, S_h))):
                if n_in == n_out:
                    desc[i][key + "_off"], desc[i][key + "_taps"] = -1, 0
                    continue
                taps = _taps(n_in, n_out, self.resample)
                if taps > cap:
                    raise ValueError(f"image {i}: resizing {n_in} -> {n_out} needs {taps} taps per output pixel, more than the kernel's cap "
                                     f"of {cap} (downscale ratio at most 31 for bilinear, 15 for bicubic)")
                k = (n_in, n_out, self.resample)
                if k not in table_off:
                    t = resample_table(*k)
                    table_off[k] = n_ints; tables.append(t); n_ints += t.size
                desc[i][key + "_off"], desc[i][key + "_taps"] = table_off[k], taps
                max_taps = max(max_taps, taps)
        off_norm = desc.nbytes
        off_tab = off_norm + self._norm.nbytes
        off_pix = off_tab + 4 * n_ints
        host_off, total = [], off_pix
        for v in views:
            if isinstance(v, torch.Tensor) and v.is_cuda:
                if v.device != dev:
                    raise ValueError(f"an image lives on {v.device}, the processor runs on {dev}")
                host_off.append(None)
            else:
                host_off.append(total)
                total += int(v.shape[0]) * int(v.shape[1]) * 3
        stage = torch.empty(total, dtype=torch.uint8, pin_memory=True)
        st = stage.numpy()
        dbuf = torch.empty(total, dtype=torch.uint8, device=dev)
        base = dbuf.data_ptr()
        for i, (v, o) in enumerate(zip(views, host_off)):
            H, W = int(v.shape[0]), int(v.shape[1])
            desc[i]["H"], desc[i]["W"] = H, W
            if o is None:                       # on the GPU already: read in place
                desc[i]["src"] = v.data_ptr()
                desc[i]["stride_y"], desc[i]["stride_x"], desc[i]["stride_c"] = (int(s) for s in v.stride())
            else:                               # packed HWC into the staging buffer
                dst = st[o:o + H * W * 3].reshape(H, W, 3)
                dst[...] = v.numpy() if isinstance(v, torch.Tensor) else v
                desc[i]["src"] = base + o
                desc[i]["stride_y"], desc[i]["stride_x"], desc[i]["stride_c"] = W * 3, 3, 1
        st[:off_norm] = desc.view(np.uint8)
        st[off_norm:off_tab] = self._norm.reshape(-1).view(np.uint8)
        if tables:
            st[off_tab:off_pix] = np.concatenate(tables).view(np.uint8)
        with torch.cuda.device(dev):
            dbuf.copy_(stage, non_blocking=True)                      # the one H2D copy
            if out is None:
                out = torch.empty(B, 3, S_h, S_w, dtype=torch.float32, device=dev)
            elif not (isinstance(out, torch.Tensor) and out.device == dev and out.dtype == torch.float32 and out.is_contiguous()
                      and tuple(out.shape) == (B, 3, S_h, S_w)):
                raise ValueError(f"out must be a contiguous fp32 tensor [{B},3,{S_h},{S_w}] on {dev}")
            res = torch.empty(B, 3, S_h, S_w, dtype=torch.uint8, device=dev) if return_resized else None
            _cabi.check(lib.dmx_glyph_resize_normalize(base, B, base + off_tab, base + off_norm, max_taps, S_h, S_w, _cabi.ptr(out),
                                                       _cabi.ptr(res), _cabi.current_stream()), "glyph_resize_normalize", lib)
        data = BatchFeature(pixel_values=out)
        if return_resized:
            data["resized"] = res
        return data

    preprocess = __call__


class TrOCRProcessor:
    """transformers' TrOCRProcessor as the reference uses it: `processor(images=..., return_tensors="pt").pixel_values`.  The image half is
    a ViTImageProcessor; the tokenizer half (`batch_decode`) is out of scope."""

    def __init__(self, image_processor=None, device=None, **image_processor_kwargs):
        self.image_processor = image_processor if image_processor is not None else ViTImageProcessor(device=device, **image_processor_kwargs)

    @classmethod
    def from_pretrained(cls, pretrained_model_name_or_path, subfolder=None, device=None, **kw):
        return cls(ViTImageProcessor.from_pretrained(pretrained_model_name_or_path, subfolder=subfolder, device=device))

    def save_pretrained(self, save_directory):
        self.image_processor.save_pretrained(save_directory)

    def __call__(self, images=None, text=None, return_tensors="pt", **kw):
        if text is not None:
            raise NotImplementedError("diffute_amd.TrOCRProcessor: the tokenizer is out of scope; only images= is implemented")
        return self.image_processor(images=images, return_tensors=return_tensors, **kw)

    def batch_decode(self, *a, **kw):
        raise NotImplementedError("diffute_amd.TrOCRProcessor.batch_decode: the tokenizer is out of scope; decode generate()'s ids with "
                                  "transformers' tokenizer")

    decode = batch_decode
