"""Glyph images from text strings on the device: the reference's `draw_text` (app.ipynb:347-363, train_diffute_v1.py:352-368 - a white
((len(text)+2)*40) x 60 canvas, black text at (40, 10), font size 40) without Pillow or a font file on the serving machine.

GlyphAtlas (host) holds what FreeType rasterised once: per character the coverage bitmap, its offset and its advance, and the non-zero
pair kernings.  GlyphRenderer turns strings into placements (glyph, x, y) on the host - integer pen arithmetic - and composes them on the
GPU (csrc/glyph_text.hip): draw_text gives the uint8 canvases, pixel_values goes from placements straight to the processor's fp32 batch.

The rule reproduces `ImageDraw.text` under Pillow's BASIC layout bit for bit (tests/test_glyph_text_host.py checks it against a live
Pillow).  RAQM, the default engine of ImageFont.truetype where libraqm is installed, shapes text (ligatures, other positions) and does
NOT follow it: from_font (re)opens the font with layout_engine=BASIC, and a caller whose environment rendered through RAQM keeps that
stage.  Black on white, one line; no stroke, anchors or colours."""
import ctypes
import os

import numpy as np
import torch

from . import _cabi, prepost, processing

PRINTABLE_ASCII = "".join(chr(c) for c in range(32, 127))
_MAX_PAIR_CHARS = 512        # above this many characters the kerning pairs are taken among `kerning_chars` only
_REC_FIELDS = 6              # pool offset, w, h, left, top, advance in 1/64 px: include/diffute_hip.h dmx_glyph_rec


class GlyphAtlas:
    """chars: str of G distinct characters; rec int32 [G,6] = (offset into pool, w, h, left, top, advance in 1/64 px); pool uint8: the
    coverage bitmaps, row-major, back to back; kern_pairs int32 [K,2] (glyph index before, after) / kern_values int32 [K] in 1/64 px."""

    def __init__(self, chars, rec, pool, kern_pairs, kern_values, size, font_name=""):
        self.chars = str(chars)
        self.rec = np.ascontiguousarray(rec, dtype=np.int32).reshape(-1, _REC_FIELDS)
        self.pool = np.ascontiguousarray(pool, dtype=np.uint8).reshape(-1)
        self.kern_pairs = np.ascontiguousarray(kern_pairs, dtype=np.int32).reshape(-1, 2)
        self.kern_values = np.ascontiguousarray(kern_values, dtype=np.int32).reshape(-1)
        self.size, self.font_name = int(size), str(font_name)
        G = len(self.chars)
        if len(set(self.chars)) != G or self.rec.shape[0] != G:
            raise ValueError(f"GlyphAtlas: {G} characters (they must be distinct) but {self.rec.shape[0]} glyph records")
        if self.kern_pairs.shape[0] != self.kern_values.shape[0]:
            raise ValueError("GlyphAtlas: kern_pairs and kern_values differ in length")
        off, w, h = self.rec[:, 0].astype(np.int64), self.rec[:, 1].astype(np.int64), self.rec[:, 2].astype(np.int64)
        if G and (bool((w < 0).any()) or bool((h < 0).any()) or bool((off < 0).any()) or bool((off + w * h > self.pool.size).any())):
            raise ValueError("GlyphAtlas: a glyph's bitmap lies outside the pool")
        if self.kern_pairs.size and (int(self.kern_pairs.min()) < 0 or int(self.kern_pairs.max()) >= G):
            raise ValueError("GlyphAtlas: a kerning pair names a glyph outside the atlas")
        self._index = {c: i for i, c in enumerate(self.chars)}
        self._kern = {(int(a), int(b)): int(v) for (a, b), v in zip(self.kern_pairs, self.kern_values)}

    def __len__(self):
        return len(self.chars)

    # ---- building (the only place Pillow is imported)
    @classmethod
    def from_font(cls, font, size=40, chars=PRINTABLE_ASCII, kerning_chars=None):
        """font: a path, or a PIL.ImageFont.FreeTypeFont (reopened at `size` with the BASIC layout).  Records every character's
        getmask2 bitmap and offset, its advance and every non-zero kerning of an ordered pair of `chars` (for more than 512
        characters: of `kerning_chars`, default none)."""
        from PIL import ImageFont
        if isinstance(font, (str, bytes, os.PathLike)):
            f = ImageFont.truetype(font, size, layout_engine=ImageFont.Layout.BASIC)
        elif isinstance(font, ImageFont.FreeTypeFont):
            f = font.font_variant(size=size, layout_engine=ImageFont.Layout.BASIC)
        else:
            raise TypeError(f"font must be a path or a PIL.ImageFont.FreeTypeFont, got {type(font).__name__}")
        chars = str(chars)
        if len(set(chars)) != len(chars):
            raise ValueError("chars must be distinct")
        bad = [c for c in chars if c in "\n\r"]
        if bad:
            raise ValueError("chars must not hold line breaks: multi-line text is not rendered")
        rec, pool, off = np.zeros((len(chars), _REC_FIELDS), dtype=np.int32), [], 0
        adv = {}
        for i, ch in enumerate(chars):
            mask, (left, top) = f.getmask2(ch, mode="L")
            w, h = mask.size
            a = np.frombuffer(bytes(mask), dtype=np.uint8)[:w * h] if w * h else np.zeros(0, dtype=np.uint8)
            adv[ch] = cls._sixtyfourths(f.getlength(ch), ch)
            rec[i] = (off, w, h, left, top, adv[ch])
            pool.append(a); off += a.size
        among = chars if len(chars) <= _MAX_PAIR_CHARS else str(kerning_chars or "")
        index = {c: i for i, c in enumerate(chars)}
        missing = [c for c in among if c not in index]
        if missing:
            raise ValueError(f"kerning_chars holds {missing[0]!r}, which is not among chars")
        pairs, values = [], []
        for a in among:
            for b in among:
                k = cls._sixtyfourths(f.getlength(a + b), a + b) - adv[a] - adv[b]
                if k:
                    pairs.append((index[a], index[b])); values.append(k)
        name = " ".join(str(s) for s in f.getname() if s)
        return cls(chars, rec, np.concatenate(pool) if pool else np.zeros(0, np.uint8), np.array(pairs, dtype=np.int32).reshape(-1, 2),
                   np.array(values, dtype=np.int32), size, name)

    @staticmethod
    def _sixtyfourths(length, what):
        v = float(length) * 64.0
        if v != round(v):
            raise ValueError(f"the length of {what!r} is no multiple of 1/64 px ({length!r}): not a BASIC-layout FreeType font")
        return int(round(v))

    # ---- persistence: one .npz, no Pillow and no font needed to load
    def save(self, path):
        np.savez_compressed(path, **self.arrays())

    def arrays(self, prefix=""):
        return {prefix + "chars": np.array([ord(c) for c in self.chars], dtype=np.int32), prefix + "rec": self.rec, prefix + "pool": self.pool,
                prefix + "kern_pairs": self.kern_pairs, prefix + "kern_values": self.kern_values,
                prefix + "size": np.int32(self.size), prefix + "font_name": np.array(self.font_name)}

    @classmethod
    def from_arrays(cls, z, prefix=""):
        return cls("".join(chr(int(c)) for c in z[prefix + "chars"]), z[prefix + "rec"], z[prefix + "pool"], z[prefix + "kern_pairs"],
                   z[prefix + "kern_values"], int(z[prefix + "size"]), str(z[prefix + "font_name"]))

    @classmethod
    def load(cls, path):
        with np.load(path, allow_pickle=False) as z:
            return cls.from_arrays(z)

    # ---- layout
    def bitmap(self, g):
        off, w, h = (int(v) for v in self.rec[g, :3])
        return self.pool[off:off + w * h].reshape(h, w)

    def place(self, text, origin=(40, 10)):
        """int32 [n,3] = (glyph index, x, y) of the top-left bitmap pixel of every character of `text` drawn at `origin`: the pen runs
        in 1/64 px - pair kerning before a glyph, its advance after it - and a glyph sits at the pen rounded to the nearest pixel."""
        ox, oy = _int_pair(origin, "origin")
        text = _check_text(text)
        out = np.zeros((len(text), 3), dtype=np.int32)
        pen, prev = 0, None
        for i, ch in enumerate(text):
            g = self._index.get(ch)
            if g is None:
                raise ValueError(f"character {ch!r} (U+{ord(ch):04X}) of {text!r} is not in the atlas")
            if prev is not None:
                pen += self._kern.get((prev, g), 0)
            out[i] = (g, ox + ((pen + 32) >> 6) + int(self.rec[g, 3]), oy + int(self.rec[g, 4]))
            pen += int(self.rec[g, 5])
            prev = g
        return out

    @staticmethod
    def canvas_size(text):
        """(H, W) of the reference's canvas for `text`: 60 x (len(text) + 2) * 40"""
        return 60, (len(_check_text(text)) + 2) * 40

    def to(self, device):
        """the atlas on a GPU: a GlyphRenderer"""
        return GlyphRenderer(self, device)


def _check_text(text):
    if not isinstance(text, str):
        raise TypeError(f"a text must be a str, got {type(text).__name__}")
    for ch in "\n\r":
        if ch in text:
            raise ValueError(f"{text!r} holds a line break ({ch!r}): multi-line text is not rendered")
    return text


def _int_pair(v, name):
    v = tuple(v)
    if len(v) != 2 or any(int(t) != t for t in v):
        raise ValueError(f"{name} must be two integers, got {v}")
    return int(v[0]), int(v[1])


def _check_texts(texts):
    if isinstance(texts, str):
        raise TypeError("texts must be a list of str, not one str")
    texts = list(texts)
    if not texts:
        raise ValueError("texts is empty")
    return [_check_text(t) for t in texts]


def layout(atlas, texts, sizes=None, origin=(40, 10)):
    """the host half of a render, no device involved: -> (texts, sizes [(H, W)], placements int32 [n,3], first [B], count [B]).
    origin: one (x, y) for all texts, or one per text."""
    texts = _check_texts(texts)
    B = len(texts)
    if sizes is None:
        sizes = [atlas.canvas_size(t) for t in texts]
    else:
        sizes = [_int_pair(s, "a size") for s in sizes]
        if len(sizes) != B:
            raise ValueError(f"{B} texts but {len(sizes)} sizes")
        if any(h < 1 or w < 1 for h, w in sizes):
            raise ValueError("a canvas must have at least one pixel")
    origin = list(origin)
    origins = [origin] * B if (len(origin) == 2 and not hasattr(origin[0], "__len__")) else origin
    if len(origins) != B:
        raise ValueError(f"{B} texts but {len(origins)} origins")
    places = [atlas.place(t, o) for t, o in zip(texts, origins)]
    count = np.array([p.shape[0] for p in places], dtype=np.int64)
    first = np.concatenate([[0], np.cumsum(count)[:-1]]).astype(np.int64)
    return texts, sizes, np.concatenate(places).astype(np.int32).reshape(-1, 3), first, count


class GlyphRenderer:
    """GlyphAtlas on one GPU: the bitmap pool and the glyph records are uploaded once; a call uploads the placements and the items."""

    def __init__(self, atlas, device=None):
        if not isinstance(atlas, GlyphAtlas):
            raise TypeError(f"atlas must be a GlyphAtlas, got {type(atlas).__name__}")
        dev = torch.device("cuda" if device is None else device)
        if dev.type != "cuda":
            raise RuntimeError("diffute_amd: the glyph renderer runs on the GPU (cuda / ROCm device); there is no CPU path")
        if dev.index is None:
            dev = torch.device("cuda", torch.cuda.current_device())
        self.atlas, self.device = atlas, dev
        self._rec_host = np.ascontiguousarray(atlas.rec)
        assert self._rec_host.dtype.itemsize * _REC_FIELDS == np.dtype(_cabi.GlyphRec).itemsize
        # pool first, padded to the records' alignment; at least one byte so the pool pointer is never null
        pool_bytes = max(int(atlas.pool.size), 1)
        off_rec = (pool_bytes + 15) // 16 * 16
        host = np.zeros(off_rec + self._rec_host.nbytes, dtype=np.uint8)
        host[:atlas.pool.size] = atlas.pool
        host[off_rec:] = self._rec_host.view(np.uint8).reshape(-1)
        self._buf = torch.from_numpy(host).to(dev)
        self._atlas = _cabi.GlyphAtlas(pool=self._buf.data_ptr(), pool_bytes=pool_bytes, glyphs_host=self._rec_host.ctypes.data,
                                       glyphs_device=self._buf.data_ptr() + off_rec, n_glyphs=len(atlas))

    def to(self, device):
        return self if torch.device(device) == self.device else GlyphRenderer(self.atlas, device)

    # ---- one staging buffer per call: items | placements (+ what the caller appends), one H2D copy
    def _stage(self, sizes, places, first, count, extra=()):
        B = len(sizes)
        items = np.zeros(B, dtype=np.dtype(_cabi.GlyphTextItem))
        items["first"], items["count"] = first, count
        items["H"], items["W"] = [s[0] for s in sizes], [s[1] for s in sizes]
        parts = [items.view(np.uint8).reshape(-1), places.view(np.uint8).reshape(-1)] + [np.ascontiguousarray(e).view(np.uint8).reshape(-1)
                                                                                         for e in extra]
        offs, total = [], 0
        for p in parts:
            offs.append(total)
            total += (p.size + 15) // 16 * 16
        stage = torch.empty(max(total, 16), dtype=torch.uint8, pin_memory=True)
        return items, places, parts, offs, stage

    def _upload(self, parts, offs, stage):
        st = stage.numpy()
        for p, o in zip(parts, offs):
            st[o:o + p.size] = p
        return stage.to(self.device, non_blocking=True)

    def draw_text(self, texts, sizes=None, origin=(40, 10), out=None):
        """the reference's draw_text for a list of strings in ONE launch: a list of uint8 CUDA [H][W][3] tensors (views of one buffer),
        H x W = canvas_size(text) or sizes[i].  origin: (x, y) for all texts or a list of one per text.  out (optional): the buffer,
        a contiguous uint8 CUDA tensor of sum(H * W * 3) elements."""
        texts, sizes, places, first, count = layout(self.atlas, texts, sizes, origin)
        B = len(texts)
        lib = _cabi.lib()
        items, places, parts, offs, stage = self._stage(sizes, places, first, count)
        nbytes = [h * w * 3 for h, w in sizes]
        starts = np.concatenate([[0], np.cumsum(nbytes)]).astype(np.int64)
        with torch.cuda.device(self.device):
            if out is None:
                canvas = torch.empty(int(starts[-1]), dtype=torch.uint8, device=self.device)
            elif not (isinstance(out, torch.Tensor) and out.device == self.device and out.dtype == torch.uint8 and out.is_contiguous()
                      and out.numel() == int(starts[-1])):
                raise ValueError(f"out must be a contiguous uint8 tensor of {int(starts[-1])} elements on {self.device}")
            else:
                canvas = out.view(-1)
            base = canvas.data_ptr()
            items["dst"] = base + starts[:-1]
            items["stride_y"], items["stride_x"], items["stride_c"] = [w * 3 for _, w in sizes], 3, 1
            dbuf = self._upload(parts, offs, stage)
            d = dbuf.data_ptr()
            _cabi.check(lib.dmx_glyph_render(ctypes.byref(self._atlas), items.ctypes.data, d + offs[0], places.ctypes.data, d + offs[1],
                                             int(places.shape[0]), B, _cabi.current_stream()), "glyph_render", lib)
        return [canvas[int(starts[i]):int(starts[i + 1])].view(h, w, 3) for i, (h, w) in enumerate(sizes)]

    def pixel_values(self, texts, processor, out=None, return_resized=False, fused=True, sizes=None, origin=(40, 10)):
        """BatchFeature(pixel_values = fp32 CUDA [B,3,height,width]) exactly as `processor(images=self.draw_text(texts))` returns it;
        processor: a diffute_amd TrOCRProcessor or ViTImageProcessor, whose resample and normalisation tables are used.  fused=True goes
        from the placements to pixel_values in one launch, no canvas in memory; when that entry refuses the shape for its LDS budget -
        and only then - the call takes the two-launch path, draw_text + the processor on the device canvases, which writes the same bytes.
        do_resize=False goes through the two-launch path too."""
        ip = getattr(processor, "image_processor", processor)
        if not isinstance(ip, processing.ViTImageProcessor):
            raise TypeError(f"processor must be a diffute_amd TrOCRProcessor or ViTImageProcessor, got {type(processor).__name__}")
        if not (fused and ip.do_resize):
            return ip(images=self.draw_text(texts, sizes, origin), device=self.device, out=out, return_resized=return_resized)
        texts, sizes, places, first, count = layout(self.atlas, texts, sizes, origin)
        B = len(texts)
        lib = _cabi.lib()
        S_h, S_w = ip.size["height"], ip.size["width"]
        # the processor's own tables, as the read-back builds them: a canvas is the box (0, 0, W, H)
        passes, table, max_taps = prepost._readback_tables([(0, 0, w, h) for h, w in sizes], ip, int(lib.dmx_glyph_max_taps()))
        n_ints = int(table.size)
        items, places, parts, offs, stage = self._stage(sizes, places, first, count, extra=(ip._norm.reshape(-1), table))
        for col, k in enumerate(("h_off", "h_taps", "v_off", "v_taps")):
            items[k] = passes[:, col]
        with torch.cuda.device(self.device):
            if out is None:
                out_t = torch.empty(B, 3, S_h, S_w, dtype=torch.float32, device=self.device)
            elif not (isinstance(out, torch.Tensor) and out.device == self.device and out.dtype == torch.float32 and out.is_contiguous()
                      and tuple(out.shape) == (B, 3, S_h, S_w)):
                raise ValueError(f"out must be a contiguous fp32 tensor [{B},3,{S_h},{S_w}] on {self.device}")
            else:
                out_t = out
            res = torch.empty(B, 3, S_h, S_w, dtype=torch.uint8, device=self.device) if return_resized else None
            dbuf = self._upload(parts, offs, stage)
            d = dbuf.data_ptr()
            rc = lib.dmx_glyph_text_pixel_values(ctypes.byref(self._atlas), items.ctypes.data, d + offs[0], places.ctypes.data, d + offs[1],
                                                 int(places.shape[0]), B, d + offs[3], int(n_ints), d + offs[2], max_taps, S_h, S_w,
                                                 _cabi.ptr(out_t), _cabi.ptr(res), _cabi.current_stream())
        if rc == _cabi.ERR_UNSUPPORTED:          # the strip of one block exceeds the entry's LDS budget: two launches, the same bytes
            return ip(images=self.draw_text(texts, sizes, origin), device=self.device, out=out, return_resized=return_resized)
        _cabi.check(rc, "glyph_text_pixel_values", lib)
        data = processing.BatchFeature(pixel_values=out_t)
        if return_resized:
            data["resized"] = res
        return data


def glyph_contexts(texts, renderer, processor, encoder):
    """[N, L, D] glyph contexts of N strings (app.ipynb:773-776): rendered and resized on the device, then through the OCR encoder"""
    pv = renderer.pixel_values(texts, processor).pixel_values
    return encoder(pv.to(encoder.dtype)).last_hidden_state
