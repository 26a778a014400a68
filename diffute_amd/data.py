"""Synthetic document pages as training data: what stands in for the reference's private dataset (train_diffute_v1.py:418-505 OursDataset
reads page images and OCR json from OSS; the README says the data "will not be publicly available").

SyntheticDocuments lays pages of text lines out on the host from a GlyphAtlas - every string, pen position and ink box is known - and
composes them on the GPU in one launch (csrc/page_compose.hip, include/diffute_hip.h dmx_page_compose): a textured background, then every
line blended in its ink with Pillow's ImageDraw.text arithmetic.  A record carries `document`, a list of {"text", "box", "score"} in the
shape of the OCR json the reference's __getitem__ reads (train_diffute_v1.py:444-453).  sample_boxes makes the choice __getitem__ makes
(train_diffute_v1.py:445-489: one confident line, its hull, the lower edge extended, the text truncated to the crop, a random crop
origin); training_batch turns pages and boxes into the dict train_step takes.

Limits: one atlas is one font at one size, so every line of a dataset has the same font size; sizes are (H, W) as everywhere in this
package; pages whose short side is below the crop are refused (the reference upscales them; these pages are made large enough)."""
import ctypes

import numpy as np
import torch

from . import _cabi, glyphs, prepost

_SCORE_KEEP = 0.8             # train_diffute_v1.py:447: lines with score > 0.8 are candidates


def _atlas_of(renderer):
    return renderer if isinstance(renderer, glyphs.GlyphAtlas) else renderer.atlas


def ink_extent(atlas, places):
    """(x0, y0, x1, y1), upper corner exclusive, of the bitmaps of placements int32 [n,3]; None if none of them has a pixel"""
    if places.shape[0] == 0:
        return None
    w, h = atlas.rec[places[:, 0], 1].astype(np.int64), atlas.rec[places[:, 0], 2].astype(np.int64)
    keep = (w > 0) & (h > 0)
    if not keep.any():
        return None
    x, y = places[keep, 1].astype(np.int64), places[keep, 2].astype(np.int64)
    return int(x.min()), int(y.min()), int((x + w[keep]).max()), int((y + h[keep]).max())


def page_tables(atlas, records):
    """the three host tables of one dmx_page_compose launch over `records`: (pages [P] dmx_page_rec without destinations, lines
    dmx_page_line, placements int32 [n,3])"""
    records = list(records)
    pages = np.zeros(len(records), dtype=np.dtype(_cabi.PageRec))
    n_lines = sum(len(r["lines"]) for r in records)
    lines = np.zeros(n_lines, dtype=np.dtype(_cabi.PageLine))
    places, l, n = [], 0, 0
    for p, r in enumerate(records):
        H, W = (int(v) for v in r["size"])
        pg = pages[p]
        pg["H"], pg["W"], pg["first_line"], pg["n_lines"] = H, W, l, len(r["lines"])
        pg["tex_seed"], pg["tex_amp"], pg["bg"] = int(r.get("tex_seed", 0)) & 0xFFFFFFFF, int(r.get("tex_amp", 0)), tuple(int(v) for v in r["bg"])
        for ln in r["lines"]:
            pl = atlas.place(ln["text"], ln["pen"])
            box = ink_extent(atlas, pl) or (0, 0, 0, 0)
            lines[l]["first"], lines[l]["count"], lines[l]["rgb"] = n, pl.shape[0], tuple(int(v) for v in ln["ink"])
            lines[l]["x0"], lines[l]["y0"], lines[l]["x1"], lines[l]["y1"] = box
            places.append(pl); n += pl.shape[0]; l += 1
    places = np.concatenate(places).astype(np.int32).reshape(-1, 3) if places else np.zeros((0, 3), dtype=np.int32)
    return pages, lines, np.ascontiguousarray(places)


def compose_pages(renderer, records, dst=None, out=None):
    """`records` (dicts with size, bg, tex_seed, tex_amp, lines of text / pen / ink) composed in ONE launch.  dst: None - the pages are
    written as uint8 CUDA [H][W][3] tensors, views of one buffer (`out`, optional: a contiguous uint8 CUDA tensor of sum(H * W * 3)
    elements), and returned as a list; or one (address, stride_y, stride_x, stride_c) per page, bytes, for destinations of the caller's
    own layout (planar, strided) - nothing is returned then."""
    records = list(records)
    if not records:
        raise ValueError("no pages to compose")
    if not isinstance(renderer, glyphs.GlyphRenderer):
        raise TypeError(f"renderer must be a GlyphRenderer, got {type(renderer).__name__}")
    pages, lines, places = page_tables(renderer.atlas, records)
    P = len(records)
    parts = [a.view(np.uint8).reshape(-1) for a in (pages, lines, places)]
    offs, total = [], 0
    for a in parts:
        offs.append(total)
        total += (a.size + 15) // 16 * 16
    stage = torch.empty(max(total, 16), dtype=torch.uint8, pin_memory=True)
    views = None
    with torch.cuda.device(renderer.device):
        if dst is None:
            sizes = [(int(r["size"][0]), int(r["size"][1])) for r in records]
            starts = np.concatenate([[0], np.cumsum([h * w * 3 for h, w in sizes])]).astype(np.int64)
            if out is None:
                buf = torch.empty(int(starts[-1]), dtype=torch.uint8, device=renderer.device)
            elif not (isinstance(out, torch.Tensor) and out.device == renderer.device and out.dtype == torch.uint8 and out.is_contiguous()
                      and out.numel() == int(starts[-1])):
                raise ValueError(f"out must be a contiguous uint8 tensor of {int(starts[-1])} elements on {renderer.device}")
            else:
                buf = out.view(-1)
            pages["dst"] = buf.data_ptr() + starts[:-1]
            pages["stride_y"], pages["stride_x"], pages["stride_c"] = [w * 3 for _, w in sizes], 3, 1
            views = [buf[int(starts[i]):int(starts[i + 1])].view(h, w, 3) for i, (h, w) in enumerate(sizes)]
        else:
            dst = list(dst)
            if len(dst) != P:
                raise ValueError(f"{P} pages but {len(dst)} destinations")
            for k, name in enumerate(("dst", "stride_y", "stride_x", "stride_c")):
                pages[name] = [int(d[k]) for d in dst]
        dbuf = renderer._upload(parts, offs, stage)                     # pages | lines | placements: one H2D copy
        d = dbuf.data_ptr()
        lib = _cabi.lib()
        _cabi.check(lib.dmx_page_compose(ctypes.byref(renderer._atlas), pages.ctypes.data, d + offs[0], P, lines.ctypes.data, d + offs[1],
                                         int(lines.shape[0]), places.ctypes.data, d + offs[2], int(places.shape[0]), _cabi.current_stream()),
                    "page_compose", lib)
    return views


def _randint(rng, lo, hi):
    """an integer in [lo, hi) from a numpy Generator or a RandomState / the numpy.random module"""
    return int(rng.integers(lo, hi)) if hasattr(rng, "integers") else int(rng.randint(lo, hi))


def train_crop_origin(lo_edge, hi_edge, crop_scale, rng):
    """one axis of the training crop (train_diffute_v1.py:470-487) for a box side [lo_edge, hi_edge] shorter than the crop: uniform in
    [max(0, hi_edge - crop_scale), lo_edge), and 0 where that range is empty.  (prepost.crop_origin is the NOTEBOOK's rule - it places the
    crop deterministically when the box is short - and says something else.)"""
    lo = max(0, hi_edge - crop_scale)
    return _randint(rng, lo, lo_edge) if lo < lo_edge else 0


def sample_boxes(records, rng, crop_scale=256):
    """The choice OursDataset.__getitem__ makes for every page (train_diffute_v1.py:445-489), on `rng` in page order - per page the line,
    then the x origin, then the y origin where they are drawn: among the lines of `document` with score > 0.8 one at random; the
    axis-aligned hull (x1, y1, x2, y2) of its four points; y2 + (y2 - y1) / 10, at most H - 1; truncated to int32; a box at least as wide
    (then: as tall) as the crop starts the crop and keeps the first int(len(text) * crop_scale / side) characters, a shorter one gets a
    random origin (train_crop_origin).  Returns (locations, origins, texts): P lists of one box, P lists of one origin - what
    prepost.preprocess_pages takes with crop_scales [[crop_scale]] * P - and the P strings glyph_contexts takes."""
    locations, origins, texts = [], [], []
    crop_scale = int(crop_scale)
    for p, r in enumerate(records):
        H, W = (int(v) for v in r["size"])
        if min(H, W) < crop_scale:
            raise ValueError(f"page {p}: {H} x {W} is smaller than the crop of {crop_scale}; the reference's upscaling of small pages is not implemented")
        doc = [d for d in r["document"] if d["score"] > _SCORE_KEEP]
        if not doc:
            raise ValueError(f"page {p}: no line with score > {_SCORE_KEEP}")
        d = doc[_randint(rng, 0, len(doc))]
        xs, ys = [pt[0] for pt in d["box"]], [pt[1] for pt in d["box"]]
        x1, y1, x2, y2 = min(xs), min(ys), max(xs), max(ys)
        y2 = min(y2 + (y2 - y1) / 10, H - 1)
        x1, y1, x2, y2 = (int(v) for v in np.int32([x1, y1, x2, y2]))
        text = d["text"]
        if x2 - x1 < crop_scale:
            x_s = train_crop_origin(x1, x2, crop_scale, rng)
        else:
            x_s, text = x1, text[:int(len(text) * crop_scale / (x2 - x1))]
        if y2 - y1 < crop_scale:
            y_s = train_crop_origin(y1, y2, crop_scale, rng)
        else:
            y_s, text = y1, text[:int(len(text) * crop_scale / (y2 - y1))]
        locations.append([(x1, y1, x2, y2)]); origins.append([(x_s, y_s)]); texts.append(text)
    return locations, origins, texts


def _check_dropout(context_dropout):
    p = float(context_dropout)
    if not 0.0 <= p <= 1.0:
        raise ValueError(f"context_dropout = {context_dropout!r}: a probability in [0, 1]")
    return p


def training_batch(pages, locations, origins, texts, glyph, size=512, crop_scale=256, context_dropout=0.0, drop_rng=None):
    """The dict train_step takes - pixel_values, masked_images fp32 [B,3,size,size], masks uint8 [B,1,size,size], ocr_embeddings [B,L,D] -
    for one box on each of B device pages: prepost.preprocess_pages (the crop of `crop_scale` resized to `size`, the reference's training
    transform) and glyph_contexts(texts, *glyph), glyph = (renderer, processor, encoder); nothing else.

    context_dropout = p > 0: the training half of classifier-free guidance - with probability p a row's ocr_embeddings are replaced by
    zeros, the default unconditional context of Guidance.  One uniform draw per row from `drop_rng` (a numpy Generator, required then), in
    row order; row b is dropped where its draw is below p.  With the default 0.0 nothing is drawn and the batch is what it always was."""
    p = _check_dropout(context_dropout)
    if p > 0.0 and drop_rng is None:
        raise ValueError("context_dropout > 0 needs drop_rng (a numpy Generator)")
    pre = prepost.preprocess_pages(pages, locations, origins, [[int(crop_scale)]] * len(pages), size)
    ctx = glyphs.glyph_contexts(texts, *glyph)
    if p > 0.0:
        drop = drop_rng.random(ctx.shape[0]) < p
        if drop.any():
            ctx = ctx.clone()
            ctx[torch.from_numpy(drop).to(ctx.device)] = 0
    return dict(pixel_values=pre["image"], masked_images=pre["masked_image"], masks=pre["mask"], ocr_embeddings=ctx)


_LETTERS = "abcdefghijklmnopqrstuvwxyzABCDEFGHIJKLMNOPQRSTUVWXYZ0123456789"


class SyntheticDocuments:
    """ds[i]: page i as a record - a pure function of (seed, i).  renderer: a GlyphRenderer (or, for layout alone, a GlyphAtlas).
    page_size: (H, W), or a callable of the page's numpy Generator returning it (ragged pages); lines: (fewest, most) lines of a page -
    fewer where the page is too short for them; chars: the characters words are made of (default: the atlas's letters and digits), the
    atlas must hold them and the space; tex_amp: amplitude of the background texture.

    A record: size (H, W); bg (r, g, b); tex_seed; tex_amp; lines: [{"text", "pen": (x, y), "ink": (r, g, b)}] top to bottom;
    document: [{"text", "box": [[x, y] * 4], "score"}], the box being the corners - first and last pixel, inclusive - of the line's ink
    extent as the atlas lays it out (the hull of its glyph bitmaps; it holds every inked pixel).  Line boxes are pairwise disjoint and
    inside the page; ink is dark on a light page, for one page in five light on a dark one; scores are uniform in [0.5, 1), so about
    two lines in five fall under the reference's 0.8, and at least one line of a page lies above it."""

    def __init__(self, renderer, *, page_size=(1100, 1300), lines=(8, 24), seed=0, chars=None, tex_amp=6):
        self.renderer = renderer if isinstance(renderer, glyphs.GlyphRenderer) else None
        self.atlas = _atlas_of(renderer)
        if not isinstance(self.atlas, glyphs.GlyphAtlas):
            raise TypeError(f"renderer must be a GlyphRenderer or a GlyphAtlas, got {type(renderer).__name__}")
        self.page_size = page_size if callable(page_size) else (int(page_size[0]), int(page_size[1]))
        self.lines = (int(lines[0]), int(lines[1]))
        if not 1 <= self.lines[0] <= self.lines[1]:
            raise ValueError(f"lines = {lines}: expected 1 <= fewest <= most")
        self.seed, self.tex_amp = int(seed), int(tex_amp)
        if not 0 <= self.tex_amp <= 255:
            raise ValueError(f"tex_amp = {tex_amp}: expected 0 .. 255")
        self.chars = "".join(c for c in _LETTERS if c in self.atlas.chars) if chars is None else str(chars)
        missing = [c for c in self.chars + " " if c not in self.atlas.chars]
        if missing or not self.chars.replace(" ", ""):
            raise ValueError(f"chars needs at least one non-space character, and the atlas must hold all of them and the space (missing: {missing})")
        self.chars = self.chars.replace(" ", "")
        self.glyph = None             # (renderer, processor, encoder) for batches(); set it, or pass glyph= there

    # ---- layout (host)
    def _line_text(self, rng, room):
        """words until the line has a random number of them or the next one would leave `room` pixels; -> (text, extent at pen (0, 0))"""
        text, ext = "", None
        for _ in range(int(rng.integers(1, 9))):
            word = "".join(self.chars[int(k)] for k in rng.integers(0, len(self.chars), int(rng.integers(1, 11))))
            cand = word if not text else text + " " + word
            e = ink_extent(self.atlas, self.atlas.place(cand, (0, 0)))
            while not text and e is not None and e[2] - e[0] > room and len(cand) > 1:      # a first word too long for the page is cut
                cand = cand[:-1]
                e = ink_extent(self.atlas, self.atlas.place(cand, (0, 0)))
            if e is None or e[2] - e[0] > room:
                break
            text, ext = cand, e
        return text, ext

    def __getitem__(self, i):
        i = int(i)
        if i < 0:
            raise IndexError("page indices start at 0")
        rng = np.random.default_rng([self.seed, i])
        H, W = (int(v) for v in (self.page_size(rng) if callable(self.page_size) else self.page_size))
        margin = min(24, H // 8, W // 8)
        light = bool(rng.random() >= 0.2)
        bg = tuple(int(v) for v in (rng.integers(215, 256, 3) if light else rng.integers(0, 51, 3)))
        tex_seed = int(rng.integers(0, 1 << 32))
        made = []
        for _ in range(int(rng.integers(self.lines[0], self.lines[1] + 1))):
            indent = int(rng.integers(0, max(W // 4, 1)))
            text, ext = self._line_text(rng, W - 2 * margin - indent)
            if text:
                ink = tuple(int(v) for v in (rng.integers(0, 91, 3) if light else rng.integers(180, 256, 3)))
                made.append((text, ext, indent, ink, float(rng.uniform(0.5, 1.0))))
        # stack top to bottom: drop lines from the end until the ink heights and one free row between neighbours fit, then hand the
        # free rows out at random - the first share above the first line, one share above every later line, the last below the last line
        room = H - 2 * margin
        while made and sum(e[3] - e[1] for _, e, _, _, _ in made) + len(made) - 1 > room:
            made.pop()
        free = room - sum(e[3] - e[1] for _, e, _, _, _ in made) - max(len(made) - 1, 0)
        cuts = np.sort(rng.integers(0, free + 1, len(made))) if made else np.zeros(0, dtype=np.int64)
        lines, document, y, taken = [], [], margin, 0
        for k, (text, e, indent, ink, score) in enumerate(made):
            y += int(cuts[k]) - taken + (1 if k else 0)
            taken = int(cuts[k])
            x = margin + indent
            pen = (x - e[0], y - e[1])
            x2, y2 = x + e[2] - e[0], y + e[3] - e[1]
            lines.append({"text": text, "pen": pen, "ink": ink})
            document.append({"text": text, "box": [[x, y], [x2 - 1, y], [x2 - 1, y2 - 1], [x, y2 - 1]], "score": score})
            y = y2
        if document and not any(d["score"] > _SCORE_KEEP for d in document):
            document[0]["score"] = 0.5 * (1.0 + _SCORE_KEEP)
        return {"size": (H, W), "bg": bg, "tex_seed": tex_seed, "tex_amp": self.tex_amp, "lines": lines, "document": document}

    # ---- device
    def _need_renderer(self):
        if self.renderer is None:
            raise RuntimeError("diffute_amd: this SyntheticDocuments was built from a GlyphAtlas; composing pages needs a GlyphRenderer (atlas.to(device))")
        return self.renderer

    def compose(self, records, out=None):
        """the records' pages as uint8 CUDA [H][W][3] tensors (views of one buffer; `out`: that buffer), one dmx_page_compose launch"""
        return compose_pages(self._need_renderer(), records, out=out)

    def batches(self, B, rng, glyph=None, size=512, crop_scale=256, start=0, context_dropout=0.0):
        """an endless iterator of train_step batches of B pages each, pages start, start + 1, ...: compose, sample_boxes, training_batch.
        glyph = (renderer, processor, encoder), default self.glyph; rng draws the boxes and origins.  context_dropout: training_batch's;
        the rows dropped from the batch that starts at page i come from np.random.default_rng([seed, i, 1]) - a function of the
        dataset's seed and the batch's first page alone, never of `rng`."""
        context_dropout = _check_dropout(context_dropout)
        glyph = self.glyph if glyph is None else glyph
        if glyph is None:
            raise ValueError("batches needs (renderer, processor, encoder) for the glyph contexts: pass glyph= or set ds.glyph")
        i = int(start)
        while True:
            records = [self[i + k] for k in range(B)]
            i += B
            pages = self.compose(records)
            locations, origins, texts = sample_boxes(records, rng, crop_scale)
            drop_rng = np.random.default_rng([self.seed, i - B, 1]) if context_dropout > 0.0 else None
            yield training_batch(pages, locations, origins, texts, glyph, size, crop_scale, context_dropout, drop_rng)
