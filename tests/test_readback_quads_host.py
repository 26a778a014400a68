"""The host half of the verified edits for quads (prepost.readback_pixel_values_quads / postprocess_select_quads,
pipeline.edit_quads_verified): the new symbols are declared and bound, every refusal of the four entries fires through the host-only
checks with dummy device addresses (they return before they launch) and names the item, the strips' resample tables are what the box
read-back's are, the restatement is sane on an axis-aligned quad, and every argument error of edit_quads_verified is raised before
anything is launched.  Nothing here needs a GPU."""
import ctypes
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import persp_cases as PC
import quad_cases as QC
import quad_restatement as QR
import readback_quads_cases as C
import readback_quads_restatement as RQ

S, PAGES = C.S, C.PAGES
ENTRIES = ["dmx_readback_pixel_values_quads", "dmx_readback_pixel_values_quads_persp", "dmx_postprocess_paste_select_quads",
           "dmx_postprocess_paste_select_quads_persp"]
DEV = 4096                                                  # a dummy device address: no entry reads through it before its checks


def test_the_new_symbols_are_declared_and_bound():
    from diffute_amd import _cabi
    for elem in ("bf16", "fp16"):
        lib = _cabi.lib(elem)
        for name in ENTRIES:
            assert name in _cabi.exported_symbols() and getattr(lib, name).argtypes is not None, name
    import diffute_amd as D
    assert "edit_quads_verified" in D.__all__ and callable(D.edit_quads_verified)
    assert callable(D.prepost.readback_pixel_values_quads) and callable(D.prepost.postprocess_select_quads)


class _Call:
    """the arguments of the four entries over prepared tables with dummy addresses; every field can be spoiled before call()"""

    def __init__(self, perspective, size=32):
        from diffute_amd import _cabi, prepost, processing
        self.lib, self.perspective = _cabi.lib(), perspective
        names, quads, frames = C.lists(perspective)
        self.B, self.P = sum(len(q) for q in quads), len(PAGES)
        if perspective:
            self.pt, self.qt, self.xt = PC.tables(PAGES, quads, frames)
        else:
            (self.pt, self.qt), self.xt = QC.tables(PAGES, quads, frames), None
        _cabi.check(self.lib.dmx_edit_quads_prepare(self.pt, self.P, self.qt, self.B, S), "edit_quads_prepare")
        if perspective:
            _cabi.check(self.lib.dmx_edit_quads_persp_prepare(self.pt, self.P, self.qt, self.xt, self.B, S), "edit_quads_persp_prepare")
        ip = processing.ViTImageProcessor(size=size)
        passes, tables, self.max_taps = prepost._readback_tables([(0, 0, q.rw, q.rh) for q in self.qt], ip, 64, "quad")
        self.passes = (_cabi.ReadbackPass * self.B)()
        ctypes.memmove(self.passes, np.ascontiguousarray(passes).ctypes.data, passes.nbytes)
        self.table_ints, self.K, self.size, self.threshold = int(tables.size), 2, size, float("-inf")
        self.names = [n for page in names for n in page]

    def _tables(self):
        t = (self.pt, DEV, self.P, self.qt, DEV)
        return t + ((self.xt, DEV) if self.perspective else ())

    def readback(self):
        fn = getattr(self.lib, "dmx_readback_pixel_values_quads" + ("_persp" if self.perspective else ""))
        rc = fn(DEV, S, *self._tables(), self.B, self.K, DEV, self.table_ints, DEV, self.passes, DEV, self.max_taps, self.size, self.size, DEV, None,
                None)
        return rc, self.lib.dmx_last_error().decode()

    def select(self):
        fn = getattr(self.lib, "dmx_postprocess_paste_select_quads" + ("_persp" if self.perspective else ""))
        rc = fn(DEV, S, DEV, self.threshold, DEV, *self._tables(), self.B, self.K, None)
        return rc, self.lib.dmx_last_error().decode()


@pytest.mark.parametrize("perspective", [False, True], ids=["similarity", "projective"])
def test_every_refusal_fires_before_a_launch_and_names_the_item(perspective):
    for k in (0, 17):
        c = _Call(perspective)
        c.K = k
        for rc, msg in (c.readback(), c.select()):
            assert rc != 0 and f"{k} candidates" in msg, msg
    c = _Call(perspective)
    c.threshold = float("nan")
    rc, msg = c.select()
    assert rc != 0 and "NaN" in msg
    # the pass tables, by item: one that ends past table_ints, one that must be skipped but is not, one with too many taps
    item = 2
    c = _Call(perspective)
    c.table_ints = c.passes[item].h_off + 10
    rc, msg = c.readback()
    assert rc != 0 and "ends past" in msg and "item" in msg
    c = _Call(perspective)
    skipped = c.names.index("rw_is_32")
    assert c.passes[skipped].h_off < 0 and c.qt[skipped].rw == 32, "rw == S_w: the table builder skips the pass"
    c.passes[skipped].h_off, c.passes[skipped].h_taps = 0, 3
    rc, msg = c.readback()
    assert rc != 0 and f"item {skipped}:" in msg and "must be skipped" in msg, msg
    c = _Call(perspective)
    c.passes[item].v_taps = c.max_taps + 1
    rc, msg = c.readback()
    assert rc != 0 and f"item {item}:" in msg and "taps" in msg, msg
    c = _Call(perspective)
    c.max_taps = 65
    rc, msg = c.readback()
    assert rc != 0 and "cap of 64" in msg
    # an unprepared quad table: a derived field that does not belong to the quad
    for call in ("readback", "select"):
        c = _Call(perspective)
        c.qt[5].rw += 1
        rc, msg = getattr(c, call)()
        assert rc != 0 and "item 5:" in msg and "dmx_edit_quads_prepare" in msg, msg
        c = _Call(perspective)
        c.pt[1].block_lo += 1
        rc, msg = getattr(c, call)()
        assert rc != 0 and "page 1" in msg, msg
    c = _Call(perspective)                                  # the select paste writes pages: it needs their addresses
    c.pt[2].out = 0
    rc, msg = c.select()
    assert rc != 0 and "page 2" in msg, msg
    if perspective:
        for call in ("readback", "select"):
            c = _Call(perspective)                          # a window the projective prepare refuses: the horizon crosses 4x the strip
            c.xt[0].crop_scale = 60000
            rc, msg = getattr(c, call)()
            assert rc != 0 and "item 0:" in msg, msg
            c = _Call(perspective)                          # a prepared map that was touched afterwards
            c.xt[3].paste.t[0] += 1
            rc, msg = getattr(c, call)()
            assert rc != 0 and "item 3:" in msg and "dmx_edit_quads_persp_prepare" in msg, msg
    # null arguments
    c = _Call(perspective)
    c.passes = None
    assert c.readback()[0] != 0 and "null" in c.readback()[1]


def test_the_strips_share_tables_by_size_and_skip_equal_sizes():
    from diffute_amd import prepost, processing
    ip = processing.ViTImageProcessor(size=32)
    boxes = [(0, 0, 121, 15), (0, 0, 32, 7), (0, 0, 121, 15), (0, 0, 16, 32), (0, 0, 15, 121)]
    passes, tables, max_taps = prepost._readback_tables(boxes, ip, 64, "quad")
    assert passes[1, 0] == -1 and passes[3, 2] == -1, "rw == S_w / rh == S_h: offset -1"
    assert passes[0].tolist() == passes[2].tolist(), "strips of equal size share their tables"
    assert passes[4, 0] == passes[0, 2] and passes[4, 2] == passes[0, 0], "a table is keyed by (in, out, filter), whichever axis asks"
    one = prepost._readback_tables(boxes[:1], ip, 64, "quad")[1]
    assert tables.size < 3 * one.size and max_taps == passes[:, [1, 3]].max()
    with pytest.raises(ValueError, match="quad 1: resizing 3000 -> 32"):
        prepost._readback_tables([(0, 0, 100, 10), (0, 0, 3000, 10)], ip, 64, "quad")
    with pytest.raises(ValueError, match="box 0"):
        prepost._readback_tables([(0, 0, 3000, 10)], ip, 64)


def test_the_restatement_on_an_axis_aligned_quad_is_the_slice_of_the_pasted_page():
    from diffute_amd import _cabi
    h, w = PAGES[0]
    x1, y1, x2, y2 = 20, 20, 50, 32
    quad, frame = QC.box_quad(x1, y1, x2, y2), (2 * 15 + S - 1, 2 * 10 + S - 1, S, 1, 0)           # the crop is page[10:74, 15:79]: it covers the quad
    pt, qt = QC.tables([(h, w)], [[quad]], [[frame]])
    _cabi.check(_cabi.lib().dmx_edit_quads_prepare(pt, 1, qt, 1, S), "edit_quads_prepare")
    q = QR.from_table(qt[0])
    rs = np.random.RandomState(3)
    page, vae = rs.randint(0, 256, (h, w, 3), dtype=np.uint8), (rs.rand(3, S, S) * 2.4 - 1.2).astype(np.float32)
    pasted = RQ.pasted_alone(page, q, vae, S)
    strip = RQ.strip(page, q, vae, S)
    assert strip.shape == (y2 - y1 + 1, x2 - x1 + 1, 3) and np.array_equal(strip, pasted[y1:y2 + 1, x1:x2 + 1])
    assert (strip != page[y1:y2 + 1, x1:x2 + 1]).any() and np.array_equal(pasted[:y1], page[:y1])
    want = np.clip(np.rint((vae[:, 10:23, 5:36] / 2 + 0.5) * 255), 0, 255).astype(np.uint8).transpose(1, 2, 0)   # crop_scale = S: a copy, clamped
    assert np.array_equal(strip, want)
    sel = RQ.select_paste(page, [q], [vae[None]], np.array([[-1.0]], np.float32), 0.0, S)
    assert sel["choice"].tolist() == [-1] and np.array_equal(sel["out"], page) and sel["union"].sum() == (y2 - y1 + 1) * (x2 - x1 + 1)


def _ocr(image_size=32, vocab=300, positions=64):
    return SimpleNamespace(encoder=SimpleNamespace(config=SimpleNamespace(image_size=image_size)),
                           decoder=SimpleNamespace(config=SimpleNamespace(vocab_size=vocab, max_position_embeddings=positions)))


def test_edit_quads_verified_raises_every_argument_error_before_anything_is_launched(monkeypatch):
    """the models are never reached (None stands in for them) and neither is prepost: each of its stage functions would raise"""
    import diffute_amd as D
    from diffute_amd import pipeline, prepost

    def reached(*a, **kw):
        raise AssertionError("a prepost stage was reached before the arguments were checked")
    for name in ("preprocess_quads", "readback_pixel_values_quads", "postprocess_select_quads", "postprocess_quads", "plan_quads"):
        monkeypatch.setattr(prepost, name, reached)
    assert pipeline.prepost is prepost
    imgs = [torch.zeros(h, w, 3, dtype=torch.uint8) for h, w in PAGES[:2]]
    quads = [[QC.box_quad(20, 20, 50, 32), QC.tilted(150, 75, 120, 14, 7)], [QC.box_quad(10, 10, 60, 30)]]
    ctx = torch.zeros(3, 77, 128)
    labels = torch.full((3, 5), -100, dtype=torch.int64)
    labels[:, :2] = 7
    proc = D.TrOCRProcessor(size=32)

    def run(exc, **kw):
        a = dict(ocr=_ocr(), processor=proc, images=imgs, quads=quads, encoder_hidden_states=ctx, labels=labels)
        a.update(kw)
        named = {k: a.pop(k) for k in list(a) if k not in ("ocr", "processor", "images", "quads", "encoder_hidden_states", "labels")}
        with pytest.raises(exc):
            D.edit_quads_verified(None, None, None, a["ocr"], a["processor"], a["images"], a["quads"], a["encoder_hidden_states"], a["labels"], 3,
                                  **dict(dict(size=S), **named))
    run(ValueError, quads=quads[:1])
    run(ValueError, quads=[[], []])
    run(ValueError, quads=[quads[0] * 33, quads[1]])                        # 67 quads
    run(ValueError, frames=[[(0, 0, 64, 1, 0)]])
    run(ValueError, frames=[[(0, 0, 64, 1, 0)], [(0, 0, 64, 1, 0)]])
    run(TypeError, images=[imgs[0], None])
    run(ValueError, candidates=0)
    run(ValueError, candidates=17)
    run(ValueError, candidates=3, seeds=[0, 1])
    run(ValueError, min_score=float("nan"))
    run(ValueError, batch_size=0)
    run(ValueError, ocr_batch_size=0)
    run(NotImplementedError, blend=D.PasteBlend())
    run(ValueError, cache_interval=0)
    run(ValueError, encoder_hidden_states=ctx[:2])
    run(ValueError, encoder_hidden_states=None)
    run(ValueError, texts=["a", "b", "c"])                                  # both contexts given
    run(ValueError, labels=labels.to(torch.int32))
    run(ValueError, labels=labels[:2])
    run(ValueError, labels=torch.full((3, 65), 7, dtype=torch.int64))
    run(ValueError, labels=torch.full((3, 5), 300, dtype=torch.int64))
    run(ValueError, processor=D.TrOCRProcessor(size=48))
    run(ValueError, processor=D.ViTImageProcessor(size=32, do_resize=False))
    run(ValueError, size=60)
