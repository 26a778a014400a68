"""Glyph images from text on the GPU (csrc/glyph_text.hip through diffute_amd/glyphs.py), from tests/golden/glyph_text.npz alone - no
Pillow, no font: draw_text bit for bit against Pillow's own canvases and the numpy restatement of the compositing rule
(tests/glyph_text_restatement.py); pixel_values - the one-launch path - bit for bit against the two-launch path, against the processor
fed the fixture's canvases and against the restatement pushed through tests/pil_resample_restatement.py; the refusals of the C-ABI entry;
the edit functions taking strings.  Both builds; every output into a sentinel-filled buffer whose guard bands must survive.

BICUBIC at the 24 x 40 output: the 880-column canvas would need 89 taps per output pixel, more than the processor's cap of 64 (a limit
of dmx_glyph_resize_normalize that this feature inherits) - that one combination is checked to be REFUSED by both paths, the other
cases of the batch run."""
import ctypes

import numpy as np
import pytest
import torch

import glyph_text_cases as C
import glyph_text_restatement as T
import pil_resample_restatement as R

pytestmark = pytest.mark.gpu

CONFIGS = [("bilinear_384", 384, R.BILINEAR), ("bicubic_384", 384, R.BICUBIC),
           ("bilinear_24x40", {"height": 24, "width": 40}, R.BILINEAR), ("bicubic_24x40", {"height": 24, "width": 40}, R.BICUBIC)]
GUARD = 4096
NAN_SENTINEL = 0x7FC0DEAD                      # a NaN no normalisation table holds


def _hw(size):
    return (size, size) if isinstance(size, int) else (size["height"], size["width"])


def _fits(case, size, resample):
    """whether the processor's tap cap (64) admits the case's canvas at this output size"""
    h, w = C.canvas_size(case[1], case[2])
    S_h, S_w = _hw(size)
    unit = 1.0 if resample == R.BILINEAR else 2.0
    return all(n_in == n_out or int(np.ceil(unit * max(n_in / n_out, 1.0))) * 2 + 1 <= 64 for n_in, n_out in ((w, S_w), (h, S_h)))


@pytest.fixture(scope="module")
def ref():
    """the fixture, its atlas, the restatement's canvases and - per processor config - the restatement's resized bytes and pixel_values
    of every case: computed once, read-only"""
    from diffute_amd.glyphs import GlyphAtlas
    g = C.load_golden()
    atlas = GlyphAtlas.from_arrays(g, "atlas.")
    canvas = {}
    for name, text, size, origin in C.CASES:
        canvas[name] = T.draw_text(atlas, text, size, origin)
        canvas[name].setflags(write=False)
    pv = {}
    for cfg, size, resample in CONFIGS:
        for case in C.CASES:
            if _fits(case, size, resample):
                u8, f32 = R.pixel_values(canvas[case[0]], _hw(size), resample)
                u8.setflags(write=False); f32.setflags(write=False)
                pv[cfg, case[0]] = (u8, f32)
    return dict(golden=g, atlas=atlas, canvas=canvas, pv=pv)


@pytest.fixture(params=["bf16", "fp16"])
def build(request, monkeypatch, cuda):
    """route every call of the test through one build of the library"""
    from diffute_amd import _cabi
    real = _cabi.lib
    real(request.param)
    monkeypatch.setattr(_cabi, "lib", lambda elem=None: real(request.param))
    return request.param


def _bits(t):
    return t.cpu().numpy().view(np.uint32)


def _args(cases):
    return [c[1] for c in cases], [C.canvas_size(c[1], c[2]) for c in cases], [c[3] for c in cases]


@pytest.mark.parametrize("cases", [C.BATCH, C.SINGLE, C.CASES[1:2]], ids=["ragged_b8", "b1_clipped", "b1_letter"])
def test_draw_text_equals_pillow_and_the_restatement(cuda, build, ref, cases):
    import diffute_amd as D
    r = D.GlyphRenderer(ref["atlas"], cuda)
    texts, sizes, origins = _args(cases)
    n = sum(h * w * 3 for h, w in sizes)
    for sentinel in (0xA5, 0x5A):              # equal to the expected bytes under two different fills: every element was written
        buf = torch.full((n + 2 * GUARD,), sentinel, dtype=torch.uint8, device=cuda)
        got = r.draw_text(texts, sizes, origins, out=buf[GUARD:GUARD + n])
        D.synchronize()
        assert bool((buf[:GUARD] == sentinel).all()) and bool((buf[GUARD + n:] == sentinel).all()), "guard band overwritten"
        assert len(got) == len(cases) and got[0].data_ptr() == buf.data_ptr() + GUARD
        for c, img, (h, w) in zip(cases, got, sizes):
            assert img.is_cuda and img.dtype == torch.uint8 and tuple(img.shape) == (h, w, 3)
            host = img.cpu().numpy()
            assert np.array_equal(host, C.rgb(ref["golden"]["canvas." + c[0]])), f"{c[0]}: differs from Pillow's canvas"
            assert np.array_equal(host, ref["canvas"][c[0]]), f"{c[0]}: differs from the restatement"
    if sizes == [C.canvas_size(t, None) for t in texts]:                      # the reference's canvas rule is the default
        again = r.draw_text(texts)
        assert all(torch.equal(a, b) for a, b in zip(again, got))


@pytest.mark.parametrize("cfg", CONFIGS, ids=[c[0] for c in CONFIGS])
def test_pixel_values_fused_equals_two_launch_processor_and_restatement(cuda, build, ref, cfg):
    import diffute_amd as D
    name, size, resample = cfg
    r = D.GlyphRenderer(ref["atlas"], cuda)
    proc = D.TrOCRProcessor(size=size, resample=resample)
    S_h, S_w = _hw(size)
    refused = [c for c in C.BATCH if not _fits(c, size, resample)]
    assert [c[0] for c in refused] == (["len20"] if name == "bicubic_24x40" else [])
    if refused:
        for fused in (True, False):
            with pytest.raises(ValueError, match="cap of 64"):
                r.pixel_values(*_args(C.BATCH)[:1], proc, fused=fused)
    for cases in ([c for c in C.BATCH if c not in refused], C.SINGLE):     # the ragged batch, then the B = 1 call
        texts, sizes, origins = _args(cases)
        B = len(cases)
        n = B * 3 * S_h * S_w
        buf = torch.tensor([NAN_SENTINEL], dtype=torch.int32).to(cuda).repeat(n + 2 * GUARD)
        out = buf.view(torch.float32)[GUARD:GUARD + n].view(B, 3, S_h, S_w)
        fused = r.pixel_values(texts, proc, out=out, return_resized=True, fused=True, sizes=sizes, origin=origins)
        D.synchronize()
        assert fused.pixel_values.data_ptr() == out.data_ptr() and fused["resized"].dtype == torch.uint8
        assert bool((buf[:GUARD] == NAN_SENTINEL).all()) and bool((buf[GUARD + n:] == NAN_SENTINEL).all()), "guard band overwritten"
        assert not bool((buf[GUARD:GUARD + n] == NAN_SENTINEL).any()), "an element was left unwritten"
        two = r.pixel_values(texts, proc, return_resized=True, fused=False, sizes=sizes, origin=origins)
        pil = proc(images=[C.rgb(ref["golden"]["canvas." + c[0]]) for c in cases], return_resized=True)
        D.synchronize()
        for k in ("pixel_values", "resized"):
            assert torch.equal(fused[k], two[k]), f"{k}: one launch differs from two"
            assert torch.equal(fused[k], pil[k]), f"{k}: differs from the processor over Pillow's canvases"
        for i, c in enumerate(cases):
            u8, f32 = ref["pv"][name, c[0]]
            assert np.array_equal(fused["resized"][i].cpu().numpy(), u8), f"{c[0]}: resized bytes differ from the restatement"
            assert np.array_equal(_bits(fused.pixel_values[i]), f32.view(np.uint32)), f"{c[0]}: pixel_values differ from the restatement"


def test_a_strip_over_the_lds_budget_takes_the_two_launch_path(cuda, build, ref, monkeypatch):
    """60 -> 3 rows needs 41 source rows per output row, 880 -> 40 columns all 880 of them: 36080 bytes, over the entry's 32768"""
    import diffute_amd as D
    from diffute_amd import _cabi
    r = D.GlyphRenderer(ref["atlas"], cuda)
    proc = D.TrOCRProcessor(size={"height": 3, "width": 40})
    case = C.CASES[6]
    calls = []
    real = r.draw_text
    monkeypatch.setattr(r, "draw_text", lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    got = r.pixel_values([case[1]], proc, fused=True)
    assert calls == [1], "the fused entry was expected to refuse this shape"
    want = r.pixel_values([case[1]], proc, fused=False)
    _, f32 = R.pixel_values(ref["canvas"][case[0]], (3, 40), R.BILINEAR)
    D.synchronize()
    assert torch.equal(got.pixel_values, want.pixel_values) and np.array_equal(_bits(got.pixel_values[0]), f32.view(np.uint32))
    assert 41 * 880 > _cabi.GLYPH_TEXT_LDS_BYTES
    # do_resize=False: the two-launch path, the canvas itself normalised
    plain = r.pixel_values([case[1]], D.TrOCRProcessor(do_resize=False))
    assert len(calls) == 3 and tuple(plain.pixel_values.shape) == (1, 3, 60, 880)
    assert np.array_equal(_bits(plain.pixel_values[0]), R.rescale_normalize(ref["canvas"][case[0]].transpose(2, 0, 1)).view(np.uint32))


def test_the_fused_entry_refuses_before_it_launches(cuda, build, ref):
    """max_taps over the cap and a placement range past the table: an error code, the output untouched; called directly with valid pointers"""
    import diffute_amd as D
    from diffute_amd import _cabi, glyphs, prepost
    lib = _cabi.lib()
    cap = int(lib.dmx_glyph_max_taps())
    r = D.GlyphRenderer(ref["atlas"], cuda)
    ip = D.TrOCRProcessor().image_processor
    _, sizes, places, first, count = glyphs.layout(ref["atlas"], ["rn m"])
    passes, table, max_taps = prepost._readback_tables([(0, 0, w, h) for h, w in sizes], ip, cap)

    def call(max_taps, count):
        items = np.zeros(1, dtype=np.dtype(_cabi.GlyphTextItem))
        items["first"], items["count"], items["H"], items["W"] = first, count, sizes[0][0], sizes[0][1]
        for col, k in enumerate(("h_off", "h_taps", "v_off", "v_taps")):
            items[k] = passes[:, col]
        d_items, d_places = torch.from_numpy(items.view(np.uint8)).to(cuda), torch.from_numpy(places.copy()).to(cuda)
        d_tab, d_norm = torch.from_numpy(table.copy()).to(cuda), torch.from_numpy(ip._norm.copy()).to(cuda)
        out = torch.zeros(1, 3, 384, 384, dtype=torch.float32, device=cuda)
        rc = lib.dmx_glyph_text_pixel_values(ctypes.byref(r._atlas), items.ctypes.data, _cabi.ptr(d_items), places.ctypes.data, _cabi.ptr(d_places),
                                             int(places.shape[0]), 1, _cabi.ptr(d_tab), int(table.size), _cabi.ptr(d_norm), max_taps, 384, 384,
                                             _cabi.ptr(out), None, _cabi.current_stream())
        D.synchronize()
        return rc, out

    rc, out = call(cap + 1, int(count[0]))
    assert rc == _cabi.ERR_ARG and float(out.abs().sum()) == 0.0
    with pytest.raises(RuntimeError, match="exceed the cap of 64"):
        _cabi.check(rc, "glyph_text_pixel_values", lib)
    rc, out = call(max_taps, int(count[0]) + 1)
    assert rc == _cabi.ERR_ARG and float(out.abs().sum()) == 0.0
    with pytest.raises(RuntimeError, match="end past the table"):
        _cabi.check(rc, "glyph_text_pixel_values", lib)
    rc, out = call(max_taps, int(count[0]))                                 # the same call with valid arguments runs
    assert rc == 0 and np.array_equal(_bits(out[0]), R.pixel_values(T.draw_text(ref["atlas"], "rn m"))[1].view(np.uint32))


# ---- strings at the public interface, on the tiny models
H, W, S, STEPS = 320, 384, 128, 2
BOXES = [(40, 60, 150, 78), (200, 150, 330, 180), (60, 250, 140, 266)]
ORIGINS = [(30, 20), (150, 90), (50, 210)]
CROPS = [128, 200, 96]
TEXTS = ["rn m", "AVATAR To.", ""]


@pytest.fixture(scope="module")
def models(cuda, ref):
    import diffute_amd as D
    from diffute_amd.init import normal
    from test_models_gpu import TINY_UNET, TINY_VAE
    unet = D.UNet2DConditionModel(**TINY_UNET).cuda().requires_grad_(False)
    vae = D.AutoencoderKL(**TINY_VAE).cuda().requires_grad_(False)
    enc = D.TrOCREncoder(device=cuda, image_size=32, patch_size=16, hidden_size=TINY_UNET["cross_attention_dim"], num_hidden_layers=1,
                         num_attention_heads=TINY_UNET["cross_attention_dim"] // 64, intermediate_size=256)
    glyph = (D.GlyphRenderer(ref["atlas"], cuda), D.TrOCRProcessor(size=32), enc)
    img = torch.from_numpy(np.random.RandomState(11).randint(0, 256, (H, W, 3), dtype=np.uint8)).to(cuda)
    enc_noise = normal(4, 71, 3 * 4 * 16 * 16, cuda).reshape(3, 4, 16, 16)
    return dict(unet=unet, vae=vae, glyph=glyph, img=img, enc_noise=enc_noise)


def test_glyph_contexts_is_the_reference_chain(cuda, models):
    import diffute_amd as D
    renderer, proc, enc = models["glyph"]
    ctx = D.glyph_contexts(TEXTS, *models["glyph"])
    pv = proc(images=renderer.draw_text(TEXTS)).pixel_values
    want = enc(pv.to(enc.dtype)).last_hidden_state
    D.synchronize()
    assert tuple(ctx.shape) == (3, 5, enc.config.hidden_size) and torch.isfinite(ctx).all() and torch.equal(ctx, want)
    assert not torch.equal(ctx[0], ctx[1])


def test_edit_boxes_and_edit_pages_take_strings(cuda, models):
    import diffute_amd as D
    m = models
    ctx = D.glyph_contexts(TEXTS, *m["glyph"])
    kw = dict(origins=ORIGINS, crop_scales=CROPS, batch_size=2, enc_noise=m["enc_noise"], size=S)
    a = D.edit_boxes(m["unet"], m["vae"], D.DDIMScheduler(), m["img"], BOXES, None, STEPS, texts=TEXTS, glyph=m["glyph"], **kw)
    b = D.edit_boxes(m["unet"], m["vae"], D.DDIMScheduler(), m["img"], BOXES, ctx, STEPS, **kw)
    D.synchronize()
    assert torch.equal(a, b) and not torch.equal(a, m["img"])
    page2 = m["img"][:300, :360].contiguous()
    kw = dict(origins=[ORIGINS[:2], ORIGINS[2:]], crop_scales=[CROPS[:2], CROPS[2:]], batch_size=2, enc_noise=m["enc_noise"], size=S)
    pa = D.edit_pages(m["unet"], m["vae"], D.DDIMScheduler(), [m["img"], page2], [BOXES[:2], BOXES[2:]], None, STEPS, texts=TEXTS,
                      glyph=m["glyph"], **kw)
    pb = D.edit_pages(m["unet"], m["vae"], D.DDIMScheduler(), [m["img"], page2], [BOXES[:2], BOXES[2:]], ctx, STEPS, **kw)
    D.synchronize()
    assert len(pa) == 2 and all(torch.equal(x, y) for x, y in zip(pa, pb))
