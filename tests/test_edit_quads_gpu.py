"""pipeline.edit_quads - skewed and rotated text lines on several pages as one batch - against the manual chain preprocess_quads ->
edit_latents per chunk (init_latents = the seed-0 draw) -> postprocess_quads, bit for bit.  Tiny UNet / VAE (the configs of
tests/test_models_gpu.py), three pages with 2 + 1 + 1 quads, S = 128, 2 DDIM steps, batch_size=3: the first chunk spans all three pages
and the last chunk has one row."""
import numpy as np
import pytest
import torch

import quad_cases as QC
from test_models_gpu import TINY_UNET, TINY_VAE

pytestmark = pytest.mark.gpu

S, STEPS, BS = 128, 2, 3
PAGES = [(320, 384), (200, 260), (384, 150)]                      # h x w
QUADS = [[QC.tilted(120, 90, 140, 18, 7), QC.tilted(250, 220, 120, 24, -15)], [QC.tilted(130, 100, 100, 16, 30)],
         [[(90, 60), (90, 200), (66, 200), (66, 60)]]]           # the last one is read top to bottom
N = 4


@pytest.fixture(scope="module")
def setup(cuda):
    """models, inputs and one edit_quads run - computed once, only read by the tests"""
    import diffute_amd as D
    from diffute_amd.init import normal
    unet = D.UNet2DConditionModel(**TINY_UNET).cuda().requires_grad_(False)
    vae = D.AutoencoderKL(**TINY_VAE).cuda().requires_grad_(False)
    rs = np.random.RandomState(11)
    imgs = [torch.from_numpy(rs.randint(0, 256, (h, w, 3), dtype=np.uint8)).to(cuda) for h, w in PAGES]
    ctx = normal(2, 13, N * 77 * 128, cuda).reshape(N, 77, 128)
    enc_noise = normal(4, 71, N * 4 * 16 * 16, cuda).reshape(N, 4, 16, 16)
    frames = D.prepost.plan_quads(QUADS, PAGES)
    s = dict(unet=unet, vae=vae, imgs=imgs, ctx=ctx, enc_noise=enc_noise, frames=frames)
    s["run"] = D.edit_quads(unet, vae, D.DDIMScheduler(), imgs, QUADS, ctx, STEPS, frames=frames, batch_size=BS, enc_noise=enc_noise,
                            return_intermediate=True, size=S)
    D.synchronize()
    return s


def _inside(quad, h, w, cuda):
    """the quad's own pixels, edges included, from the edge functions in int64 torch arithmetic"""
    Y, X = torch.meshgrid(torch.arange(h, device=cuda), torch.arange(w, device=cuda), indexing="ij")
    ok = torch.ones(h, w, dtype=torch.bool, device=cuda)
    for k in range(4):
        (x0, y0), (x1, y1) = quad[k], quad[(k + 1) % 4]
        ok &= (x1 - x0) * (Y - y0) - (y1 - y0) * (X - x0) >= 0
    return ok


def test_edit_quads_is_the_manual_chain(cuda, setup):
    import diffute_amd as D
    s = setup
    out, image_vae, pre = s["run"]
    assert isinstance(out, list) and len(out) == 3 and image_vae.shape == (N, 3, S, S)
    want_pre = D.prepost.preprocess_quads(s["imgs"], QUADS, s["frames"], size=S)
    assert sorted(pre) == sorted(want_pre) and all(torch.equal(pre[k], want_pre[k]) for k in pre)
    init = torch.randn((1, 4, S // 8, S // 8), generator=torch.manual_seed(0), dtype=torch.float32).to(cuda)      # app.ipynb:796-801
    chunks = []
    for lo in range(0, N, BS):                               # rows 0 .. 2 lie on three pages
        hi = min(N, lo + BS)
        chunks.append(D.edit_latents(s["unet"], s["vae"], D.DDIMScheduler(), want_pre["image"][lo:hi], want_pre["masked_image"][lo:hi],
                                     want_pre["mask"][lo:hi], s["ctx"][lo:hi], STEPS, init_latents=init.expand(hi - lo, -1, -1, -1).contiguous(),
                                     enc_noise=s["enc_noise"][lo:hi]).clone())
    want_vae = torch.cat(chunks, 0)
    assert torch.equal(image_vae, want_vae), "image_vae differs from edit_latents over the chunks"
    want = D.prepost.postprocess_quads(want_vae, s["imgs"], QUADS, s["frames"])
    D.synchronize()
    for p, (h, w) in enumerate(PAGES):
        assert out[p].shape == (h, w, 3) and out[p].dtype == torch.uint8 and torch.equal(out[p], want[p]), f"page {p}"
        covered = torch.zeros(h, w, dtype=torch.bool, device=cuda)
        for q in QUADS[p]:
            covered |= _inside(q, h, w, cuda)
        assert torch.equal(out[p][~covered], s["imgs"][p][~covered]), "pixels outside all quads must be untouched"
        assert (out[p][covered] != s["imgs"][p][covered]).any() and 1000 < int(covered.sum()) < h * w // 10
    plain = D.edit_quads(s["unet"], s["vae"], D.DDIMScheduler(), s["imgs"], QUADS, s["ctx"], STEPS, frames=s["frames"], batch_size=BS,
                         enc_noise=s["enc_noise"], size=S)
    assert isinstance(plain, list) and all(torch.equal(a, b) for a, b in zip(plain, out))


def test_frames_none_plans_what_plan_quads_gives(cuda, setup):
    import diffute_amd as D
    s = setup
    out, image_vae, pre = D.edit_quads(s["unet"], s["vae"], D.DDIMScheduler(), s["imgs"], QUADS, s["ctx"], STEPS, batch_size=BS,
                                       enc_noise=s["enc_noise"], return_intermediate=True, size=S)
    D.synchronize()
    ref_out, ref_vae, ref_pre = s["run"]
    assert all(torch.equal(pre[k], ref_pre[k]) for k in ref_pre) and torch.equal(image_vae, ref_vae)
    assert all(torch.equal(a, b) for a, b in zip(out, ref_out))


def test_texts_and_glyph(cuda, setup):
    """texts= / glyph= instead of encoder_hidden_states: the contexts are glyph_contexts(texts, *glyph)"""
    import diffute_amd as D
    s = setup
    import glyph_text_cases as C
    from diffute_amd.glyphs import GlyphAtlas
    renderer = D.GlyphRenderer(GlyphAtlas.from_arrays(C.load_golden(), "atlas."), cuda)
    proc = D.TrOCRProcessor(size=32)
    enc = D.TrOCREncoder(device=cuda, image_size=32, patch_size=16, hidden_size=TINY_UNET["cross_attention_dim"], num_hidden_layers=1,
                         num_attention_heads=TINY_UNET["cross_attention_dim"] // 64, intermediate_size=256)
    texts = ["rn m", "AVATAR To.", "", "To."]
    ctx = D.glyph_contexts(texts, renderer, proc, enc)
    a = D.edit_quads(s["unet"], s["vae"], D.DDIMScheduler(), s["imgs"], QUADS, None, 1, texts=texts, glyph=(renderer, proc, enc), batch_size=BS,
                     enc_noise=s["enc_noise"], size=S)
    b = D.edit_quads(s["unet"], s["vae"], D.DDIMScheduler(), s["imgs"], QUADS, ctx, 1, batch_size=BS, enc_noise=s["enc_noise"], size=S)
    D.synchronize()
    assert all(torch.equal(x, y) for x, y in zip(a, b))


def test_mismatched_lists_raise_before_any_launch(cuda, setup):
    """None stands in for the models: a call that got as far as a launch would fail with another error"""
    import diffute_amd as D
    s = setup

    def run(exc, images=s["imgs"], quads=QUADS, ctx=s["ctx"], **kw):
        with pytest.raises(exc):
            D.edit_quads(None, None, None, images, quads, ctx, STEPS, size=S, **kw)
    run(ValueError, images=s["imgs"][:2])
    run(ValueError, quads=QUADS[:2])
    run(ValueError, frames=s["frames"][:2])
    run(ValueError, frames=[s["frames"][0][:1], s["frames"][1], s["frames"][2]])
    run(ValueError, ctx=s["ctx"][:3])
    run(ValueError, batch_size=0)
    run(ValueError, quads=[QUADS[0], [], QUADS[2]], ctx=s["ctx"][:3])
    run(ValueError, texts=["a"] * N)
