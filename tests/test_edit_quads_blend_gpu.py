"""pipeline.edit_quads / edit_quads_verified with blend=QuadBlend(...) on the GPU, with the tiny models of
tests/test_edit_quads_verified_gpu.py: two pages, three quads (two of them overlap), both frames.  The pasted pages equal the integer
restatement (tests/quad_blend_restatement.py) applied to the run's OWN decoder outputs, QuadBlend() gives edit_quads' pages bit for bit
(every quad here lies on its crop: asserted on the CPU first), and nothing outside the grown bounding boxes changes."""
import numpy as np
import pytest
import torch

import quad_blend_cases as BC
import quad_blend_restatement as QB
import quad_cases as QC
import readback_restatement as RB
from test_models_gpu import TINY_UNET, TINY_VAE

pytestmark = pytest.mark.gpu

S, STEPS, K, T = 128, 3, 3, 6
SIZES = [(150, 300), (97, 131)]
QUADS = [[QC.tilted(150, 75, 120, 14, 7), QC.tilted(170, 80, 100, 16, 30)], [[(2, 78), (60, 84), (59, 95), (1, 93)]]]
N = 3
BLEND = dict(feather=4, grow=3, match_color=True, ring=6, max_shift=24)
FRAME_IDS = ["similarity", "projective"]


@pytest.fixture(scope="module")
def setup(cuda):
    import diffute_amd as D
    from diffute_amd.init import normal
    unet = D.UNet2DConditionModel(**TINY_UNET).cuda().requires_grad_(False)
    vae = D.AutoencoderKL(**TINY_VAE).cuda().requires_grad_(False)
    ocr = D.VisionEncoderDecoderModel(
        D.TrOCREncoder(device=cuda, image_size=32, patch_size=16, hidden_size=256, num_hidden_layers=1, num_attention_heads=4, intermediate_size=256),
        D.TrOCRForCausalLM(device=cuda, d_model=256, decoder_layers=1, decoder_attention_heads=4, decoder_ffn_dim=512, vocab_size=300,
                           max_position_embeddings=64))
    rs = np.random.RandomState(11)
    pages = []
    for h, w in SIZES:                                       # a slope under noise: the decoder's tone is off against it
        yy, xx = np.mgrid[0:h, 0:w]
        pages.append(np.clip(100 + (xx * 80) // w + (yy * 30) // h + rs.randint(-15, 16, (h, w)), 0, 255)[:, :, None].repeat(3, 2).astype(np.uint8))
    imgs = [torch.from_numpy(p.copy()).to(cuda) for p in pages]
    ctx = normal(2, 13, N * 77 * 128, cuda).reshape(N, 77, 128)
    enc_noise = normal(4, 71, N * 4 * 16 * 16, cuda).reshape(N, 4, 16, 16)
    labels = torch.from_numpy(np.random.RandomState(3).randint(3, 300, (N, T))).to(torch.int64)
    labels[1, 4:] = -100
    labels[2, 2:] = -100
    return dict(unet=unet, vae=vae, ocr=ocr, proc=D.TrOCRProcessor(size=32), imgs=imgs, pages=pages, ctx=ctx, enc_noise=enc_noise, labels=labels)


def _edit(s, perspective, blend, **kw):
    import diffute_amd as D
    out = D.edit_quads(s["unet"], s["vae"], D.DDIMScheduler(), s["imgs"], QUADS, s["ctx"], STEPS, batch_size=2, enc_noise=s["enc_noise"],
                       return_intermediate=True, size=S, perspective=perspective, blend=blend, **kw)
    D.synchronize()
    return out


def _verified(s, perspective, blend, **kw):
    import diffute_amd as D
    out = D.edit_quads_verified(s["unet"], s["vae"], D.DDIMScheduler(), s["ocr"], s["proc"], s["imgs"], QUADS, s["ctx"], s["labels"], STEPS,
                                candidates=K, batch_size=2, ocr_batch_size=4, enc_noise=s["enc_noise"], size=S, return_intermediate=True,
                                perspective=perspective, blend=blend, **kw)
    D.synchronize()
    return out


def _restated(s, perspective, rows, blend):
    """the restatement's pages for the decoder rows `rows` (one per quad, None = skipped)"""
    from diffute_amd import prepost
    frames = prepost.plan_quads(QUADS, SIZES, perspective, S)
    items = BC.prepared(perspective, QUADS, frames, SIZES, S)
    out, lo = [], 0
    for p, page in enumerate(s["pages"]):
        n = len(QUADS[p])
        out.append(QB.paste_page(page, [items[b] + (rows[b],) for b in range(lo, lo + n)], S, blend))
        lo += n
    return out, items


def _outside_is_untouched(s, pages, blend):
    import diffute_amd as D
    boxes = [blend.grown(qs, h, w) for qs, (h, w) in zip(QUADS, SIZES)]
    assert D.metrics.outside_diff_pages(pages, s["imgs"], boxes).changed.tolist() == [0] * len(SIZES)


@pytest.mark.parametrize("perspective", [False, True], ids=FRAME_IDS)
def test_edit_quads_with_a_blend_is_the_restatement_of_its_own_decoder_outputs(cuda, setup, perspective):
    import diffute_amd as D
    blend = D.QuadBlend(**BLEND)
    pages, image_vae, pre = _edit(setup, perspective, blend)
    plain, plain_vae, _ = _edit(setup, perspective, None)
    assert torch.equal(image_vae, plain_vae), "the blend changes the paste alone"
    rows = image_vae.cpu().numpy()
    want, _ = _restated(setup, perspective, list(rows), QB.Blend(**BLEND))
    for p in range(len(SIZES)):
        assert np.array_equal(pages[p].cpu().numpy(), want[p][0]), f"page {p} differs from the restatement"
        assert all(st[0] > 0 for st in want[p][2])
        assert not torch.equal(pages[p], plain[p]) and not torch.equal(pages[p], setup["imgs"][p])
    _outside_is_untouched(setup, pages, blend)
    only = D.edit_quads(setup["unet"], setup["vae"], D.DDIMScheduler(), setup["imgs"], QUADS, setup["ctx"], STEPS, batch_size=2,
                        enc_noise=setup["enc_noise"], size=S, perspective=perspective, blend=blend)
    assert isinstance(only, list) and all(torch.equal(a, b) for a, b in zip(only, pages))


@pytest.mark.parametrize("perspective", [False, True], ids=FRAME_IDS)
def test_everything_off_is_edit_quads_bit_for_bit(cuda, setup, perspective):
    import diffute_amd as D
    _, items = _restated(setup, perspective, [None] * N, QB.Blend())
    lo = 0
    for p, page in enumerate(setup["pages"]):                # the premise, on the CPU: every pixel of every quad lies on that quad's crop
        n = len(QUADS[p])
        assert QB.covered_off_crop(page, [it + (None,) for it in items[lo:lo + n]], S) == 0
        lo += n
    plain, _, _ = _edit(setup, perspective, None)
    off, _, _ = _edit(setup, perspective, D.QuadBlend())
    assert all(torch.equal(a, b) for a, b in zip(plain, off))
    _outside_is_untouched(setup, off, D.QuadBlend())


@pytest.mark.parametrize("perspective", [False, True], ids=FRAME_IDS)
def test_edit_quads_verified_with_a_blend_skips_and_blends_the_chosen_rows(cuda, setup, perspective):
    """min_score between the lowest and the second-lowest best score of a first run: one quad is skipped.  The pages are the restatement
    of the run's own chosen rows; the scores are those of the hard paste (the blend plays no part in the read-back)"""
    import diffute_amd as D
    blend = D.QuadBlend(**BLEND)
    first = _verified(setup, perspective, None)
    best = np.sort(first.scores.cpu().numpy().max(axis=1))
    min_score = float((best[0] + best[1]) / 2)
    r = _verified(setup, perspective, blend, min_score=min_score)
    assert torch.equal(r.pixel_values, first.pixel_values), "the read-back scores the candidates as the hard paste shows them"
    choice = RB.select(r.scores.cpu().numpy(), min_score)
    assert r.choice.cpu().tolist() == choice.tolist() and (choice < 0).sum() == 1, "one quad below min_score"
    vae = r.image_vae.cpu().numpy()
    rows = [None if k < 0 else vae[b, k] for b, k in enumerate(choice)]
    want, _ = _restated(setup, perspective, rows, QB.Blend(**BLEND))
    for p in range(len(SIZES)):
        assert np.array_equal(r.image[p].cpu().numpy(), want[p][0]), f"page {p} differs from the restatement"
    _outside_is_untouched(setup, r.image, blend)
    hard = _verified(setup, perspective, None, min_score=min_score)
    assert torch.equal(hard.choice, r.choice) and any(not torch.equal(a, b) for a, b in zip(hard.image, r.image))
