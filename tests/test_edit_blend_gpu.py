"""blend=PasteBlend(...) through the editing functions (pipeline.edit_boxes / edit_pages / edit_boxes_verified; edit_quads refuses it): the
page each returns against the integer restatement (tests/paste_blend_restatement.py) applied to the decoder outputs the same call
returns, bit for bit, and blend=None / PasteBlend() against today's hard paste.  The tiny models, the image and the three boxes of
tests/test_edit_boxes_gpu.py at S = 128, 3 DDIM steps."""
import numpy as np
import pytest
import torch

import paste_blend_restatement as PB
from test_edit_boxes_gpu import BOXES, CROPS, E2E_EMU, H, ORIGINS, S, STEPS, TINY_UNET, TINY_VAE, W
from util import assert_close

pytestmark = pytest.mark.gpu

SOFT = dict(feather=2, grow=2, match_color=True)


@pytest.fixture(scope="module")
def setup(cuda):
    import diffute_amd as D
    from diffute_amd.init import normal
    unet = D.UNet2DConditionModel(**TINY_UNET).cuda().requires_grad_(False)
    vae = D.AutoencoderKL(**TINY_VAE).cuda().requires_grad_(False)
    rs = np.random.RandomState(11)
    img = torch.from_numpy(rs.randint(0, 256, (H, W, 3), dtype=np.uint8)).to(cuda)
    img2 = torch.from_numpy(rs.randint(0, 256, (H - 31, W - 57, 3), dtype=np.uint8)).to(cuda)
    ctx = normal(2, 13, 3 * 77 * 128, cuda).reshape(3, 77, 128)
    enc_noise = normal(4, 71, 3 * 4 * 16 * 16, cuda).reshape(3, 4, 16, 16)
    return dict(unet=unet, vae=vae, img=img, img2=img2, ctx=ctx, enc_noise=enc_noise)


def _boxes(s, **kw):
    import diffute_amd as D
    out = D.edit_boxes(s["unet"], s["vae"], D.DDIMScheduler(), s["img"], BOXES, s["ctx"], STEPS, origins=ORIGINS, crop_scales=CROPS, batch_size=2,
                       enc_noise=s["enc_noise"], size=S, **kw)
    D.synchronize()
    return out


def _restated(page, rows, boxes, origins, crops, blend):
    items = [(None if r is None else r.cpu().numpy(), b, o, c) for r, b, o, c in zip(rows, boxes, origins, crops)]
    return PB.paste_chain(page.cpu().numpy(), items, PB.Blend(**blend))[0]


def test_no_blend_and_an_empty_blend_are_todays_page(cuda, setup):
    import diffute_amd as D
    plain, vae_plain, _ = _boxes(setup, return_intermediate=True)
    none = _boxes(setup, blend=None)
    off, vae_off, _ = _boxes(setup, blend=D.PasteBlend(), return_intermediate=True)
    today = D.prepost.postprocess_batch(vae_plain, setup["img"], BOXES, ORIGINS, CROPS)
    assert torch.equal(vae_off, vae_plain), "the paste must not reach back into the denoise loop"
    assert torch.equal(plain, today) and torch.equal(none, today) and torch.equal(off, today)


def test_edit_boxes_with_a_blend_is_the_restatement_of_its_decoder_outputs(cuda, setup):
    import diffute_amd as D
    blend = D.PasteBlend(**SOFT)
    out, image_vae, _ = _boxes(setup, blend=blend, return_intermediate=True)
    want = _restated(setup["img"], image_vae, BOXES, ORIGINS, CROPS, SOFT)
    assert np.array_equal(out.cpu().numpy(), want)
    assert not torch.equal(out, D.prepost.postprocess_batch(image_vae, setup["img"], BOXES, ORIGINS, CROPS)), "the blend changed nothing"
    diff = D.metrics.outside_diff(out, setup["img"], blend.grown(BOXES, H, W))
    assert int(diff.changed[0]) == 0 and int(diff.sse[0]) == 0
    assert int(D.metrics.outside_diff(out, setup["img"], BOXES).changed[0]) > 0, "grow = 2: the ramp lies around the boxes"


def test_edit_pages_with_a_blend_is_the_restatement_page_by_page(cuda, setup):
    import diffute_amd as D
    blend = D.PasteBlend(**SOFT)
    pages = [setup["img"], setup["img2"]]
    split = lambda l: [l[:2], l[2:]]
    out, image_vae, _ = D.edit_pages(setup["unet"], setup["vae"], D.DDIMScheduler(), pages, split(BOXES), setup["ctx"], STEPS, origins=split(ORIGINS),
                                     crop_scales=split(CROPS), batch_size=2, enc_noise=setup["enc_noise"], size=S, blend=blend, return_intermediate=True)
    D.synchronize()
    for p, (lo, hi) in enumerate(((0, 2), (2, 3))):
        want = _restated(pages[p], image_vae[lo:hi], BOXES[lo:hi], ORIGINS[lo:hi], CROPS[lo:hi], SOFT)
        assert np.array_equal(out[p].cpu().numpy(), want), f"page {p}"
    grown = [blend.grown(b, *pg.shape[:2]) for b, pg in zip(split(BOXES), pages)]
    diff = D.metrics.outside_diff_pages(out, pages, grown)
    assert diff.changed.tolist() == [0, 0]
    # the first page's rows saw the same crops as edit_boxes' rows 0 and 1: the same edit up to the batch plan
    _, vae_boxes, _ = _boxes(setup, blend=blend, return_intermediate=True)
    assert_close(image_vae[:2], vae_boxes[:2].cpu(), E2E_EMU, "edit_pages rows 0, 1 vs edit_boxes")


def test_edit_boxes_verified_pastes_the_restatement_of_the_chosen_rows(cuda, setup):
    import diffute_amd as D
    ocr = D.VisionEncoderDecoderModel(
        D.TrOCREncoder(device=cuda, image_size=32, patch_size=16, hidden_size=256, num_hidden_layers=1, num_attention_heads=4, intermediate_size=256),
        D.TrOCRForCausalLM(device=cuda, d_model=256, decoder_layers=1, decoder_attention_heads=4, decoder_ffn_dim=512, vocab_size=300,
                           max_position_embeddings=64))
    labels = torch.from_numpy(np.random.RandomState(3).randint(3, 300, (3, 6))).to(torch.int64)
    blend = D.PasteBlend(**SOFT)

    def run(**kw):
        r = D.edit_boxes_verified(setup["unet"], setup["vae"], D.DDIMScheduler(), ocr, D.TrOCRProcessor(size=32), setup["img"], BOXES, setup["ctx"],
                                  labels, STEPS, candidates=2, batch_size=2, ocr_batch_size=4, origins=ORIGINS, crop_scales=CROPS,
                                  enc_noise=setup["enc_noise"], size=S, return_intermediate=True, blend=blend, **kw)
        D.synchronize()
        return r
    r = run()
    choice = r.choice.cpu().tolist()
    assert r.image_vae.shape == (3, 2, 3, S, S) and all(k in (0, 1) for k in choice)
    want = _restated(setup["img"], [r.image_vae[b, k] for b, k in enumerate(choice)], BOXES, ORIGINS, CROPS, SOFT)
    assert np.array_equal(r.image.cpu().numpy(), want)
    # a threshold no candidate reaches (the scores are log-probabilities): every box is skipped, the page is the original
    none = run(min_score=0.0)
    assert none.choice.cpu().tolist() == [-1, -1, -1] and torch.equal(none.image, setup["img"])
    # ... and one that only the best box reaches: that box alone is pasted
    best = r.scores.max(dim=1).values.cpu()
    top = best.sort().values
    assert float(top[2]) > float(top[1]), "two boxes read equally well: the threshold below separates nothing"
    some = run(min_score=(float(top[2]) + float(top[1])) / 2)
    sc = some.choice.cpu().tolist()
    assert [k >= 0 for k in sc] == [b == int(best.argmax()) for b in range(3)]
    want = _restated(setup["img"], [some.image_vae[b, k] if k >= 0 else None for b, k in enumerate(sc)], BOXES, ORIGINS, CROPS, SOFT)
    assert np.array_equal(some.image.cpu().numpy(), want)


def test_edit_quads_refuses_a_blend(cuda, setup):
    import diffute_amd as D
    quad = [(40, 60), (150, 60), (150, 78), (40, 78)]
    with pytest.raises(NotImplementedError, match="quads"):
        D.edit_quads(setup["unet"], setup["vae"], D.DDIMScheduler(), [setup["img"]], [[quad]], setup["ctx"][:1], STEPS, size=S,
                     blend=D.PasteBlend(feather=1))
