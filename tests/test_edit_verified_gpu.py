"""pipeline.edit_boxes_verified - K candidates per text box, read back by the OCR model, the best-reading one pasted - on the three boxes
of tests/test_edit_boxes_gpu.py with K = 3: every intermediate it returns against the existing function it stands for (the paste ->
slice -> processor chain, a direct ocr.score call at the same chunking, the numpy selection rule, postprocess_batch of the chosen
rows), and across settings against edit_boxes itself.  Tiny UNet / VAE (the configs of tests/test_models_gpu.py), a tiny TrOCR with a
32 x 32 encoder, a 320 x 384 image, S = 128, 3 DDIM steps; batch_size=2 and ocr_batch_size=4 so that both loops end on a short chunk.
`choice` is compared within one run only: across batch plans near-ties may legitimately flip."""
import numpy as np
import pytest
import torch

import readback_restatement as RB
from test_edit_boxes_gpu import BOXES, CROPS, H, ORIGINS, S, STEPS, W
from test_models_gpu import E2E_EMU, TINY_UNET, TINY_VAE
from util import assert_close

pytestmark = pytest.mark.gpu

K, T = 3, 6


@pytest.fixture(scope="module")
def setup(cuda):
    """models, inputs, one K = 3 run with its intermediates and the edit_boxes run it is compared with - computed once, only read"""
    import diffute_amd as D
    from diffute_amd.init import normal
    unet = D.UNet2DConditionModel(**TINY_UNET).cuda().requires_grad_(False)
    vae = D.AutoencoderKL(**TINY_VAE).cuda().requires_grad_(False)
    ocr = D.VisionEncoderDecoderModel(
        D.TrOCREncoder(device=cuda, image_size=32, patch_size=16, hidden_size=256, num_hidden_layers=1, num_attention_heads=4, intermediate_size=256),
        D.TrOCRForCausalLM(device=cuda, d_model=256, decoder_layers=1, decoder_attention_heads=4, decoder_ffn_dim=512, vocab_size=300,
                           max_position_embeddings=64))
    proc = D.TrOCRProcessor(size=32)
    img = torch.from_numpy(np.random.RandomState(11).randint(0, 256, (H, W, 3), dtype=np.uint8)).to(cuda)
    ctx = normal(2, 13, 3 * 77 * 128, cuda).reshape(3, 77, 128)
    enc_noise = normal(4, 71, 3 * 4 * 16 * 16, cuda).reshape(3, 4, 16, 16)
    labels = torch.from_numpy(np.random.RandomState(3).randint(3, 300, (3, T))).to(torch.int64)
    labels[1, 4:] = -100                                    # ragged targets: the score is a mean over the tokens that count
    labels[2, 2:] = -100
    s = dict(unet=unet, vae=vae, ocr=ocr, proc=proc, img=img, ctx=ctx, enc_noise=enc_noise, labels=labels)
    s["res"] = _verified(s)
    s["ref"] = D.edit_boxes(unet, vae, D.DDIMScheduler(), img, BOXES, ctx, STEPS, origins=ORIGINS, crop_scales=CROPS, batch_size=2,
                            enc_noise=enc_noise, return_intermediate=True, size=S)
    D.synchronize()
    return s


def _verified(s, **kw):
    import diffute_amd as D
    a = dict(candidates=K, batch_size=2, ocr_batch_size=4, origins=ORIGINS, crop_scales=CROPS, enc_noise=s["enc_noise"], size=S, return_intermediate=True)
    a.update(kw)
    out = D.edit_boxes_verified(s["unet"], s["vae"], D.DDIMScheduler(), s["ocr"], s["proc"], s["img"], BOXES, s["ctx"], s["labels"], STEPS, **a)
    D.synchronize()
    return out


def test_intermediates_are_what_the_existing_functions_give(cuda, setup):
    import diffute_amd as D
    r, img = setup["res"], setup["img"]
    assert r.image.shape == (H, W, 3) and r.image.dtype == torch.uint8 and r.image_vae.shape == (3, K, 3, S, S)
    assert r.pixel_values.shape == (3 * K, 3, 32, 32) and r.scores.shape == (3, K) and r.choice.shape == (3,) and r.choice.dtype == torch.int32
    # pixel_values: paste -> slice -> processor, per candidate
    slices = []
    for b, (x1, y1, x2, y2) in enumerate(BOXES):
        for k in range(K):
            slices.append(D.prepost.postprocess(r.image_vae[b, k], img, BOXES[b], ORIGINS[b][0], ORIGINS[b][1], CROPS[b])[y1:y2, x1:x2])
    assert torch.equal(r.pixel_values, setup["proc"](images=slices).pixel_values)
    # scores: ocr.score on them at the same chunking, mean log-probability per label token
    lab = setup["labels"].to(cuda).repeat_interleave(K, 0)
    parts = [setup["ocr"].score(r.pixel_values[lo:lo + 4], labels=lab[lo:lo + 4]) for lo in range(0, 3 * K, 4)]
    want = torch.cat([p.sequence_logprobs for p in parts]) / torch.cat([p.num_tokens for p in parts]).clamp(min=1)
    assert torch.equal(r.scores.reshape(-1).view(torch.int32), want.view(torch.int32))
    assert bool(torch.isfinite(r.scores).all()) and bool((r.scores < 0).all())
    assert torch.cat([p.num_tokens for p in parts]).tolist() == [T] * K + [4] * K + [2] * K
    # choice: the numpy rule on the scores; image: the existing batched paste of the chosen rows
    choice = RB.select(r.scores.cpu().numpy())
    assert r.choice.cpu().numpy().tolist() == choice.tolist() and (choice >= 0).all()
    chosen = r.image_vae[torch.arange(3), torch.from_numpy(choice).long()]
    assert torch.equal(r.image, D.prepost.postprocess_batch(chosen, img, BOXES, ORIGINS, CROPS))
    again = D.prepost.preprocess_batch(img, BOXES, ORIGINS, CROPS, size=S)
    assert sorted(r.pre) == sorted(again) and all(torch.equal(r.pre[k], again[k]) for k in again)
    outside = torch.ones(H, W, dtype=torch.bool, device=cuda)
    for x1, y1, x2, y2 in BOXES:
        outside[y1:y2, x1:x2] = False
    assert torch.equal(r.image[outside], img[outside]) and bool((r.image[~outside] != img[~outside]).any())
    # candidates of one box start from different noise and differ from one another
    for b in range(3):
        for k in range(K):
            for j in range(k):
                assert not torch.equal(r.image_vae[b, k], r.image_vae[b, j]), (b, j, k)
    print("edit_boxes_verified scores", r.scores.cpu().numpy().round(4).tolist(), "choice", choice.tolist())


def test_one_candidate_is_edit_boxes_bit_for_bit(cuda, setup):
    one = _verified(setup, candidates=1)
    ref_out, ref_vae, _ = setup["ref"]
    assert torch.equal(one.image_vae[:, 0], ref_vae) and torch.equal(one.image, ref_out)
    assert one.choice.tolist() == [0, 0, 0] and one.scores.shape == (3, 1)
    page = _verified(setup, candidates=1, return_intermediate=False)
    assert torch.equal(page, ref_out)


def test_candidate_0_is_the_reference_start(cuda, setup):
    """seed 0 first: candidate 0 of every box runs edit_boxes' arithmetic under another tile plan (rows of other candidates beside it)"""
    ref_vae = setup["ref"][1].cpu()
    for b in range(3):
        e = assert_close(setup["res"].image_vae[b, 0], ref_vae[b], E2E_EMU, f"box {b}, candidate 0 vs edit_boxes")
        print(f"edit_boxes_verified box {b} candidate 0: rel-L2 {e:.2e} vs edit_boxes")
    other = _verified(setup, seeds=[5, 0, 9])               # the seed, not the position, decides the start
    assert_close(other.image_vae[:, 1], ref_vae, E2E_EMU, "seed 0 as candidate 1 vs edit_boxes")


def test_a_second_run_is_bit_identical(cuda, setup):
    r, again = setup["res"], _verified(setup)
    for name in ("image", "choice", "scores", "image_vae", "pixel_values"):
        assert torch.equal(getattr(again, name), getattr(r, name)), name


def test_min_score_keeps_the_original_where_nothing_reads_well_enough(cuda, setup):
    r = setup["res"]
    none = _verified(setup, min_score=0.0)                  # scores are log-probabilities: all below 0
    assert none.choice.tolist() == [-1, -1, -1] and torch.equal(none.image, setup["img"])
    best = r.scores.max(1).values.cpu().numpy()
    thr = float(np.sort(best)[1])                           # the median best score: the boxes at or above it are pasted, the one below is not
    some = _verified(setup, min_score=thr)
    want = RB.select(some.scores.cpu().numpy(), thr)
    assert some.choice.cpu().numpy().tolist() == want.tolist() and (want < 0).sum() == 1 and torch.equal(some.scores, r.scores)
