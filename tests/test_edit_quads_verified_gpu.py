"""pipeline.edit_quads_verified on the GPU with the tiny models of tests/test_edit_verified_gpu.py: two pages, three quads (one page holds
two), K = 3, ragged labels.  Every intermediate equals what the function it stands for gives, one candidate is edit_quads bit for bit in
both frames, and a min_score above every score keeps every page.  `choice` is compared within one run only: the scores of two runs are
bit-equal here (test_edit_verified_gpu.py explains why this is checked per run), but nothing below relies on it."""
import numpy as np
import pytest
import torch

import quad_cases as QC
import readback_restatement as RB
from test_models_gpu import TINY_UNET, TINY_VAE

pytestmark = pytest.mark.gpu

S, STEPS, K, T = 128, 3, 3, 6
SIZES = [(150, 300), (97, 131)]
QUADS = [[QC.tilted(150, 75, 120, 14, 7), QC.tilted(170, 80, 100, 16, 30)], [[(2, 78), (60, 84), (59, 95), (1, 93)]]]
N = 3


@pytest.fixture(scope="module")
def setup(cuda):
    """models, inputs and one K = 3 run with its intermediates: computed once, only read"""
    import diffute_amd as D
    from diffute_amd.init import normal
    unet = D.UNet2DConditionModel(**TINY_UNET).cuda().requires_grad_(False)
    vae = D.AutoencoderKL(**TINY_VAE).cuda().requires_grad_(False)
    ocr = D.VisionEncoderDecoderModel(
        D.TrOCREncoder(device=cuda, image_size=32, patch_size=16, hidden_size=256, num_hidden_layers=1, num_attention_heads=4, intermediate_size=256),
        D.TrOCRForCausalLM(device=cuda, d_model=256, decoder_layers=1, decoder_attention_heads=4, decoder_ffn_dim=512, vocab_size=300,
                           max_position_embeddings=64))
    proc = D.TrOCRProcessor(size=32)
    rs = np.random.RandomState(11)
    imgs = [torch.from_numpy(rs.randint(0, 256, (h, w, 3), dtype=np.uint8)).to(cuda) for h, w in SIZES]
    ctx = normal(2, 13, N * 77 * 128, cuda).reshape(N, 77, 128)
    enc_noise = normal(4, 71, N * 4 * 16 * 16, cuda).reshape(N, 4, 16, 16)
    labels = torch.from_numpy(np.random.RandomState(3).randint(3, 300, (N, T))).to(torch.int64)
    labels[1, 4:] = -100                                    # ragged targets: the score is a mean over the tokens that count
    labels[2, 2:] = -100
    s = dict(unet=unet, vae=vae, ocr=ocr, proc=proc, imgs=imgs, ctx=ctx, enc_noise=enc_noise, labels=labels)
    s["res"] = _verified(s)
    return s


def _verified(s, **kw):
    import diffute_amd as D
    a = dict(candidates=K, batch_size=2, ocr_batch_size=4, enc_noise=s["enc_noise"], size=S, return_intermediate=True)
    a.update(kw)
    out = D.edit_quads_verified(s["unet"], s["vae"], D.DDIMScheduler(), s["ocr"], s["proc"], s["imgs"], QUADS, s["ctx"], s["labels"], STEPS, **a)
    D.synchronize()
    return out


def test_intermediates_are_what_the_existing_functions_give(cuda, setup):
    import diffute_amd as D
    r, imgs = setup["res"], setup["imgs"]
    frames = D.prepost.plan_quads(QUADS, SIZES)
    assert isinstance(r.image, list) and [tuple(p.shape) for p in r.image] == [s + (3,) for s in SIZES] and r.image_vae.shape == (N, K, 3, S, S)
    assert r.pixel_values.shape == (N * K, 3, 32, 32) and r.scores.shape == (N, K) and r.choice.shape == (N,) and r.choice.dtype == torch.int32
    # pixel_values: paste alone -> rectify -> processor, per candidate
    flat = [(p, q, f) for p, (qs, fs) in enumerate(zip(QUADS, frames)) for q, f in zip(qs, fs)]
    strips = []
    for b, (p, q, f) in enumerate(flat):
        for k in range(K):
            pasted = D.prepost.postprocess_quads(r.image_vae[b, k][None], [imgs[p]], [[q]], [[f]])
            strips += D.prepost.rectify_quads(pasted, [[q]])
    assert torch.equal(r.pixel_values, setup["proc"](images=strips).pixel_values)
    # scores: ocr.score on them at the same chunking, mean log-probability per label token
    lab = setup["labels"].to(cuda).repeat_interleave(K, 0)
    parts = [setup["ocr"].score(r.pixel_values[lo:lo + 4], labels=lab[lo:lo + 4]) for lo in range(0, N * K, 4)]
    want = torch.cat([p.sequence_logprobs for p in parts]) / torch.cat([p.num_tokens for p in parts]).clamp(min=1)
    assert torch.equal(r.scores.reshape(-1).view(torch.int32), want.view(torch.int32))
    assert bool(torch.isfinite(r.scores).all()) and bool((r.scores < 0).all())
    # choice: the numpy rule on the scores of THIS run; pages: the existing quad paste of the chosen rows
    choice = RB.select(r.scores.cpu().numpy())
    assert r.choice.cpu().numpy().tolist() == choice.tolist() and (choice >= 0).all()
    chosen = r.image_vae[torch.arange(N), torch.from_numpy(choice).long()]
    want_pages = D.prepost.postprocess_quads(chosen, imgs, QUADS, frames)
    assert all(torch.equal(a, b) for a, b in zip(r.image, want_pages))
    again = D.prepost.preprocess_quads(imgs, QUADS, frames, size=S)
    assert sorted(r.pre) == sorted(again) and all(torch.equal(r.pre[k], again[k]) for k in again)
    assert all(bool((a != b).any()) for a, b in zip(r.image, imgs))
    print("edit_quads_verified scores", r.scores.cpu().numpy().round(4).tolist(), "choice", choice.tolist())


@pytest.mark.parametrize("perspective", [False, True], ids=["similarity", "projective"])
def test_one_candidate_is_edit_quads_bit_for_bit(cuda, setup, perspective):
    import diffute_amd as D
    s = setup
    ref_pages, ref_vae, _ = D.edit_quads(s["unet"], s["vae"], D.DDIMScheduler(), s["imgs"], QUADS, s["ctx"], STEPS, batch_size=2,
                                         enc_noise=s["enc_noise"], return_intermediate=True, size=S, perspective=perspective)
    one = _verified(s, candidates=1, perspective=perspective)
    assert torch.equal(one.image_vae[:, 0], ref_vae) and all(torch.equal(a, b) for a, b in zip(one.image, ref_pages))
    assert one.choice.tolist() == [0] * N and one.scores.shape == (N, 1)
    pages = _verified(s, candidates=1, perspective=perspective, return_intermediate=False)
    assert isinstance(pages, list) and all(torch.equal(a, b) for a, b in zip(pages, ref_pages))


def test_min_score_above_every_score_keeps_every_page(cuda, setup):
    none = _verified(setup, min_score=0.0)                  # scores are log-probabilities: all below 0
    assert none.choice.tolist() == [-1] * N and all(torch.equal(a, b) for a, b in zip(none.image, setup["imgs"]))
    assert torch.equal(none.scores, setup["res"].scores)


def test_a_blend_is_refused(cuda, setup):
    import diffute_amd as D
    with pytest.raises(NotImplementedError):
        _verified(setup, blend=D.PasteBlend())
