"""pipeline.edit_pages / edit_pages_verified - text boxes on SEVERAL pages as one batch - against the per-box loop over the single-box
chain preprocess -> edit_latents(init_latents = the seed-0 draw) -> postprocess on each box's own page, and against edit_boxes /
the paged prepost functions bit for bit.  Tiny UNet / VAE (the configs of tests/test_models_gpu.py), the tiny TrOCR of
tests/test_edit_verified_gpu.py, three pages of different sizes with 2 + 1 + 1 boxes, S = 128, 3 DDIM steps, batch_size=3: the first
chunk spans all three pages and the last chunk has one row.  The batch runs the loop's arithmetic under another tile plan (B = 3
instead of 1): the bound is test_models_gpu's E2E_EMU, as in tests/test_edit_boxes_gpu.py."""
import numpy as np
import pytest
import torch

import readback_restatement as RB
from test_models_gpu import E2E_EMU, TINY_UNET, TINY_VAE
from util import assert_close

pytestmark = pytest.mark.gpu

S, STEPS, K, T = 128, 3, 2, 6
PAGES = [(320, 384), (200, 260), (384, 150)]                      # h x w
BOXES = [[(40, 60, 150, 78), (200, 150, 330, 180)], [(60, 120, 140, 136)], [(20, 300, 120, 320)]]
ORIGINS = [[(30, 20), (150, 90)], [(50, 70)], [(10, 250)]]
CROPS = [[128, 200], [96], [128]]                                 # identity, downscale, upscale, identity at S = 128
FLAT = [(p, j) for p in range(3) for j in range(len(BOXES[p]))]
N = len(FLAT)


@pytest.fixture(scope="module")
def setup(cuda):
    """models, inputs, the per-box loop's decoder outputs and one edit_pages run - computed once, only read by the tests"""
    import diffute_amd as D
    from diffute_amd.init import normal
    unet = D.UNet2DConditionModel(**TINY_UNET).cuda().requires_grad_(False)
    vae = D.AutoencoderKL(**TINY_VAE).cuda().requires_grad_(False)
    rs = np.random.RandomState(11)
    imgs = [torch.from_numpy(rs.randint(0, 256, (h, w, 3), dtype=np.uint8)).to(cuda) for h, w in PAGES]
    ctx = normal(2, 13, N * 77 * 128, cuda).reshape(N, 77, 128)
    enc_noise = normal(4, 71, N * 4 * 16 * 16, cuda).reshape(N, 4, 16, 16)
    init = torch.randn((1, 4, S // 8, S // 8), generator=torch.manual_seed(0), dtype=torch.float32).to(cuda)      # app.ipynb:796-801
    loop_vae = []
    for b, (p, j) in enumerate(FLAT):
        pre = D.prepost.preprocess(imgs[p], BOXES[p][j], ORIGINS[p][j][0], ORIGINS[p][j][1], CROPS[p][j], size=S)
        loop_vae.append(D.edit_latents(unet, vae, D.DDIMScheduler(), pre["image"], pre["masked_image"], pre["mask"], ctx[b:b + 1], STEPS,
                                       init_latents=init, enc_noise=enc_noise[b:b + 1]).clone())
    s = dict(unet=unet, vae=vae, imgs=imgs, ctx=ctx, enc_noise=enc_noise, loop_vae=torch.cat(loop_vae, 0).cpu())
    s["run"] = D.edit_pages(unet, vae, D.DDIMScheduler(), imgs, BOXES, ctx, STEPS, origins=ORIGINS, crop_scales=CROPS, batch_size=3,
                            enc_noise=enc_noise, return_intermediate=True, size=S)
    D.synchronize()
    return s


@pytest.fixture(scope="module")
def ocr_setup(cuda, setup):
    import diffute_amd as D
    ocr = D.VisionEncoderDecoderModel(
        D.TrOCREncoder(device=cuda, image_size=32, patch_size=16, hidden_size=256, num_hidden_layers=1, num_attention_heads=4, intermediate_size=256),
        D.TrOCRForCausalLM(device=cuda, d_model=256, decoder_layers=1, decoder_attention_heads=4, decoder_ffn_dim=512, vocab_size=300,
                           max_position_embeddings=64))
    labels = torch.from_numpy(np.random.RandomState(3).randint(3, 300, (N, T))).to(torch.int64)
    labels[1, 4:] = -100                                    # ragged targets: the score is a mean over the tokens that count
    labels[3, 2:] = -100
    return dict(ocr=ocr, proc=D.TrOCRProcessor(size=32), labels=labels)


def _verified(s, o, **kw):
    import diffute_amd as D
    a = dict(candidates=K, batch_size=3, ocr_batch_size=3, origins=ORIGINS, crop_scales=CROPS, enc_noise=s["enc_noise"], size=S, return_intermediate=True)
    a.update(kw)
    out = D.edit_pages_verified(s["unet"], s["vae"], D.DDIMScheduler(), o["ocr"], o["proc"], s["imgs"], BOXES, s["ctx"], o["labels"], STEPS, **a)
    D.synchronize()
    return out


def test_edit_pages_matches_the_per_box_loop(cuda, setup):
    import diffute_amd as D
    out, image_vae, pre = setup["run"]
    imgs = setup["imgs"]
    assert image_vae.shape == (N, 3, S, S) and isinstance(out, list) and len(out) == 3
    e = assert_close(image_vae, setup["loop_vae"], E2E_EMU, "edit_pages(batch_size=3) image_vae vs the per-box loop")
    for b, (p, j) in enumerate(FLAT):
        eb = assert_close(image_vae[b], setup["loop_vae"][b], E2E_EMU, f"box {j} of page {p}")
        print(f"edit_pages page {p} box {j}: rel-L2 {eb:.2e} vs the single-box chain")
    print(f"edit_pages batch_size=3: image_vae rel-L2 {e:.2e} vs the per-box loop")
    # the preprocess dict is the paged preprocess of the original pages: row b is the single-box kernel on its own page
    again = D.prepost.preprocess_pages(imgs, BOXES, ORIGINS, CROPS, size=S)
    assert sorted(pre) == sorted(again) and all(torch.equal(pre[k], again[k]) for k in pre)
    # every returned page is the chain of single pastes of the returned decoder outputs over that page's boxes, bit for bit
    b = 0
    for p, (h, w) in enumerate(PAGES):
        assert out[p].shape == (h, w, 3) and out[p].dtype == torch.uint8
        chain, outside = imgs[p], torch.ones(h, w, dtype=torch.bool, device=cuda)
        for j, (x1, y1, x2, y2) in enumerate(BOXES[p]):
            chain = D.prepost.postprocess(image_vae[b:b + 1], chain, BOXES[p][j], ORIGINS[p][j][0], ORIGINS[p][j][1], CROPS[p][j])
            outside[y1:y2, x1:x2] = False
            b += 1
        assert torch.equal(out[p], chain), f"page {p} differs from the chain of single pastes"
        assert torch.equal(out[p][outside], imgs[p][outside]), "pixels outside all boxes must be untouched"
        assert (out[p][~outside] != imgs[p][~outside]).any()


def test_one_page_is_edit_boxes_bit_for_bit(cuda, setup):
    import diffute_amd as D
    s = setup
    kw = dict(origins=ORIGINS[0], crop_scales=CROPS[0], batch_size=3, enc_noise=s["enc_noise"][:2], return_intermediate=True, size=S)
    ref_out, ref_vae, ref_pre = D.edit_boxes(s["unet"], s["vae"], D.DDIMScheduler(), s["imgs"][0], BOXES[0], s["ctx"][:2], STEPS, **kw)
    kw.update(origins=ORIGINS[:1], crop_scales=CROPS[:1])
    out, image_vae, pre = D.edit_pages(s["unet"], s["vae"], D.DDIMScheduler(), s["imgs"][:1], BOXES[:1], s["ctx"][:2], STEPS, **kw)
    D.synchronize()
    assert len(out) == 1 and torch.equal(out[0], ref_out) and torch.equal(image_vae, ref_vae)
    assert all(torch.equal(pre[k], ref_pre[k]) for k in ref_pre)
    page = D.edit_pages(s["unet"], s["vae"], D.DDIMScheduler(), s["imgs"][:1], BOXES[:1], s["ctx"][:2], STEPS, origins=ORIGINS[:1],
                        crop_scales=CROPS[:1], batch_size=3, enc_noise=s["enc_noise"][:2], size=S)
    assert isinstance(page, list) and torch.equal(page[0], ref_out)


def test_edit_pages_plans_the_crops_itself(cuda, setup):
    """origins / crop_scales left out: prepost.plan_pages' plan, page after page on one rng stream"""
    import diffute_amd as D
    s = setup
    boxes = [BOXES[0], BOXES[1] + [(5, 100, 255, 104)], BOXES[2]]        # wider than page 1's short side: its x origin is drawn
    ctx = torch.cat([s["ctx"], s["ctx"][:1]], 0)
    plans = D.prepost.plan_pages(boxes, PAGES, np.random.RandomState(3))
    origins, crops = [[p[:2] for p in pl] for pl in plans], [[p[2] for p in pl] for pl in plans]
    out, image_vae, pre = D.edit_pages(s["unet"], s["vae"], D.DDIMScheduler(), s["imgs"], boxes, ctx, 1, rng=np.random.RandomState(3), batch_size=4,
                                       return_intermediate=True, size=S)
    want = D.prepost.preprocess_pages(s["imgs"], boxes, origins, crops, size=S)
    assert all(torch.equal(pre[k], want[k]) for k in want)
    pages = D.prepost.postprocess_pages(image_vae, s["imgs"], boxes, origins, crops)
    assert all(torch.equal(a, b) for a, b in zip(out, pages))


def test_verified_intermediates_are_what_the_paged_functions_give(cuda, setup, ocr_setup):
    import diffute_amd as D
    s, o = setup, ocr_setup
    r = _verified(s, o)
    assert isinstance(r.image, list) and [tuple(p.shape) for p in r.image] == [(h, w, 3) for h, w in PAGES]
    assert r.image_vae.shape == (N, K, 3, S, S) and r.pixel_values.shape == (N * K, 3, 32, 32) and r.scores.shape == (N, K)
    assert r.choice.shape == (N,) and r.choice.dtype == torch.int32
    # scores: ocr.score on readback_pixel_values_pages' rows at the same chunking, mean log-probability per label token
    pv = D.prepost.readback_pixel_values_pages(r.image_vae, s["imgs"], BOXES, ORIGINS, CROPS, o["proc"])
    assert torch.equal(r.pixel_values, pv)
    lab = o["labels"].to(cuda).repeat_interleave(K, 0)
    parts = [o["ocr"].score(pv[lo:lo + 3], labels=lab[lo:lo + 3]) for lo in range(0, N * K, 3)]
    want = torch.cat([p.sequence_logprobs for p in parts]) / torch.cat([p.num_tokens for p in parts]).clamp(min=1)
    assert torch.equal(r.scores.reshape(-1).view(torch.int32), want.view(torch.int32))
    assert bool(torch.isfinite(r.scores).all()) and bool((r.scores < 0).all())
    # choice: the host arg-max of the returned scores; pages: postprocess_select_pages of the returned tensors
    choice = RB.select(r.scores.cpu().numpy())
    assert r.choice.cpu().numpy().tolist() == choice.tolist() and (choice >= 0).all()
    pages, choice2 = D.prepost.postprocess_select_pages(r.image_vae, r.scores, s["imgs"], BOXES, ORIGINS, CROPS)
    assert torch.equal(choice2, r.choice) and all(torch.equal(a, b) for a, b in zip(r.image, pages))
    again = D.prepost.preprocess_pages(s["imgs"], BOXES, ORIGINS, CROPS, size=S)
    assert all(torch.equal(r.pre[k], again[k]) for k in again)
    for b in range(N):
        assert not torch.equal(r.image_vae[b, 0], r.image_vae[b, 1]), "candidates of one box start from different noise"
    print("edit_pages_verified scores", r.scores.cpu().numpy().round(4).tolist(), "choice", choice.tolist())
    # min_score above every score: every box keeps the original pixels
    none = _verified(s, o, min_score=0.0)
    assert none.choice.tolist() == [-1] * N and all(torch.equal(a, b) for a, b in zip(none.image, s["imgs"]))


def test_one_candidate_is_edit_pages_bit_for_bit(cuda, setup, ocr_setup):
    ref_out, ref_vae, _ = setup["run"]
    one = _verified(setup, ocr_setup, candidates=1)
    assert torch.equal(one.image_vae[:, 0], ref_vae) and all(torch.equal(a, b) for a, b in zip(one.image, ref_out))
    assert one.choice.tolist() == [0] * N and one.scores.shape == (N, 1)
    pages = _verified(setup, ocr_setup, candidates=1, return_intermediate=False)
    assert isinstance(pages, list) and all(torch.equal(a, b) for a, b in zip(pages, ref_out))


def test_mismatched_lists_raise_before_any_launch(cuda, setup, ocr_setup):
    """None stands in for the models: a call that got as far as a launch would fail with another error"""
    import diffute_amd as D
    s, o = setup, ocr_setup

    def both(exc, images=s["imgs"], locations=BOXES, ctx=s["ctx"], labels=o["labels"], **kw):
        kw = dict(dict(origins=ORIGINS, crop_scales=CROPS, size=S), **kw)
        with pytest.raises(exc):
            D.edit_pages(None, None, None, images, locations, ctx, STEPS, **kw)
        with pytest.raises(exc):
            D.edit_pages_verified(None, None, None, o["ocr"], o["proc"], images, locations, ctx, labels, STEPS, candidates=K, **kw)
    both(ValueError, images=s["imgs"][:2])
    both(ValueError, locations=BOXES[:2])
    both(ValueError, origins=ORIGINS[:2])
    both(ValueError, crop_scales=CROPS + [[128]])
    both(ValueError, origins=[ORIGINS[0][:1], ORIGINS[1], ORIGINS[2]])
    both(ValueError, crop_scales=[CROPS[0], CROPS[1] + [96], CROPS[2]])
    both(ValueError, ctx=s["ctx"][:3])
    both(ValueError, batch_size=0)
    both(ValueError, locations=[BOXES[0], [], BOXES[2]], origins=[ORIGINS[0], [], ORIGINS[2]], crop_scales=[CROPS[0], [], CROPS[2]], ctx=s["ctx"][:3],
         labels=o["labels"][:3])
    with pytest.raises(ValueError):
        _verified(s, o, candidates=2, seeds=[0])
    with pytest.raises(ValueError):
        D.edit_pages_verified(None, None, None, o["ocr"], o["proc"], s["imgs"], BOXES, s["ctx"], o["labels"][:3], STEPS, origins=ORIGINS, crop_scales=CROPS,
                              size=S)
    with pytest.raises(ValueError, match="page 2"):                         # a box outside ITS page (150 wide), inside the other two
        D.edit_pages_verified(None, None, None, o["ocr"], o["proc"], s["imgs"], [BOXES[0], BOXES[1], [(20, 300, 160, 320)]], s["ctx"], o["labels"], STEPS,
                              origins=ORIGINS, crop_scales=CROPS, size=S)
