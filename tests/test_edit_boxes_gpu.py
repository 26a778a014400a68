"""pipeline.edit_boxes - several text boxes of one image as one batch - against a per-box loop over the existing single-box chain
preprocess -> edit_latents(init_latents = the seed-0 draw) -> postprocess with the same injected noise.  Tiny UNet / VAE (the configs
of tests/test_models_gpu.py), a 320 x 384 image, three boxes, batch_size=2 so that the last chunk has one row, 3 DDIM steps.  The
batch runs the same arithmetic as the loop under another tile plan (B = 2 / 3 instead of 1): the bound is test_models_gpu's E2E_EMU."""
import numpy as np
import pytest
import torch

from test_models_gpu import E2E_EMU, TINY_UNET, TINY_VAE
from util import assert_close

pytestmark = pytest.mark.gpu

H, W, S, STEPS = 320, 384, 128, 3
BOXES = [(40, 60, 150, 78), (200, 150, 330, 180), (60, 250, 140, 266)]
ORIGINS = [(30, 20), (150, 90), (50, 210)]
CROPS = [128, 200, 96]              # identity, downscale and upscale to S = 128


@pytest.fixture(scope="module")
def setup(cuda):
    """models, inputs and the per-box loop's results - computed once, only read by the tests"""
    import diffute_amd as D
    from diffute_amd.init import normal
    unet = D.UNet2DConditionModel(**TINY_UNET).cuda().requires_grad_(False)
    vae = D.AutoencoderKL(**TINY_VAE).cuda().requires_grad_(False)
    img = torch.from_numpy(np.random.RandomState(11).randint(0, 256, (H, W, 3), dtype=np.uint8)).to(cuda)
    ctx = normal(2, 13, 3 * 77 * 128, cuda).reshape(3, 77, 128)
    enc_noise = normal(4, 71, 3 * 4 * 16 * 16, cuda).reshape(3, 4, 16, 16)
    init = torch.randn((1, 4, S // 8, S // 8), generator=torch.manual_seed(0), dtype=torch.float32).to(cuda)      # app.ipynb:796-801
    loop_vae, chained = [], img
    for b in range(3):
        x_s, y_s = ORIGINS[b]
        pre = D.prepost.preprocess(img, BOXES[b], x_s, y_s, CROPS[b], size=S)        # every crop from the ORIGINAL image, as edit_boxes states
        v = D.edit_latents(unet, vae, D.DDIMScheduler(), pre["image"], pre["masked_image"], pre["mask"], ctx[b:b + 1], STEPS,
                           init_latents=init, enc_noise=enc_noise[b:b + 1])
        loop_vae.append(v.clone())
        chained = D.prepost.postprocess(v, chained, BOXES[b], x_s, y_s, CROPS[b])
    D.synchronize()
    return dict(unet=unet, vae=vae, img=img, ctx=ctx, enc_noise=enc_noise, loop_vae=torch.cat(loop_vae, 0).cpu(), chained=chained)


def _run(s, batch_size):
    import diffute_amd as D
    out = D.edit_boxes(s["unet"], s["vae"], D.DDIMScheduler(), s["img"], BOXES, s["ctx"], STEPS, origins=ORIGINS, crop_scales=CROPS,
                       batch_size=batch_size, enc_noise=s["enc_noise"], return_intermediate=True, size=S)
    D.synchronize()
    return out


def test_edit_boxes_matches_the_per_box_loop(cuda, setup):
    import diffute_amd as D
    out, image_vae, pre = _run(setup, 2)
    assert image_vae.shape == (3, 3, S, S) and out.shape == (H, W, 3) and out.dtype == torch.uint8
    e = assert_close(image_vae, setup["loop_vae"], E2E_EMU, "edit_boxes(batch_size=2) image_vae vs the per-box loop")
    for b in range(3):
        eb = assert_close(image_vae[b], setup["loop_vae"][b], E2E_EMU, f"box {b}")
        print(f"edit_boxes box {b}: rel-L2 {eb:.2e} vs the single-box chain")
    print(f"edit_boxes batch_size=2: image_vae rel-L2 {e:.2e} vs the per-box loop")
    # the returned image is the batched paste of the returned decoder outputs, bit for bit
    assert torch.equal(out, D.prepost.postprocess_batch(image_vae, setup["img"], BOXES, ORIGINS, CROPS))
    # ... and the preprocess dict is the batched preprocess of the original image
    again = D.prepost.preprocess_batch(setup["img"], BOXES, ORIGINS, CROPS, size=S)
    assert sorted(pre) == sorted(again) and all(torch.equal(pre[k], again[k]) for k in pre)
    # pixels outside all boxes equal the original, bit for bit; inside, the edit is what the loop's paste gives up to the bound above
    outside = torch.ones(H, W, dtype=torch.bool, device=cuda)
    for x1, y1, x2, y2 in BOXES:
        outside[y1:y2, x1:x2] = False
    assert torch.equal(out[outside], setup["img"][outside])
    assert torch.equal(setup["chained"][outside], setup["img"][outside])
    assert (out[~outside] != setup["img"][~outside]).any()


@pytest.mark.parametrize("batch_size", [3, 1])
def test_edit_boxes_chunking_changes_only_the_tile_plan(cuda, setup, batch_size):
    out, image_vae, _ = _run(setup, batch_size)
    e = assert_close(image_vae, setup["loop_vae"], E2E_EMU, f"edit_boxes(batch_size={batch_size}) image_vae vs the per-box loop")
    print(f"edit_boxes batch_size={batch_size}: image_vae rel-L2 {e:.2e} vs the per-box loop")


def test_edit_boxes_plans_the_crops_itself(cuda, setup):
    """origins / crop_scales left out: the reference's ladder and origin rule, random origins drawn from `rng` in box order"""
    import diffute_amd as D
    boxes = BOXES + [(10, 100, 380, 104)]                 # wider than the short side: its x origin is drawn
    ctx = torch.cat([setup["ctx"], setup["ctx"][:1]], 0)
    plans = D.prepost.plan_edits(boxes, H, W, np.random.RandomState(3))
    # ladder rungs of 128 / 256 / 128 / short side, at S = 128
    out, image_vae, pre = D.edit_boxes(setup["unet"], setup["vae"], D.DDIMScheduler(), setup["img"], boxes, ctx, 1, rng=np.random.RandomState(3),
                                       batch_size=4, return_intermediate=True, size=S)
    want = D.prepost.preprocess_batch(setup["img"], boxes, [p[:2] for p in plans], [p[2] for p in plans], size=S)
    assert all(torch.equal(pre[k], want[k]) for k in want)
    assert torch.equal(out, D.prepost.postprocess_batch(image_vae, setup["img"], boxes, [p[:2] for p in plans], [p[2] for p in plans]))
    with pytest.raises(ValueError):
        D.edit_boxes(setup["unet"], setup["vae"], D.DDIMScheduler(), setup["img"], boxes, setup["ctx"], 1, size=S)      # 4 boxes, 3 contexts
