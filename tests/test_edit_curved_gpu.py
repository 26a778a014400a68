"""pipeline.edit_curved on the tiny models of tests/test_edit_quads_gpu.py: S = 128, two pages with 2 + 1 curved regions (an arc in six
cells, an S-bend, a line read top to bottom), batch_size = 2 - the first chunk spans both pages, the last has one row.  The result equals
the manual chain plan_curved -> preprocess_curved -> the chunks of edit_pages -> postprocess_curved, bit for bit; blend= raises."""
import numpy as np
import pytest
import torch

import curved_cases as CC
import curved_restatement as CR
from test_models_gpu import TINY_UNET, TINY_VAE

pytestmark = pytest.mark.gpu

S, STEPS, BS = 128, 2, 2
PAGES = [(320, 384), (384, 200)]                                  # h x w
POLYGONS = [[CC.arc(190, 330, 200, 236, 240, 300, 7), [(60, 240), (120, 230), (180, 246), (240, 236), (242, 262), (180, 272), (120, 256), (62, 266)]],
            [[(120, 60), (124, 130), (120, 200), (92, 200), (96, 130), (92, 60)]]]       # the last one is read top to bottom
N = 3


@pytest.fixture(scope="module")
def setup(cuda):
    """models, inputs and one edit_curved run - computed once, only read by the tests"""
    import diffute_amd as D
    from diffute_amd.init import normal
    unet = D.UNet2DConditionModel(**TINY_UNET).cuda().requires_grad_(False)
    vae = D.AutoencoderKL(**TINY_VAE).cuda().requires_grad_(False)
    rs = np.random.RandomState(13)
    imgs = [torch.from_numpy(rs.randint(0, 256, (h, w, 3), dtype=np.uint8)).to(cuda) for h, w in PAGES]
    ctx = normal(2, 13, N * 77 * 128, cuda).reshape(N, 77, 128)
    enc_noise = normal(4, 71, N * 4 * 16 * 16, cuda).reshape(N, 4, 16, 16)
    s = dict(unet=unet, vae=vae, imgs=imgs, ctx=ctx, enc_noise=enc_noise)
    s["run"] = D.edit_curved(unet, vae, D.DDIMScheduler(), imgs, POLYGONS, ctx, STEPS, batch_size=BS, enc_noise=enc_noise, return_intermediate=True,
                             size=S)                             # frames planned
    D.synchronize()
    return s


def test_edit_curved_is_the_manual_chain(cuda, setup):
    import diffute_amd as D
    s = setup
    out, image_vae, pre = s["run"]
    assert isinstance(out, list) and len(out) == 2 and image_vae.shape == (N, 3, S, S)
    frames = D.prepost.plan_curved(POLYGONS, PAGES, size=S)
    assert all(len(f) == 3 for fs in frames for f in fs)
    want_pre = D.prepost.preprocess_curved(s["imgs"], POLYGONS, frames, size=S)
    assert sorted(pre) == sorted(want_pre) and all(torch.equal(pre[k], want_pre[k]) for k in pre)
    init = torch.randn((1, 4, S // 8, S // 8), generator=torch.manual_seed(0), dtype=torch.float32).to(cuda)
    chunks = []
    for lo in range(0, N, BS):
        hi = min(N, lo + BS)
        chunks.append(D.edit_latents(s["unet"], s["vae"], D.DDIMScheduler(), want_pre["image"][lo:hi], want_pre["masked_image"][lo:hi],
                                     want_pre["mask"][lo:hi], s["ctx"][lo:hi], STEPS, init_latents=init.expand(hi - lo, -1, -1, -1).contiguous(),
                                     enc_noise=s["enc_noise"][lo:hi]).clone())
    want_vae = torch.cat(chunks, 0)
    assert torch.equal(image_vae, want_vae), "image_vae differs from edit_latents over the chunks"
    want = D.prepost.postprocess_curved(want_vae, s["imgs"], POLYGONS, frames)
    D.synchronize()
    for p, (h, w) in enumerate(PAGES):
        assert out[p].shape == (h, w, 3) and out[p].dtype == torch.uint8 and torch.equal(out[p], want[p]), f"page {p}"
        Y, X = np.mgrid[0:h, 0:w]
        covered = np.zeros((h, w), bool)
        for c in POLYGONS[p]:
            covered |= CR.inside(dict(cells=CR.cell_dicts(c)), X, Y)
        covered = torch.from_numpy(covered).to(cuda)
        assert torch.equal(out[p][~covered], s["imgs"][p][~covered]), "pixels outside all polygons must be untouched"
        assert (out[p][covered] != s["imgs"][p][covered]).any() and 1000 < int(covered.sum()) < h * w // 5
    given = D.edit_curved(s["unet"], s["vae"], D.DDIMScheduler(), s["imgs"], POLYGONS, s["ctx"], STEPS, frames=frames, batch_size=BS,
                          enc_noise=s["enc_noise"], size=S)
    D.synchronize()
    assert isinstance(given, list) and all(torch.equal(a, b) for a, b in zip(given, out))


def test_blend_raises(cuda, setup):
    """there is no blend for curved regions: anything but None raises before any launch (None stands in for the models)"""
    import diffute_amd as D
    s = setup
    for blend in (D.prepost.QuadBlend(feather=2), D.prepost.PasteBlend(feather=2), 1):
        with pytest.raises(NotImplementedError, match="blend"):
            D.edit_curved(None, None, None, s["imgs"], POLYGONS, s["ctx"], STEPS, blend=blend, size=S)
        with pytest.raises(NotImplementedError, match="blend"):
            D.prepost.postprocess_curved(s["run"][1], s["imgs"], POLYGONS, None, blend=blend)
    assert "edit_curved" in D.__all__


def test_mismatched_lists_raise_before_any_launch(cuda, setup):
    import diffute_amd as D
    s = setup
    with pytest.raises(ValueError, match="lengths must agree"):
        D.edit_curved(None, None, None, s["imgs"], POLYGONS[:1], s["ctx"], STEPS, size=S)
    with pytest.raises(ValueError, match="lengths must agree"):
        D.edit_curved(None, None, None, s["imgs"], POLYGONS, s["ctx"], STEPS, frames=[[(10, 10, 64)], [(10, 10, 64)]], size=S)
    with pytest.raises(ValueError, match="batch_size"):
        D.edit_curved(None, None, None, s["imgs"], POLYGONS, s["ctx"], STEPS, batch_size=0, size=S)
