"""Several text boxes of one image per launch (csrc/prepost_batch.hip through prepost.preprocess_batch / postprocess_batch) against
the numpy restatement of the notebook's host code (oracle/prepost.py) AND against the single-box kernels - bit-exact both ways, on
both builds: it is integer / byte work plus a handful of ordered fp32 operations, and both kernel families compute a pixel through
the same functions (csrc/prepost_resize.h).  One image, one item list that takes every path of tests/test_prepost_gpu.py's cases in
ONE launch."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

H, W = 1100, 1300
# name, box (x1, y1, x2, y2), crop origin, crop_scale
ITEMS = [
    ("up_128", (150, 120, 230, 138), (120, 60), 128),               # 80 x 18 box, upscale x4
    ("identity_512", (300, 300, 520, 380), (200, 150), 512),
    ("down_784", (400, 500, 900, 620), (250, 200), 784),
    ("area_1024", (400, 500, 900, 620), (70, 40), 1024),            # exact 2x downscale -> INTER_AREA path (same box as down_784: overlap)
    ("odd_333", (10, 10, 300, 60), (0, 0), 333),
    ("clipped_bottom_256", (950, 1020, 1100, 1060), (900, 1000), 256),   # crop clipped at the bottom border: 256 x 100, non-square
    ("box_at_corner", (0, 0, 200, 40), (0, 0), 256),
]
# the paste also gets two boxes that overlap each other and one that sticks out of its own crop on both sides
POST_ITEMS = ITEMS + [
    ("overlap_a", (600, 300, 760, 340), (560, 260), 256),
    ("overlap_b", (700, 320, 860, 360), (650, 250), 256),
    ("out_of_crop", (1000, 100, 1250, 140), (1100, 50), 128),
]


def _split(items):
    return [list(i[1]) for i in items], [i[2] for i in items], [i[3] for i in items]


@pytest.fixture(scope="module")
def ref():
    """the image, the decoder outputs and the oracle's results, computed once and only read afterwards (the image stays writable only
    because torch.from_numpy warns about a read-only array)"""
    from oracle import prepost as OP
    img = np.random.RandomState(20240517).randint(0, 256, (H, W, 3), dtype=np.uint8)
    pre = [OP.preprocess(img, list(box), org[0], org[1], crop) for _, box, org, crop in ITEMS]
    g = torch.Generator().manual_seed(5)
    vae = (torch.randn(len(POST_ITEMS), 3, 512, 512, generator=g) * 0.6).clamp(-1.3, 1.3)      # some values leave [-1, 1]: the clamp path
    chain = img
    for b, (_, box, org, crop) in enumerate(POST_ITEMS):
        chain = OP.postprocess(vae[b].numpy(), chain, list(box), org[0], org[1], crop)
    union = np.zeros((H, W), np.uint8)
    for _, box, _, _ in POST_ITEMS:
        union |= OP.generate_mask((W, H), box)
    for a in [chain, union] + [v for p in pre for v in p.values()]:
        a.setflags(write=False)
    return dict(img=img, pre=pre, vae=vae, chain=chain, union=union)


@pytest.fixture(params=["bf16", "fp16"])
def build(request, monkeypatch, cuda):
    """route every prepost call of the test - single-box and batched - through one build of the library"""
    from diffute_amd import _cabi
    real = _cabi.lib
    real(request.param)                                  # loaded (or a clear error) before the patch
    monkeypatch.setattr(_cabi, "lib", lambda elem=None: real(request.param))
    return request.param


def test_preprocess_batch_rows(cuda, build, ref):
    import diffute_amd as D
    img = torch.from_numpy(ref["img"]).to(cuda)
    boxes, origins, crops = _split(ITEMS)
    got = D.prepost.preprocess_batch(img, boxes, origins, crops)
    B = len(ITEMS)
    assert sorted(got) == ["image", "mask", "mask_latent", "masked_image"]
    assert got["image"].shape == (B, 3, 512, 512) and got["masked_image"].shape == (B, 3, 512, 512)
    assert got["mask"].shape == (B, 1, 512, 512) and got["mask"].dtype == torch.uint8 and got["mask_latent"].shape == (B, 1, 64, 64)
    host = {k: v.cpu().numpy() for k, v in got.items()}
    for b, (name, box, org, crop) in enumerate(ITEMS):
        want = ref["pre"][b]
        for k in ("image", "masked_image", "mask", "mask_latent"):
            row = host[k][b] if k in ("image", "masked_image") else host[k][b, 0]
            assert np.array_equal(row, want[k]), f"{name}: {k} of row {b} differs from the host pipeline"
        one = D.prepost.preprocess(img, list(box), org[0], org[1], crop)
        for k in ("image", "masked_image", "mask", "mask_latent"):
            assert torch.equal(got[k][b:b + 1], one[k]), f"{name}: {k} of row {b} differs from the single-box kernel"
    assert set(np.unique(host["mask"])) <= {0, 1} and float(got["image"].abs().max()) <= 1.0
    # each item's mask holds its own box only: down_784's crop contains identity_512's box, and shows nothing of it
    assert host["mask"][2, 0][:100].sum() == 0 and host["mask"][2, 0].sum() > 0


def _post_chain_gpu(D, vae, img, items):
    out = img
    for b, (_, box, org, crop) in enumerate(items):
        out = D.prepost.postprocess(vae[b:b + 1], out, list(box), org[0], org[1], crop)
    return out


def test_postprocess_batch_is_the_chain_of_single_pastes(cuda, build, ref):
    import diffute_amd as D
    img = torch.from_numpy(ref["img"]).to(cuda)
    vae = ref["vae"].to(cuda)
    boxes, origins, crops = _split(POST_ITEMS)
    got, union = D.prepost.postprocess_batch(vae, img, boxes, origins, crops, return_mask=True)
    assert got.shape == (H, W, 3) and got.dtype == torch.uint8 and union.shape == (H, W) and union.dtype == torch.uint8
    assert torch.equal(got, D.prepost.postprocess_batch(vae, img, boxes, origins, crops)), "the union mask must not change the image"
    host = got.cpu().numpy()
    assert np.array_equal(host, ref["chain"]), "differs from oracle.prepost.postprocess chained over the items in order"
    assert torch.equal(got, _post_chain_gpu(D, vae, img, POST_ITEMS)), "differs from the single-box paste chained over the items in order"
    outside = np.ones((H, W), bool)
    for x1, y1, x2, y2 in boxes:
        outside[y1:y2, x1:x2] = False
    assert np.array_equal(host[outside], ref["img"][outside]), "pixels outside every text box must be untouched"
    assert (host[~outside] != ref["img"][~outside]).any()
    assert np.array_equal(union.cpu().numpy(), ref["union"]), "union mask differs from the OR of PIL's rectangles"
    # where the two overlapping boxes meet the later one wins: that patch is overlap_b's resize alone
    alone = D.prepost.postprocess(vae[8:9], img, boxes[8], origins[8][0], origins[8][1], crops[8])
    assert torch.equal(got[320:340, 700:760], alone[320:340, 700:760])


def test_batch_limits(cuda, build, ref):
    import diffute_amd as D
    img = torch.from_numpy(ref["img"]).to(cuda)
    vae10 = ref["vae"].to(cuda)
    # B = 1
    _, box, org, crop = ITEMS[3]
    pre1 = D.prepost.preprocess_batch(img, [box], [org], [crop])
    assert np.array_equal(pre1["image"][0].cpu().numpy(), ref["pre"][3]["image"]) and np.array_equal(pre1["mask"][0, 0].cpu().numpy(), ref["pre"][3]["mask"])
    assert torch.equal(D.prepost.postprocess_batch(vae10[3:4], img, [box], [org], [crop]), D.prepost.postprocess(vae10[3:4], img, list(box), org[0], org[1], crop))
    # B = 64: the list repeated, each repeat with another decoder output so that "the last one wins" is visible among equal boxes
    items = (POST_ITEMS * 7)[:64]
    pick = torch.tensor([(3 * i + 1) % len(POST_ITEMS) for i in range(64)], device=cuda)
    vae = vae10[pick]
    boxes, origins, crops = _split(items)
    pre = D.prepost.preprocess_batch(img, boxes, origins, crops)
    for b in range(64):
        k = b % len(POST_ITEMS)
        if k < len(ITEMS):
            assert np.array_equal(pre["masked_image"][b].cpu().numpy(), ref["pre"][k]["masked_image"]), f"row {b} of 64"
            assert np.array_equal(pre["mask_latent"][b, 0].cpu().numpy(), ref["pre"][k]["mask_latent"]), f"row {b} of 64"
        if b >= len(POST_ITEMS):
            for key in pre:
                assert torch.equal(pre[key][b], pre[key][k]), f"{key}: row {b} of 64 differs from row {k}, the same item"
    got, union = D.prepost.postprocess_batch(vae, img, boxes, origins, crops, return_mask=True)
    assert torch.equal(got, _post_chain_gpu(D, vae, img, items)), "B = 64 differs from 64 chained single pastes"
    assert np.array_equal(union.cpu().numpy(), ref["union"])
    # B = 65
    items = (POST_ITEMS * 7)[:65]
    boxes, origins, crops = _split(items)
    with pytest.raises(ValueError):
        D.prepost.preprocess_batch(img, boxes, origins, crops)
    with pytest.raises(ValueError):
        D.prepost.postprocess_batch(vae10[pick[:1]].expand(65, -1, -1, -1), img, boxes, origins, crops)


def test_bad_item_raises_by_index_and_host_tensors_are_refused(cuda, ref):
    import diffute_amd as D
    img = torch.from_numpy(ref["img"]).to(cuda)
    boxes, origins, crops = _split(ITEMS)
    origins = list(origins); origins[5] = (W, 0)
    with pytest.raises(RuntimeError, match="item 5"):
        D.prepost.preprocess_batch(img, boxes, origins, crops)
    with pytest.raises(TypeError):
        D.prepost.preprocess_batch(torch.from_numpy(ref["img"]), *_split(ITEMS))
    with pytest.raises(TypeError):
        D.prepost.postprocess_batch(ref["vae"][:len(ITEMS)], img, *_split(ITEMS))
