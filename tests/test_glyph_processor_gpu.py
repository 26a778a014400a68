"""TrOCRProcessor on the GPU (csrc/prepost.hip dmx_glyph_resize_normalize through diffute_amd/processing.py): bit for bit against what
Pillow and transformers produced (tests/golden/glyph_processor.npz) and against the numpy restatement of the published algorithm
(tests/pil_resample_restatement.py), for the uint8 resize and the fp32 pixel_values, over every input form the scripts use."""
import numpy as np
import pytest
import torch

import glyph_cases as G
import pil_resample_restatement as R

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def golden():
    return G.load_golden()


def _proc(case, **kw):
    import diffute_amd as D
    _, _, _, out_hw, resample = case
    return D.TrOCRProcessor(size={"height": out_hw[0], "width": out_hw[1]}, resample=resample, **kw)


def _bits(t):
    return t.cpu().numpy().view(np.uint32)


@pytest.mark.parametrize("case", G.CASES, ids=G.CASE_IDS)
def test_processor_equals_golden_and_restatement(cuda, golden, case):
    import diffute_amd as D
    name, _, _, out_hw, resample = case
    img = G.case_input(golden, case)
    got = _proc(case)(images=img, return_tensors="pt", return_resized=True)
    D.synchronize()
    pv, res = got.pixel_values, got["resized"]
    assert pv is got["pixel_values"] and pv.is_cuda and pv.dtype == torch.float32 and tuple(pv.shape) == (1, 3) + out_hw
    want_u8 = golden[name + ".pil_resized"].transpose(2, 0, 1)
    assert np.array_equal(res[0].cpu().numpy(), want_u8), "uint8 resize differs from Pillow's"
    assert np.array_equal(_bits(pv[0]), golden[name + ".pixel_values"].view(np.uint32)), "pixel_values differ from transformers'"
    r_u8, r_pv = R.pixel_values(img, out_hw, resample)
    assert np.array_equal(res[0].cpu().numpy(), r_u8) and np.array_equal(_bits(pv[0]), r_pv.view(np.uint32)), "differs from the restatement"


def test_default_processor_is_trocr_large_printed(cuda, golden):
    """`D.TrOCRProcessor()` with no arguments: 384, bilinear, 1/255, 0.5 / 0.5"""
    import diffute_amd as D
    case = G.CASES[0]
    pv = D.TrOCRProcessor()(images=G.case_input(golden, case), return_tensors="pt").pixel_values
    assert np.array_equal(_bits(pv[0]), golden[case[0] + ".pixel_values"].view(np.uint32))


def test_mixed_batch_equals_per_image_calls(cuda, golden):
    """every bilinear 384-target case in ONE call (ragged sizes, one skipped-pass image) against the golden and against one call each"""
    import diffute_amd as D
    cases = [c for c in G.CASES if c[0] in G.MIXED_BATCH]
    assert len(cases) == 5
    imgs = [G.case_input(golden, c) for c in cases]
    p = D.TrOCRProcessor()
    got = p(images=imgs, return_tensors="pt", return_resized=True)
    assert tuple(got.pixel_values.shape) == (len(cases), 3, 384, 384)
    for i, c in enumerate(cases):
        assert np.array_equal(_bits(got.pixel_values[i]), golden[c[0] + ".pixel_values"].view(np.uint32)), c[0]
        assert np.array_equal(got["resized"][i].cpu().numpy(), golden[c[0] + ".pil_resized"].transpose(2, 0, 1)), c[0]
        one = p(images=imgs[i], return_tensors="pt").pixel_values
        assert torch.equal(one[0], got.pixel_values[i]), c[0]


@pytest.mark.parametrize("name", ["glyph_len12", "noise_500x700_bicubic"])
def test_identical_across_input_forms(cuda, golden, name):
    case = G.CASES[G.CASE_IDS.index(name)]
    img = G.case_input(golden, case)
    p = _proc(case)
    want = golden[name + ".pixel_values"].view(np.uint32)
    chw = torch.from_numpy(img).permute(2, 0, 1).contiguous()                 # what ToTensorV2 hands the training script
    forms = {
        "hwc_numpy": img,
        "chw_numpy": np.ascontiguousarray(img.transpose(2, 0, 1)),
        "chw_torch": chw,
        "hwc_torch": torch.from_numpy(img),
        "chw_torch_view": torch.from_numpy(img).permute(2, 0, 1),           # CHW shape over HWC memory
        "hwc_cuda": torch.from_numpy(img).to(cuda),
        "chw_cuda": chw.to(cuda),
    }
    for form, x in forms.items():
        pv = p(images=x, return_tensors="pt").pixel_values
        assert np.array_equal(_bits(pv[0]), want), form
    both = p(images=[forms["hwc_cuda"], img, forms["chw_cuda"], chw], return_tensors="pt").pixel_values      # GPU and host images in one call
    for i in range(4):
        assert np.array_equal(_bits(both[i]), want), f"mixed host / GPU batch, image {i}"


def test_pil_input(cuda, golden):
    Image = pytest.importorskip("PIL.Image")
    case = G.CASES[0]
    img = G.case_input(golden, case)
    pv = _proc(case)(images=[Image.fromarray(img)], return_tensors="pt").pixel_values
    assert np.array_equal(_bits(pv[0]), golden[case[0] + ".pixel_values"].view(np.uint32))
    with pytest.raises(ValueError):
        _proc(case)(images=Image.fromarray(img).convert("L"))


def test_strided_cuda_view_equals_its_contiguous_copy(cuda):
    import diffute_amd as D
    rng = np.random.RandomState(3)
    big = torch.from_numpy(rng.randint(0, 256, (300, 400, 3), dtype=np.uint8)).to(cuda)
    p = D.TrOCRProcessor()
    views = [big[100:160, 50:330], big[:, 7:8], big[10:290:3, 20:399:2],
             big.permute(2, 0, 1)[:, 17:77, 100:300]]
    for v in views:
        assert not v.is_contiguous()
        a = p(images=v, return_tensors="pt").pixel_values
        b = p(images=v.contiguous(), return_tensors="pt").pixel_values
        hwc = v if v.shape[-1] == 3 else v.permute(1, 2, 0)
        _, want = R.pixel_values(hwc.cpu().numpy(), (384, 384), G.BILINEAR)
        assert torch.equal(a, b) and np.array_equal(_bits(a[0]), want.view(np.uint32)), tuple(v.shape)


def test_writes_every_element_and_nothing_else(cuda, golden):
    """pixel_values written into the middle of a sentinel-filled buffer: the guard bands survive, no sentinel is left inside"""
    import diffute_amd as D
    cases = [c for c in G.CASES if c[0] in G.MIXED_BATCH]
    imgs = [G.case_input(golden, c) for c in cases]
    n, guard = len(cases) * 3 * 384 * 384, 4096
    sentinel = torch.tensor([0x7FC0DEAD], dtype=torch.int32)                   # a NaN no normalisation table holds
    buf = sentinel.to(cuda).repeat(n + 2 * guard)
    out = buf.view(torch.float32)[guard:guard + n].view(len(cases), 3, 384, 384)
    got = D.TrOCRProcessor()(images=imgs, return_tensors="pt", out=out)
    D.synchronize()
    assert got.pixel_values.data_ptr() == out.data_ptr()
    assert bool((buf[:guard] == 0x7FC0DEAD).all()) and bool((buf[guard + n:] == 0x7FC0DEAD).all()), "guard band overwritten"
    assert not bool((buf[guard:guard + n] == 0x7FC0DEAD).any()), "an element was left unwritten"
    for i, c in enumerate(cases):
        assert np.array_equal(_bits(out[i]), golden[c[0] + ".pixel_values"].view(np.uint32)), c[0]


def test_postprocess_box_view_feeds_the_encoder_on_the_device(cuda):
    """the read-back chain: prepost.postprocess -> the text box as a strided view of its result -> processor -> TrOCREncoder (tiny ViT), pixels
    never leaving the GPU, against the same encoder fed the restatement's pixel_values of the host copy of that box"""
    import diffute_amd as D
    rng = np.random.RandomState(11)
    img = torch.from_numpy(rng.randint(0, 256, (300, 400, 3), dtype=np.uint8)).to(cuda)
    box, x_s, y_s, crop = [150, 120, 262, 150], 90, 40, 256
    vae = (torch.randn(1, 3, 512, 512, generator=torch.Generator().manual_seed(5)) * 0.6).clamp(-1.3, 1.3).to(cuda)
    out = D.prepost.postprocess(vae, img, box, x_s, y_s, crop)
    view = out[box[1]:box[3], box[0]:box[2]]
    assert view.is_cuda and not view.is_contiguous()
    proc = D.TrOCRProcessor(size=64)
    pv = proc(images=view, return_tensors="pt").pixel_values
    enc = D.TrOCREncoder(device=cuda, image_size=64, patch_size=16, num_channels=3, hidden_size=256, num_hidden_layers=2,
                         num_attention_heads=4, intermediate_size=512, qkv_bias=True)
    got = enc(pv).last_hidden_state
    _, want_pv = R.pixel_values(view.cpu().numpy(), (64, 64), G.BILINEAR)
    assert np.array_equal(_bits(pv[0]), want_pv.view(np.uint32))
    want = enc(torch.from_numpy(want_pv)[None].to(cuda)).last_hidden_state
    D.synchronize()
    assert torch.isfinite(got).all() and torch.equal(got, want)


def test_over_cap_downscale_is_refused_and_the_device_stays_usable(cuda, golden):
    import diffute_amd as D
    from diffute_amd import _cabi
    lib = _cabi.lib()
    cap = lib.dmx_glyph_max_taps()
    assert cap == 64
    small = D.TrOCRProcessor(size=8)
    with pytest.raises(ValueError, match="cap of 64"):
        small(images=np.zeros((600, 40, 3), dtype=np.uint8))                  # 600 -> 8 bilinear: 151 taps
    with pytest.raises(ValueError, match="cap of 64"):
        D.TrOCRProcessor(size=8, resample=3)(images=torch.zeros(3, 40, 260, dtype=torch.uint8, device=cuda))     # 260 -> 8 bicubic: 131 taps
    small(images=np.zeros((248, 40, 3), dtype=np.uint8))                      # 248 -> 8 bilinear: 63 taps, inside the cap
    # the C-ABI entry refuses on its own, before it launches anything
    dummy = torch.zeros(4096, dtype=torch.uint8, device=cuda)
    o = torch.zeros(1, 3, 8, 8, dtype=torch.float32, device=cuda)
    rc = lib.dmx_glyph_resize_normalize(_cabi.ptr(dummy), 1, _cabi.ptr(dummy), _cabi.ptr(dummy), cap + 1, 8, 8, _cabi.ptr(o), None, _cabi.current_stream())
    assert rc != 0
    with pytest.raises(RuntimeError, match="exceed the cap of 64"):
        _cabi.check(rc, "glyph_resize_normalize", lib)
    D.synchronize()
    assert float(o.abs().sum()) == 0.0
    case = G.CASES[0]
    pv = D.TrOCRProcessor()(images=G.case_input(golden, case)).pixel_values
    D.synchronize()
    assert np.array_equal(_bits(pv[0]), golden[case[0] + ".pixel_values"].view(np.uint32))
