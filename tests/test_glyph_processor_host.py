"""TrOCRProcessor (diffute_amd/processing.py) on the host: the numpy restatement of Pillow's 8-bit resample and transformers' float
arithmetic (tests/pil_resample_restatement.py) against what Pillow and transformers themselves produced
(tests/golden/glyph_processor.npz, scripts/make_glyph_golden.py) and, where Pillow is importable, against Pillow live; the product's
coefficient tables and normalisation table against the restatement and the golden; config persistence and the refusals.  Everything
is compared bit for bit."""
import json
import os

import numpy as np
import pytest
import torch

import glyph_cases as G
import pil_resample_restatement as R


@pytest.fixture(scope="module")
def golden():
    return G.load_golden()


@pytest.mark.parametrize("case", G.CASES, ids=G.CASE_IDS)
def test_restatement_equals_pillow_and_transformers_golden(golden, case):
    name, _, _, out_hw, resample = case
    img = G.case_input(golden, case)
    resized, pv = R.pixel_values(img, out_hw, resample)
    want_u8 = golden[name + ".pil_resized"].transpose(2, 0, 1)
    assert resized.shape == want_u8.shape and np.array_equal(resized, want_u8), "uint8 resize differs from Pillow's"
    want_pv = golden[name + ".pixel_values"]
    assert pv.dtype == np.float32 and np.array_equal(pv.view(np.uint32), want_pv.view(np.uint32)), "pixel_values differ from transformers'"
    if resample == G.BICUBIC:                    # the case is there for the clamp: both ends must be reached
        assert resized.min() == 0 and resized.max() == 255


def test_restatement_equals_pillow_live():
    Image = pytest.importorskip("PIL.Image")
    g = G.load_golden()
    for case in G.CASES:
        name, _, _, out_hw, resample = case
        img = G.case_input(g, case)
        want = np.asarray(Image.fromarray(img).resize((out_hw[1], out_hw[0]), resample=resample))
        assert np.array_equal(R.resize(img, out_hw, resample), want), name
    rng = np.random.RandomState(20240517)
    for i in range(50):                          # 50 seeded size pairs in [1, 900] -> [1, 400], each axis drawn on its own
        h, w = int(rng.randint(1, 901)), int(rng.randint(1, 901))
        oh, ow = int(rng.randint(1, 401)), int(rng.randint(1, 401))
        resample = G.BILINEAR if i % 2 == 0 else G.BICUBIC
        img = rng.randint(0, 256, (h, w, 3), dtype=np.uint8)
        want = np.asarray(Image.fromarray(img).resize((ow, oh), resample=resample))
        assert np.array_equal(R.resize(img, (oh, ow), resample), want), f"{h}x{w} -> {oh}x{ow} filter {resample}"


def test_product_tables_equal_the_restatement():
    """the vectorised float64 table builder that feeds the kernel against the literal one, over up- and down-scales and both filters"""
    from diffute_amd import processing as P
    rng = np.random.RandomState(7)
    pairs = [(60, 384), (200, 384), (560, 384), (1680, 384), (37, 384), (181, 384), (500, 96), (700, 96), (1, 8), (2, 5), (3, 7), (900, 29)]
    pairs += [(int(rng.randint(1, 901)), int(rng.randint(1, 401))) for _ in range(20)]
    for n_in, n_out in pairs:
        if n_in == n_out:
            continue
        for resample in (G.BILINEAR, G.BICUBIC):
            ksize, bounds, kk = R.precompute_coeffs(n_in, n_out, resample)
            t = P.resample_table(n_in, n_out, resample)
            assert P._taps(n_in, n_out, resample) == ksize and t.dtype == np.int32 and t.size == n_out * (2 + ksize)
            assert np.array_equal(t[:2 * n_out].reshape(n_out, 2), np.array(bounds)), (n_in, n_out, resample)
            assert np.array_equal(t[2 * n_out:].reshape(n_out, ksize), np.array(kk)), (n_in, n_out, resample)


@pytest.mark.parametrize("tag", ["half", "imagenet"])
def test_normalisation_table_equals_transformers_exhaustively(golden, tag):
    """all 256 bytes x 3 channels, for trocr-large-printed's mean = std = 0.5 and for the ImageNet statistics.  The order that holds for
    both: float32(float64(x) * rescale_factor), then (v - float32(mean)) / float32(std) in float32 - transformers' own."""
    from diffute_amd import processing as P
    mean, std = golden["table." + tag + ".mean_std"]
    want = golden["table." + tag]
    got = P.normalisation_table(True, 1 / 255, True, list(mean), list(std))
    assert got.shape == (3, 256) and got.dtype == np.float32
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    ramp = np.broadcast_to(np.arange(256, dtype=np.uint8)[None, :, None], (3, 256, 1))
    rest = R.rescale_normalize(ramp, image_mean=list(mean), image_std=list(std))[..., 0]
    assert np.array_equal(rest.view(np.uint32), want.view(np.uint32))


def test_normalisation_table_equals_transformers_live():
    T = pytest.importorskip("transformers")
    from diffute_amd import processing as P
    ramp = np.broadcast_to(np.arange(256, dtype=np.uint8)[None, :, None], (3, 256, 2)).copy()
    for mean, std in (([0.5] * 3, [0.5] * 3), ([0.485, 0.456, 0.406], [0.229, 0.224, 0.225])):
        proc = T.ViTImageProcessorPil(do_resize=False, do_rescale=True, rescale_factor=1 / 255, do_normalize=True, image_mean=mean, image_std=std)
        want = proc(images=ramp, return_tensors="np", input_data_format="channels_first").pixel_values[0][..., 0]
        got = P.normalisation_table(True, 1 / 255, True, mean, std)
        assert np.array_equal(got.view(np.uint32), np.ascontiguousarray(want).view(np.uint32))


def test_public_names_and_defaults():
    import diffute_amd as D
    assert "TrOCRProcessor" in D.__all__ and "ViTImageProcessor" in D.__all__
    p = D.TrOCRProcessor()
    ip = p.image_processor
    assert isinstance(ip, D.ViTImageProcessor)
    assert ip.size == {"height": 384, "width": 384} and ip.resample == 2 and ip.do_resize and ip.do_rescale and ip.do_normalize
    assert ip.rescale_factor == 1 / 255 and ip.image_mean == [0.5, 0.5, 0.5] and ip.image_std == [0.5, 0.5, 0.5]


def test_config_round_trip(tmp_path):
    import diffute_amd as D
    cfg = {"do_resize": True, "size": {"height": 96, "width": 128}, "resample": 3, "do_rescale": True, "rescale_factor": 0.00392156862745098,
           "do_normalize": True, "image_mean": [0.485, 0.456, 0.406], "image_std": [0.229, 0.224, 0.225],
           "image_processor_type": "ViTImageProcessor", "processor_class": "TrOCRProcessor", "some_future_key": {"ignored": 1}}
    src = tmp_path / "a"; src.mkdir()
    (src / "preprocessor_config.json").write_text(json.dumps(cfg))
    p = D.TrOCRProcessor.from_pretrained(str(src))
    ip = p.image_processor
    assert ip.size == {"height": 96, "width": 128} and ip.resample == 3 and ip.image_mean == cfg["image_mean"] and ip.image_std == cfg["image_std"]
    assert ip.rescale_factor == cfg["rescale_factor"]
    dst = tmp_path / "b"
    p.save_pretrained(str(dst))
    saved = json.loads((dst / "preprocessor_config.json").read_text())
    for k in ("do_resize", "size", "resample", "do_rescale", "rescale_factor", "do_normalize", "image_mean", "image_std"):
        assert saved[k] == cfg[k], k
    again = D.ViTImageProcessor.from_pretrained(str(dst))
    assert again.to_dict() == ip.to_dict()
    # `size` as an int
    (src / "preprocessor_config.json").write_text(json.dumps(dict(cfg, size=224, resample=2)))
    assert D.ViTImageProcessor.from_pretrained(str(src)).size == {"height": 224, "width": 224}
    # any other resample is refused
    for bad in (0, 1, 4, 5):
        (src / "preprocessor_config.json").write_text(json.dumps(dict(cfg, resample=bad)))
        with pytest.raises(NotImplementedError):
            D.TrOCRProcessor.from_pretrained(str(src))


def test_refusals_before_any_gpu_work():
    """every refusal here is raised while the inputs are inspected, before the library or the device is touched"""
    import diffute_amd as D
    p = D.TrOCRProcessor()
    with pytest.raises(TypeError):
        p(images=np.zeros((60, 200, 3), dtype=np.float32))
    with pytest.raises(TypeError):
        p(images=torch.zeros(3, 60, 200, dtype=torch.float32))
    with pytest.raises(TypeError):
        p(images="glyph.png")
    with pytest.raises(ValueError):
        p(images=np.zeros((3, 200, 3), dtype=np.uint8))              # channels first or last? not guessed
    with pytest.raises(ValueError):
        p(images=np.zeros((60, 200), dtype=np.uint8))
    with pytest.raises(ValueError):
        p(images=np.zeros((60, 200, 4), dtype=np.uint8))
    with pytest.raises(ValueError):
        p(images=[])
    with pytest.raises(NotImplementedError, match="tokenizer"):
        p.batch_decode([[0, 1, 2]])
    with pytest.raises(NotImplementedError):
        D.ViTImageProcessor(resample=1)
