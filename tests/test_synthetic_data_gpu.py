"""The synthetic document dataset on the GPU (diffute_amd/data.py over csrc/page_compose.hip), from tests/golden's atlas alone: the
boxes of `document` cover all ink (metrics.outside_diff_pages against the same pages without lines is 0) and every box holds ink;
training_batch is prepost.preprocess_pages + glyph_contexts bit for bit, with the shapes and dtypes train_step documents; one train_step
of the tiny models on a batch of the dataset gives a finite loss and a finite gradient norm."""
import numpy as np
import pytest
import torch

import page_compose_cases as C
import page_compose_restatement as T

pytestmark = pytest.mark.gpu

TINY_UNET = dict(block_out_channels=(64, 128, 256, 256), attention_head_dim=(1, 2, 4, 4), cross_attention_dim=128)      # test_models_gpu.py's
TINY_VAE = dict(block_out_channels=(64, 128, 128, 128), layers_per_block=1)


@pytest.fixture(scope="module")
def world(cuda):
    """four small ragged pages, composed once with their lines and once without; read-only"""
    import diffute_amd as D
    atlas = D.GlyphAtlas.from_arrays(C.load_atlas_arrays(), "atlas.")
    renderer = D.GlyphRenderer(atlas, cuda)
    ds = D.SyntheticDocuments(renderer, page_size=lambda rng: (int(rng.integers(280, 420)), int(rng.integers(300, 520))), lines=(2, 6), seed=11)
    records = [ds[i] for i in range(4)]
    pages = ds.compose(records)
    blank = ds.compose([dict(r, lines=[]) for r in records])
    enc = D.TrOCREncoder(device=cuda, image_size=32, patch_size=16, hidden_size=TINY_UNET["cross_attention_dim"], num_hidden_layers=1,
                         num_attention_heads=TINY_UNET["cross_attention_dim"] // 64, intermediate_size=256)
    D.synchronize()
    return dict(atlas=atlas, ds=ds, records=records, pages=pages, blank=blank, glyph=(renderer, D.TrOCRProcessor(size=32), enc))


def _boxes(record):
    """the document's boxes with an exclusive upper corner, as diffute_amd.metrics takes them"""
    return [(min(p[0] for p in d["box"]), min(p[1] for p in d["box"]), max(p[0] for p in d["box"]) + 1, max(p[1] for p in d["box"]) + 1)
            for d in record["document"]]


def test_the_document_boxes_cover_all_ink_and_every_box_holds_ink(cuda, world):
    import diffute_amd as D
    from diffute_amd import metrics
    w = world
    boxes = [_boxes(r) for r in w["records"]]
    out = metrics.outside_diff_pages(w["blank"], w["pages"], boxes)
    m = metrics.box_metrics_pages(w["blank"], w["pages"], boxes)
    D.synchronize()
    assert out.changed.tolist() == [0] * 4 and out.sse.tolist() == [0] * 4, "ink outside the document's boxes"
    sse = m.sse.sum(1).tolist()
    texts = [d["text"] for r in w["records"] for d in r["document"]]
    assert len(sse) == len(texts) >= 8 and all(s > 0 for s, t in zip(sse, texts) if t), sse
    for r, page, blank in zip(w["records"], w["pages"], w["blank"]):                        # the pages are what the restatement composes
        assert np.array_equal(page.cpu().numpy(), T.compose(w["atlas"], r))
        assert np.array_equal(blank.cpu().numpy(), T.background(r["size"], r["bg"], r["tex_seed"], r["tex_amp"]))


def test_training_batch_is_preprocess_pages_and_glyph_contexts(cuda, world):
    import diffute_amd as D
    from diffute_amd import prepost
    w = world
    locations, origins, texts = D.sample_boxes(w["records"], np.random.default_rng(5))
    batch = D.training_batch(w["pages"], locations, origins, texts, w["glyph"])
    pre = prepost.preprocess_pages(w["pages"], locations, origins, [[256]] * 4, 512)
    ctx = D.glyph_contexts(texts, *w["glyph"])
    D.synchronize()
    assert set(batch) == {"pixel_values", "masked_images", "masks", "ocr_embeddings"}
    for k, want, shape, dtype in (("pixel_values", pre["image"], (4, 3, 512, 512), torch.float32),
                                  ("masked_images", pre["masked_image"], (4, 3, 512, 512), torch.float32),
                                  ("masks", pre["mask"], (4, 1, 512, 512), torch.uint8),
                                  ("ocr_embeddings", ctx, (4, 5, 128), w["glyph"][2].dtype)):
        assert batch[k].is_cuda and tuple(batch[k].shape) == shape and batch[k].dtype == dtype, k
        assert torch.equal(batch[k], want), k
    assert torch.isfinite(batch["ocr_embeddings"].float()).all()
    pv, mi, mk = batch["pixel_values"], batch["masked_images"], batch["masks"]
    assert float(pv.min()) >= -1.0 and float(pv.max()) <= 1.0 and int(mk.min()) == 0 and int(mk.max()) == 1
    assert all(not torch.equal(pv[b], mi[b]) for b in range(4))                             # every row has a box inside its crop
    # the iterator is compose + sample_boxes + training_batch on the same streams
    w["ds"].glyph = w["glyph"]
    first = next(w["ds"].batches(4, np.random.default_rng(5)))
    D.synchronize()
    assert all(torch.equal(first[k], batch[k]) for k in batch)
    small = next(w["ds"].batches(2, np.random.default_rng(5), size=128, start=2))
    assert tuple(small["pixel_values"].shape) == (2, 3, 128, 128) and tuple(small["masks"].shape) == (2, 1, 128, 128)


def test_one_train_step_on_a_synthetic_batch(cuda, world):
    import diffute_amd as D
    from diffute_amd.training import train_step
    w = world
    unet = D.UNet2DConditionModel(**TINY_UNET).cuda()
    vae = D.AutoencoderKL(**TINY_VAE).cuda().requires_grad_(False)
    opt = D.FusedAdamW(unet, lr=1e-4, weight_decay=1e-2, max_grad_norm=1.0)
    batch = next(w["ds"].batches(2, np.random.default_rng(9), glyph=w["glyph"], size=128))
    out = train_step(unet, vae, D.DDPMScheduler(), opt, batch, generator=torch.Generator(device=cuda).manual_seed(3))
    D.synchronize()
    assert torch.isfinite(out["loss"]) and float(out["loss"]) > 0 and torch.isfinite(out["grad_norm"]) and float(out["grad_norm"]) > 0
