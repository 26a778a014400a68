"""Test-local restatement of the OCR read-back of an edited text box and of the best-of-K selection rule
(tests/test_readback_host.py, tests/test_readback_gpu.py, tests/test_select_paste_gpu.py, tests/test_edit_verified_gpu.py).

The read-back is the reference's chain written out in numpy: paste ONE decoder output over the original page
(oracle.prepost.postprocess, app.ipynb:825-846), slice the box `[y1:y2, x1:x2]` (app.ipynb:842-846) and run the processor on the slice
(tests/pil_resample_restatement.py: Pillow's 8-bit resample, then transformers' rescale / normalise).  The cases below are shared by the
host test, which pins the chain's resize against Pillow's own Image.resize, and by the GPU test of the fused kernel."""
import ctypes

import numpy as np

import pil_resample_restatement as R

BILINEAR, BICUBIC = R.BILINEAR, R.BICUBIC
H, W, S, K = 320, 384, 128, 3

# (box (x1, y1, x2, y2), crop origin (x_s, y_s), crop side) on the 384 x 320 page at S = 128
ITEMS = {
    "identity": ((40, 60, 150, 78), (30, 20), 128),                 # crop = S; the box is 110 wide: 9 bilinear taps into 32
    "downscale": ((200, 150, 330, 180), (150, 90), 200),            # the decoder output is enlarged to the crop
    "upscale": ((60, 250, 140, 266), (50, 210), 96),                # ... and shrunk to it
    "clipped": ((310, 260, 370, 280), (300, 250), 128),             # the crop is cut to 84 x 70 by the image border
    "exact2x": ((105, 110, 137, 120), (100, 100), 64),              # S == 2 * crop: the 2x2-mean path; box width 32 = output width: no horizontal pass
    "wider_than_crop": ((190, 50, 290, 66), (200, 40), 64),         # the crop covers x 200 .. 263 only: original pixels enter on both sides
    "one_pixel_high": ((20, 200, 90, 201), (10, 150), 128),
    "height_is_output": ((30, 100, 80, 132), (0, 60), 128),         # box height 32 = output height: no vertical pass
}
SET_A = ["identity", "downscale", "upscale", "clipped"]
SET_B = ["exact2x", "wider_than_crop", "one_pixel_high", "height_is_output"]
# (id, items, resample, output size)
CASES = [("a_bilinear_32", SET_A, BILINEAR, 32), ("a_bicubic_32", SET_A, BICUBIC, 32), ("b_bilinear_32", SET_B, BILINEAR, 32),
         ("b_bicubic_32", SET_B, BICUBIC, 32), ("a_bilinear_384", SET_A, BILINEAR, 384)]
CASE_IDS = [c[0] for c in CASES]


def page():
    return np.random.RandomState(11).randint(0, 256, (H, W, 3), dtype=np.uint8)


def decoder_outputs(names):
    """fp32 [B][K][3][S][S] in [-1.2, 1.2]: beyond [-1, 1] the paste's clamp to a byte is exercised"""
    rng = np.random.RandomState(sum(map(ord, "".join(names))))
    return (rng.rand(len(names), K, 3, S, S) * 2.4 - 1.2).astype(np.float32)


def box_slice(image_vae, instance_image, item):
    """the slice the reference reads back: one paste over the ORIGINAL page, then [y1:y2, x1:x2] -> uint8 [bh][bw][3]"""
    from oracle import prepost as OP
    box, (x_s, y_s), crop = item
    x1, y1, x2, y2 = box
    return OP.postprocess(image_vae, instance_image, box, x_s, y_s, crop)[y1:y2, x1:x2]


def readback(image_vae, instance_image, item, size, resample):
    """-> (resized uint8 [3][size][size], pixel_values fp32 [3][size][size]) of one candidate of one box"""
    return R.pixel_values(np.ascontiguousarray(box_slice(image_vae, instance_image, item)), (size, size), resample)


def select(scores, threshold=-np.inf):
    """the selection rule, one box at a time: arg-max, the lowest k on a tie; a NaN never wins; 0 if every score is NaN; -1 if the best
    score is below the threshold"""
    out = []
    for row in np.asarray(scores, dtype=np.float32):
        best = -1
        for k, v in enumerate(row):
            if np.isnan(v):
                continue
            if best < 0 or v > row[best]:
                best = k
        out.append(0 if best < 0 else (-1 if row[best] < np.float32(threshold) else best))
    return np.array(out, dtype=np.int32)


def entry_tables(items, size, resample, h=H, w=W, s=S):
    """the host half of one dmx_readback_pixel_values call, built from the product's table builder: (prepared item table, pass table,
    int32 tables, float32 norm, max_taps)"""
    from diffute_amd import _cabi, prepost, processing
    ip = processing.ViTImageProcessor(size=size, resample=resample)
    arr = (_cabi.EditItem * len(items))()
    for it, (box, (x_s, y_s), crop) in zip(arr, items):
        it.x1, it.y1, it.x2, it.y2 = box
        it.x_s, it.y_s, it.crop_scale = x_s, y_s, crop
    _cabi.check(_cabi.lib().dmx_edit_items_prepare(arr, len(items), h, w, s), "prepare")
    passes, tables, max_taps = prepost._readback_tables([i[0] for i in items], ip, _cabi.lib().dmx_glyph_max_taps())
    pa = (_cabi.ReadbackPass * len(items))()
    ctypes.memmove(pa, np.ascontiguousarray(passes).ctypes.data, passes.nbytes)
    return arr, pa, tables, ip._norm, max_taps
