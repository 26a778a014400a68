"""Writes tests/golden/glyph_processor.npz: inputs, Pillow's own uint8 `Image.resize` results and transformers'
`ViTImageProcessor(...)(images, return_tensors="np").pixel_values` for the cases of tests/test_glyph_processor_*.py.

    python scripts/make_glyph_golden.py            # needs Pillow and transformers; the tests only need the file

The cases and their seeded inputs live in tests/glyph_cases.py (glyph-like images - white ground, dark bars on the reference draw_text's
60 x (len(text)+2)*40 canvas - at the 384 output so the file compresses; dense noise only at small output sizes, sparse noise at 384);
the file keeps a CRC32 of each input, not the input."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "golden", "glyph_processor.npz")

sys.path.insert(0, os.path.join(ROOT, "tests"))
from glyph_cases import CASES, crc, make_input  # noqa: E402


def main():
    from PIL import Image
    import PIL
    import transformers
    from transformers import ViTImageProcessorPil
    data = {}
    for name, kind, hw, out_hw, resample in CASES:
        img = make_input(name, kind, hw)
        resized = np.asarray(Image.fromarray(img).resize((out_hw[1], out_hw[0]), resample=resample))
        proc = ViTImageProcessorPil(do_resize=True, size={"height": out_hw[0], "width": out_hw[1]}, resample=resample, do_rescale=True,
                                    rescale_factor=1 / 255, do_normalize=True, image_mean=[0.5, 0.5, 0.5], image_std=[0.5, 0.5, 0.5])
        pv = proc(images=img, return_tensors="np", input_data_format="channels_last").pixel_values[0]
        assert pv.dtype == np.float32 and pv.shape == (3,) + out_hw and resized.shape == out_hw + (3,)
        data[name + ".input_crc"] = np.array(crc(img), dtype=np.int64)
        data[name + ".pil_resized"] = resized
        data[name + ".pixel_values"] = pv
    # the 3 x 256 normalisation table out of transformers itself, for trocr-large-printed's mean = std = 0.5 and for the ImageNet statistics
    ramp = np.broadcast_to(np.arange(256, dtype=np.uint8)[None, :, None], (3, 256, 2)).copy()      # CHW, every byte in every channel
    for tag, mean, std in (("half", [0.5] * 3, [0.5] * 3), ("imagenet", [0.485, 0.456, 0.406], [0.229, 0.224, 0.225])):
        proc = ViTImageProcessorPil(do_resize=False, do_rescale=True, rescale_factor=1 / 255, do_normalize=True, image_mean=mean, image_std=std)
        t = proc(images=ramp, return_tensors="np", input_data_format="channels_first").pixel_values[0]
        assert t.shape == (3, 256, 2) and np.array_equal(t[..., 0], t[..., 1])
        data["table." + tag] = t[..., 0].copy()
        data["table." + tag + ".mean_std"] = np.array([mean, std], dtype=np.float64)
    data["versions"] = np.array([f"Pillow {PIL.__version__}", f"transformers {transformers.__version__}", f"numpy {np.__version__}"])
    np.savez_compressed(OUT, **data)
    size = os.path.getsize(OUT)
    print(f"{OUT}: {size} bytes, {len(CASES)} cases")
    if size > 512 * 1024:
        sys.exit("golden file larger than 512 KB")


if __name__ == "__main__":
    main()
