"""diffute_amd - MI355X-native (gfx950) hot path of DiffUTE behind the reference's diffusers surface.

Public names mirror what train_diffute_v1.py / app.ipynb import from diffusers
(`AutoencoderKL, DDPMScheduler, UNet2DConditionModel`, train_diffute_v1.py:51) so the scripts can
switch with `from diffute_amd import ...`.
"""
from .models import (AutoencoderKL, UNet2DConditionModel, DiagonalGaussianDistribution, TrOCREncoder,
                     SD2_INPAINT_UNET_CONFIG, SD_VAE_CONFIG, TROCR_LARGE_VIT_CONFIG)
from .schedulers import DDIMScheduler, DDPMScheduler, DPMSolverMultistepScheduler, Guidance, SD2_SCHEDULER_CONFIG
from .pipeline import denoise, edit_boxes, edit_boxes_verified, edit_latents, edit_pages, edit_curved, edit_pages_verified, edit_quads, edit_quads_verified, mask_to_latent
from .inflight import DenoiseEngine
from .optim import FusedAdamW, GradScaler
from .training_utils import EMAModel
from .lora import LoraConfig
from .ocr import TrOCRForCausalLM, VisionEncoderDecoderModel, TROCR_LARGE_DECODER_CONFIG
from .processing import TrOCRProcessor, ViTImageProcessor
from .glyphs import GlyphAtlas, GlyphRenderer, glyph_contexts
from .data import SyntheticDocuments, sample_boxes, training_batch
from ._cabi import set_exclusive_device, synchronize
from .prepost import PasteBlend, QuadBlend

__all__ = ["AutoencoderKL", "UNet2DConditionModel", "DDPMScheduler", "DDIMScheduler", "DPMSolverMultistepScheduler", "DenoiseEngine", "Guidance", "denoise", "edit_latents", "edit_boxes", "edit_boxes_verified", "edit_pages", "edit_pages_verified", "edit_quads", "edit_quads_verified", "edit_curved",
           "mask_to_latent", "FusedAdamW", "GradScaler", "EMAModel", "TrOCREncoder", "TrOCRForCausalLM", "VisionEncoderDecoderModel", "TrOCRProcessor", "ViTImageProcessor", "GlyphAtlas", "GlyphRenderer", "glyph_contexts", "SyntheticDocuments", "sample_boxes", "training_batch", "TROCR_LARGE_DECODER_CONFIG", "TROCR_LARGE_VIT_CONFIG", "DiagonalGaussianDistribution", "SD2_INPAINT_UNET_CONFIG", "SD_VAE_CONFIG",
           "SD2_SCHEDULER_CONFIG", "set_exclusive_device", "synchronize", "LoraConfig", "PasteBlend", "QuadBlend"]
__version__ = "0.1.0"
from . import prepost  # noqa: E402,F401  (on-device pre/post-processing)
from . import metrics  # noqa: E402,F401  (per-box MSE / PSNR / SSIM and the outside-the-boxes diff of two versions of a page)
