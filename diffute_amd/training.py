"""The DiffUTE training step (train_diffute_v1.py:859-935) on the product classes.

    latents / masked latents  : frozen VAE encode -> latent_dist.sample() * scaling_factor      (:875-887)
    mask                      : nearest downsample to the latent grid                             (:880-884)
    noisy latents             : scheduler.add_noise(latents, noise, timesteps)                    (:889-897)
    prediction                : unet(cat([noisy, mask, masked_latents], 1), timesteps, ocr_embeddings).sample   (:911-913)
    loss                      : mse_loss(pred.float(), target.float())                            (:918)
    backward / clip / AdamW   : loss.backward(); clip_grad_norm_(unet.parameters(), 1.0); optimizer.step()   (:925-930)

Every FLOP of the models runs in the HIP library; torch provides the autograd plumbing.  The optimizer is either
diffute_amd.FusedAdamW (clipping + AdamW + EMA as one HIP pass over the packed fp32 arenas) or any
torch optimizer over `unet.parameters()` (the backward then exports per-parameter gradients into `.grad`).  With
`dist` set, gradients are averaged across ranks inside the backward (bucketed RCCL all-reduce of the packed gradient
arena on a side stream, UNet2DConditionModel.set_gradient_sync)."""
import math
from collections import namedtuple

import torch

from . import _cabi, ops
from .models import mse_loss
from .pipeline import mask_to_latent


def encode_latents(vae, images, noise=None, generator=None):
    """vae.encode(x).latent_dist.sample() * scaling_factor, no gradient (the VAE is frozen, train_diffute_v1.py:639)."""
    with torch.no_grad():
        dist = vae.encode(images).latent_dist
        z = dist.sample(noise=noise) if noise is not None else dist.sample(generator=generator)
        return z * vae.config.scaling_factor


def training_target(scheduler, latents, noise, timesteps):
    pt = scheduler.config.prediction_type
    if pt == "epsilon":
        return noise
    if pt == "v_prediction":
        return scheduler.get_velocity(latents, noise, timesteps)
    raise ValueError(f"Unknown prediction type {pt}")                      # train_diffute_v1.py:909


DiffusionLoss = namedtuple("DiffusionLoss", "loss per_sample_mse masked_mse unmasked_mse weight records")


class _DiffusionLossFn(torch.autograd.Function):
    """dmx_diffusion_loss under autograd: dLoss/dpred is computed with the loss at upstream gradient 1 and scaled in backward, as _MSEFn does"""

    @staticmethod
    def forward(ctx, pred, latents, noise, timesteps, mask, sa, sb, wt, v_prediction, mask_weight):
        loss, records, dp = ops.diffusion_loss(pred.detach().to(torch.float32).contiguous(), latents, noise, timesteps, sa, sb, wt, mask=mask,
                                               v_prediction=v_prediction, mask_weight=mask_weight, grad_scale=1.0)
        ctx.save_for_backward(dp)
        ctx.in_dtype, ctx.in_shape = pred.dtype, pred.shape
        ctx.mark_non_differentiable(records)
        return loss.reshape(()), records

    @staticmethod
    def backward(ctx, g, _):
        (dp,) = ctx.saved_tensors
        return ((dp * g).to(ctx.in_dtype).reshape(ctx.in_shape),) + (None,) * 9


def diffusion_loss(pred, latents, noise, timesteps, scheduler, *, mask=None, snr_gamma=None, mask_weight=0.0):
    """The denoiser's objective with Min-SNR-gamma sample weights and an emphasis on the text box, as one HIP entry (dmx_diffusion_loss, two launches):

        loss = (1/N) sum_b w(t_b) sum_{c,y,x} (1 + mask_weight * M[b,y,x]) (pred - target)^2,        N = B*C*h*w

    target = noise or scheduler.get_velocity(latents, noise, timesteps) by the scheduler's prediction_type (computed inside the kernel, the
    same bits), w = scheduler.loss_weights(snr_gamma), M = `mask` [B,1,h,w] at latent resolution (mask_to_latent: 1 inside the box) or None.
    With snr_gamma=None and mask_weight=0 it is the plain MSE; with mask_weight=0 it is diffusers' Min-SNR loss.  The emphasis is deliberately
    NOT renormalised by sum(1 + mask_weight * M): mask_weight changes the scale of the loss (and of the gradient), not only its balance.
    A timestep outside [0, num_train_timesteps) makes that sample's weight, its gradient rows and the loss NaN.

    Returns DiffusionLoss(loss, per_sample_mse, masked_mse, unmasked_mse, weight, records); only `loss` is differentiable (with respect to
    pred).  per_sample_mse [B] is the unweighted mean of (pred - target)^2 over a sample; masked_mse [B] = sum(M q) / (C sum M) is that mean
    inside the box, NaN where the mask is empty or None; unmasked_mse [B] = sum((1 - M) q) / (C sum(1 - M)) is its complement (the whole
    sample when mask is None); weight [B] = w(t_b); records [B, LOSS_ROW_FLOATS] are the kernel's per-sample sums (include/diffute_hip.h).
    The derived fields are torch arithmetic on the records; nothing synchronises.  Where no gradient is wanted (under no_grad, or a pred that
    does not require one) the kernel is asked for the loss and the records only."""
    lam = float(mask_weight)
    if not (math.isfinite(lam) and lam >= 0):
        raise ValueError(f"mask_weight must be finite and >= 0, got {mask_weight!r}")
    scheduler._check_snr_gamma(snr_gamma)
    pt = scheduler.config.prediction_type
    if pt not in ("epsilon", "v_prediction"):
        raise ValueError(f"Unknown prediction type {pt}")
    if pred.dim() != 4:
        raise ValueError(f"pred must be [B,C,h,w], got {tuple(pred.shape)}")
    B, C, h, w = pred.shape
    if tuple(latents.shape) != tuple(pred.shape):
        raise ValueError(f"latents {tuple(latents.shape)} must have the shape of pred {tuple(pred.shape)}")
    if tuple(noise.shape) != tuple(pred.shape):
        raise ValueError(f"noise {tuple(noise.shape)} must have the shape of pred {tuple(pred.shape)}")
    if timesteps.numel() != B:
        raise ValueError(f"timesteps must have one entry per sample: {timesteps.numel()} for B = {B}")
    if mask is not None and tuple(mask.shape) != (B, 1, h, w):
        raise ValueError(f"mask must be [B,1,h,w] = {(B, 1, h, w)}, got {tuple(mask.shape)}")
    _cabi.require_cuda(pred, latents, noise, mask)
    dev = pred.device
    sa, sb = scheduler._coef_tables(dev)
    wt = scheduler._loss_weight_table(dev, snr_gamma)
    f32 = lambda t: None if t is None else t.detach().to(device=dev, dtype=torch.float32).contiguous()      # noqa: E731
    ts = timesteps.detach().to(dev).reshape(-1).long().contiguous()
    if torch.is_grad_enabled() and pred.requires_grad:
        loss, rec = _DiffusionLossFn.apply(pred, f32(latents), f32(noise), ts, f32(mask), sa, sb, wt, pt == "v_prediction", lam)
    else:                                                 # evaluation: loss and records only, the kernel writes no gradient (dpred = NULL)
        loss, rec, _ = ops.diffusion_loss(f32(pred), f32(latents), f32(noise), ts, sa, sb, wt, mask=f32(mask), v_prediction=pt == "v_prediction",
                                          mask_weight=lam, dpred=None)
        loss = loss.reshape(())
    sq_all, sq_mask, inside = rec[:, _cabi.LOSS_SQ_ALL], rec[:, _cabi.LOSS_SQ_MASK], rec[:, _cabi.LOSS_MASK_SUM] * C
    return DiffusionLoss(loss, sq_all / (C * h * w), sq_mask / inside, (sq_all - sq_mask) / (C * h * w - inside), rec[:, _cabi.LOSS_WEIGHT], rec)


def train_step(unet, vae, scheduler, optimizer, batch, *, noise=None, timesteps=None, enc_noise=None, enc_noise_masked=None,
               max_grad_norm=1.0, generator=None, scaler=None, snr_gamma=None, mask_weight=0.0):
    """One optimizer step.  batch: dict with pixel_values [B,3,H,W], masked_images [B,3,H,W], masks [B,1,H,W] and
    ocr_embeddings [B,S,1024] (the frozen TrOCR encoder's output, train_diffute_v1.py:868-871; from the batch's strings it is
    `diffute_amd.glyph_contexts(batch_texts, renderer, processor, encoder)`, rendered on the device).  The random draws can be
    injected (tests); otherwise they come from torch's device RNG like the reference.  Returns loss / grad_norm tensors.
    scaler: a diffute_amd.GradScaler (or torch.amp.GradScaler with a torch optimizer) - `--mixed_precision fp16` (train_diffute_v1.py:267,583):
    backward on the scaled loss, unscale before clipping, the step skipped and the scale halved when the gradient overflowed.
    snr_gamma / mask_weight: with either set (snr_gamma not None, mask_weight != 0) the objective is `diffusion_loss` with the batch's latent
    mask - Min-SNR-gamma sample weights and / or an emphasis on the text box, target and gradient from one kernel - and the result also
    carries per_sample_mse, masked_mse, unmasked_mse (unweighted, [B]) and the timesteps drawn.  With both at their defaults the step is
    training_target + mse_loss, as it always was."""
    pv = batch["pixel_values"]
    # both frozen-VAE encodes (train_diffute_v1.py:875,886) as one batch of 2B images: same arithmetic per image, half the launches
    nz = None if enc_noise is None else torch.cat([enc_noise, enc_noise_masked], 0)
    both = encode_latents(vae, torch.cat([pv, batch["masked_images"]], 0), nz, generator)
    latents, masked_latents = both[:pv.shape[0]].contiguous(), both[pv.shape[0]:].contiguous()
    factor = 2 ** (len(vae.config.block_out_channels) - 1)
    mask = mask_to_latent(batch["masks"], factor).to(latents.dtype)
    B = latents.shape[0]
    if noise is None:
        noise = torch.randn(latents.shape, device=latents.device, dtype=latents.dtype, generator=generator)
    if timesteps is None:
        timesteps = torch.randint(0, scheduler.num_train_timesteps, (B,), device=latents.device, generator=generator).long()
    noisy = scheduler.add_noise(latents, noise, timesteps)
    weighted = snr_gamma is not None or mask_weight != 0
    extra = {}
    if not weighted:
        target = training_target(scheduler, latents, noise, timesteps)
    pred = unet(torch.cat([noisy, mask, masked_latents], dim=1), timesteps, batch["ocr_embeddings"]).sample
    if weighted:
        dl = diffusion_loss(pred.float(), latents, noise, timesteps, scheduler, mask=mask, snr_gamma=snr_gamma, mask_weight=mask_weight)
        loss = dl.loss
        extra = dict(per_sample_mse=dl.per_sample_mse, masked_mse=dl.masked_mse, unmasked_mse=dl.unmasked_mse, timesteps=timesteps)
    else:
        loss = mse_loss(pred.float(), target.float())
    (loss if scaler is None else scaler.scale(loss)).backward()
    if hasattr(optimizer, "masters"):                 # diffute_amd.optim.FusedAdamW: (unscaling,) clipping and the update are one HIP pass
        if scaler is None:
            optimizer.step()
        else:
            scaler.step(optimizer); scaler.update()
        grad_norm = optimizer.grad_norm
    else:
        if scaler is not None:
            scaler.unscale_(optimizer)
        grad_norm = torch.nn.utils.clip_grad_norm_(unet.parameters(), max_grad_norm) if max_grad_norm else None
        if scaler is None:
            optimizer.step()
        else:
            scaler.step(optimizer); scaler.update()
        optimizer.zero_grad(set_to_none=True)
    return dict(loss=loss.detach(), grad_norm=grad_norm, **extra)


def train_vae_step(vae, optimizer, images, target=None, max_grad_norm=None, scaler=None):
    """One optimizer step of train_vae.py:716-736: pred = vae(x)["sample"] (decode of the posterior mode),
    loss = mse_loss(pred.float(), target.float()), backward, optimizer step.  `target` defaults to the input images.
    scaler: loss scaling for the fp16 build (see train_step)."""
    pred = vae(images)["sample"]
    loss = mse_loss(pred.float(), (images if target is None else target).float())
    (loss if scaler is None else scaler.scale(loss)).backward()
    if scaler is not None:
        scaler.unscale_(optimizer)
    grad_norm = torch.nn.utils.clip_grad_norm_(vae.parameters(), max_grad_norm) if max_grad_norm else None
    if scaler is None:
        optimizer.step()
    else:
        scaler.step(optimizer); scaler.update()
    optimizer.zero_grad(set_to_none=True)
    return dict(loss=loss.detach(), grad_norm=grad_norm)
