"""Does the training loop learn on rendered text, and does the glyph context carry anything the UNet can use?

    python scripts/train_synthetic.py [--steps 300] [--batch 4] [--lr 2e-4] [--size 128] [--eval-pages 8] [--context_dropout 0]
                                      [--snr_gamma G] [--mask_weight L] [--out profiles/train_synthetic_line.json]

The tiny UNet / VAE / glyph encoder of the tests (random initialisation; VAE and encoder frozen, as in the reference) are trained with
train_step + FusedAdamW on SyntheticDocuments.batches: pages composed on the device, one confident line per page, the reference's
256-pixel crop resized to --size, the line's text rendered and encoded as the glyph context.  Held-out pages (indices the training never
reaches) are evaluated at fixed timesteps and fixed noise in two ways: with each row's OWN glyph context, and with the contexts ROTATED
by one row (row b gets the text of row b + 1).  If the UNet uses the context, the own-context loss falls below the rotated one.

Prints one JSON line (and writes it to --out): the mean loss of the first and of the last tenth of the steps, and the two held-out losses
before and after training.  The numbers are reported, not asserted: nobody has measured whether a random frozen VAE leaves a visible gap.

--context_dropout P (the training half of classifier-free guidance, diffute_amd.Guidance): with probability P a training row's glyph
context is replaced by zeros (SyntheticDocuments.batches(context_dropout=P)).  The line then also carries the held-out loss under the NULL
(all-zero) context before and after training, next to the own / rotated figures.  With the default 0 the line is what it always was.

--snr_gamma G / --mask_weight L: train on the weighted objective (train_step(snr_gamma=G, mask_weight=L): Min-SNR-gamma sample weights and / or
1 + L times the loss inside the text box, diffute_amd.training.diffusion_loss).  With neither, training and every figure above are what they
always were.  The held-out evaluation is an UNWEIGHTED statistic whatever the training objective, and the line always carries it split at the
text box as well (the `masked` / `unmasked` entries: the mean over rows and EVAL_TIMESTEPS of diffusion_loss(...).masked_mse / .unmasked_mse at
snr_gamma=None, mask_weight=0, no gradient asked of the kernel) for the own, rotated and - with --context_dropout - null contexts, before and
after training, with the own-versus-rotated gap inside the box."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

TINY_UNET = dict(block_out_channels=(64, 128, 256, 256), attention_head_dim=(1, 2, 4, 4), cross_attention_dim=128)      # tests/test_models_gpu.py
TINY_VAE = dict(block_out_channels=(64, 128, 128, 128), layers_per_block=1)
EVAL_TIMESTEPS = (100, 400, 700, 900)
HELD_OUT = 1 << 20              # first held-out page index


@torch.no_grad()
def held_out_loss(unet, vae, scheduler, batch, contexts, fixed):
    """mean over EVAL_TIMESTEPS of the (unweighted) training loss on `batch` with `contexts`, every random draw taken from `fixed`
    -> (loss, the same inside the text box, outside it)"""
    import diffute_amd as D
    from diffute_amd.models import mse_loss
    from diffute_amd.training import diffusion_loss, encode_latents, training_target
    pv = batch["pixel_values"]
    B = pv.shape[0]
    both = encode_latents(vae, torch.cat([pv, batch["masked_images"]], 0), fixed["enc_noise"], None)
    latents, masked = both[:B].contiguous(), both[B:].contiguous()
    mask = D.mask_to_latent(batch["masks"], 2 ** (len(vae.config.block_out_channels) - 1)).to(latents.dtype)
    losses, inside, outside = [], [], []
    for t in EVAL_TIMESTEPS:
        ts = torch.full((B,), t, device=pv.device, dtype=torch.long)
        noisy = scheduler.add_noise(latents, fixed["noise"], ts)
        pred = unet(torch.cat([noisy, mask, masked], 1), ts, contexts).sample
        losses.append(float(mse_loss(pred.float(), training_target(scheduler, latents, fixed["noise"], ts).float())))
        split = diffusion_loss(pred.float(), latents, fixed["noise"], ts, scheduler, mask=mask)
        inside.append(split.masked_mse); outside.append(split.unmasked_mse)
    return sum(losses) / len(losses), float(torch.nanmean(torch.stack(inside))), float(torch.nanmean(torch.stack(outside)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=300)
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--lr", type=float, default=2e-4)
    ap.add_argument("--size", type=int, default=128)
    ap.add_argument("--eval-pages", type=int, default=8)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--context_dropout", type=float, default=0.0)
    ap.add_argument("--snr_gamma", type=float, default=None)
    ap.add_argument("--mask_weight", type=float, default=0.0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "train_synthetic_line.json"))
    args = ap.parse_args()
    import diffute_amd as D
    from diffute_amd.training import train_step
    from glyph_text_cases import load_golden
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    renderer = D.GlyphAtlas.from_arrays(load_golden(), "atlas.").to(dev)
    ds = D.SyntheticDocuments(renderer, page_size=(600, 800), lines=(4, 10), seed=args.seed)
    unet = D.UNet2DConditionModel(**TINY_UNET).to(dev)
    vae = D.AutoencoderKL(**TINY_VAE).to(dev).requires_grad_(False)
    enc = D.TrOCREncoder(device=dev, image_size=64, patch_size=16, hidden_size=TINY_UNET["cross_attention_dim"], num_hidden_layers=1,
                         num_attention_heads=TINY_UNET["cross_attention_dim"] // 64, intermediate_size=256)
    ds.glyph = (renderer, D.TrOCRProcessor(size=64), enc)
    sched = D.DDPMScheduler()
    opt = D.FusedAdamW(unet, lr=args.lr, weight_decay=1e-2, max_grad_norm=1.0)
    gen = torch.Generator(device=dev).manual_seed(args.seed + 1)

    E, S = args.eval_pages, args.size
    held = next(ds.batches(E, np.random.default_rng(args.seed + 2), size=S, start=HELD_OUT))
    fixed = dict(noise=torch.randn(E, 4, S // 8, S // 8, device=dev, generator=gen),
                 enc_noise=torch.randn(2 * E, 4, S // 8, S // 8, device=dev, generator=gen))
    own, rotated = held["ocr_embeddings"], torch.roll(held["ocr_embeddings"], -1, 0)

    def evaluate():
        r = held_out_loss(unet, vae, sched, held, own, fixed), held_out_loss(unet, vae, sched, held, rotated, fixed)
        return r + (held_out_loss(unet, vae, sched, held, torch.zeros_like(own), fixed),) if args.context_dropout > 0 else r

    before = evaluate()
    losses, t0 = [], time.perf_counter()
    drop = dict(context_dropout=args.context_dropout) if args.context_dropout > 0 else {}
    weighted = args.snr_gamma is not None or args.mask_weight != 0
    objective = dict(snr_gamma=args.snr_gamma, mask_weight=args.mask_weight) if weighted else {}
    batches = ds.batches(args.batch, np.random.default_rng(args.seed + 3), size=S, **drop)
    for _ in range(args.steps):
        out = train_step(unet, vae, sched, opt, next(batches), generator=gen, **objective)
        losses.append(out["loss"])
    losses = [float(l) for l in torch.stack(losses).cpu()]
    D.synchronize()
    seconds = time.perf_counter() - t0
    after = evaluate()
    tenth = max(args.steps // 10, 1)
    res = dict(bench="train_synthetic", steps=args.steps, batch=args.batch, lr=args.lr, size=S, eval_pages=E, eval_timesteps=list(EVAL_TIMESTEPS),
               finite=bool(np.isfinite(losses).all()),
               loss_first_tenth=round(float(np.mean(losses[:tenth])), 6), loss_last_tenth=round(float(np.mean(losses[-tenth:])), 6),
               held_out_own_before=round(before[0][0], 6), held_out_rotated_before=round(before[1][0], 6),
               held_out_own_after=round(after[0][0], 6), held_out_rotated_after=round(after[1][0], 6),
               gap_before=round(before[1][0] - before[0][0], 6), gap_after=round(after[1][0] - after[0][0], 6),
               ms_per_step_with_data=round(seconds / args.steps * 1e3, 2))
    if args.context_dropout > 0:
        res.update(context_dropout=args.context_dropout, held_out_null_before=round(before[2][0], 6), held_out_null_after=round(after[2][0], 6),
                   null_gap_before=round(before[2][0] - before[0][0], 6), null_gap_after=round(after[2][0] - after[0][0], 6))
    if weighted:
        res.update(snr_gamma=args.snr_gamma, mask_weight=args.mask_weight)
    for when, r in (("before", before), ("after", after)):
        for i, ctx in enumerate(("own", "rotated", "null")[:len(r)]):
            res[f"masked_{ctx}_{when}"], res[f"unmasked_{ctx}_{when}"] = round(r[i][1], 6), round(r[i][2], 6)
        res[f"masked_gap_{when}"] = round(r[1][1] - r[0][1], 6)
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
