"""LoRA on the full-size UNet (random weights, r = 16 on the default targets: the 128 attention projections), three figures in one process:

 (a) adapter switch: `set_adapters(other)` until the arena is ready (dmx_unet_lora_apply: merge, pack of the 128 targets, refresh of the derived
     weights), synchronised - against what a user without adapters does: `load_state_dict` of the pre-merged weights (already on the device) plus
     the full `_ensure_packed` of all 686 parameters, on a second model in the same process;
 (b) one training step at the cfg4 per-GPU shape (8 x 512 px, bf16; VAE encodes + forward + backward + clip + optimizer): the adapters under
     torch.optim.AdamW(unet.lora_parameters()) against the full fine-tune under FusedAdamW, with torch.cuda.max_memory_allocated of each.  The
     LoRA model is measured first, with nothing but the VAE and the batch beside it; the full fine-tune's peak is taken with the LoRA model still
     resident and reported less what was resident when it started, plus what both sides share (the VAE, its workspace, the batch);
 (c) the size of the adapter file.

    python scripts/bench_lora.py [--windows 7] [--out profiles/lora_line.json]

(a) and (b) are medians of --windows round-robin windows (one measurement of each side per window) after two warm-up windows.  One JSON line."""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--rank", type=int, default=16)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lora_line.json"))
    args = ap.parse_args()
    import diffute_amd as D
    from diffute_amd.training import encode_latents, train_step
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    GB = 2.0 ** 30

    def sync_ms(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        t1 = time.perf_counter()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, (t1 - t0) * 1e3

    # what both training sides share: the frozen VAE (with the workspace of its encodes) and the batch
    vae = D.AutoencoderKL(device=dev).requires_grad_(False)
    B = args.batch
    gd = torch.Generator(device=dev).manual_seed(5)
    batch = dict(pixel_values=torch.rand(B, 3, 512, 512, device=dev, generator=gd) * 2 - 1, masked_images=torch.rand(B, 3, 512, 512, device=dev, generator=gd) * 2 - 1,
                 masks=(torch.rand(B, 1, 512, 512, device=dev, generator=gd) > 0.7).float(), ocr_embeddings=torch.randn(B, 577, 1024, device=dev, generator=gd))
    with torch.no_grad():
        encode_latents(vae, torch.cat([batch["pixel_values"], batch["masked_images"]], 0))
    torch.cuda.synchronize()
    shared = torch.cuda.memory_allocated(dev)

    unet = D.UNet2DConditionModel(device=dev)
    g = torch.Generator().manual_seed(0)
    for name in ("a", "b"):
        unet.add_adapter(D.LoraConfig(r=args.rank, lora_alpha=args.rank), adapter_name=name)
        with torch.no_grad():
            for p in unet.lora_parameters(name):
                p.copy_((torch.randn(p.shape, generator=g) * 0.02).to(dev))
    n_lora = sum(p.numel() for p in unet.lora_parameters("a"))
    n_base = sum(p.numel() for k, p in unet.named_parameters() if not k.startswith("lora_adapters."))

    # ---- (c) the file
    with tempfile.TemporaryDirectory() as d:
        file_bytes = os.path.getsize(unet.save_lora_weights(d, "a"))

    # ---- (a) the switch
    merged = {}
    base_sd = {k: v for k, v in unet.state_dict().items() if not k.startswith("lora_adapters.")}
    for name in ("a", "b"):
        unet.set_adapters(name)
        sd = dict(base_sd)
        sd.update({k: v.clone() for k, v in unet.merged_lora_weights().items()})
        merged[name] = sd
    plain = D.UNet2DConditionModel(device=dev)
    plain.load_state_dict(merged["b"]); plain._ensure_packed()
    sw, sw_host, rp, rp_load = [], [], [], []
    for w in range(args.windows + 2):
        name = "ab"[w % 2]

        def switch():
            unet.set_adapters(name); unet._ensure_packed()

        def load():
            plain.load_state_dict(merged[name])
        t, h = sync_ms(switch)
        tl, _ = sync_ms(load)
        tp, _ = sync_ms(plain._ensure_packed)
        if w >= 2:
            sw.append(t); sw_host.append(h); rp.append(tl + tp); rp_load.append(tl)
    same = bool(torch.equal(unet._arena, plain._arena))              # both now hold the adapter of the last window
    del plain, merged
    torch.cuda.empty_cache()

    # ---- (b) the training step
    sched = D.DDPMScheduler()
    st = torch.cuda.Stream(device=dev)
    unet.set_adapters("a")
    opt_l = torch.optim.AdamW(unet.lora_parameters("a"), lr=1e-4, weight_decay=1e-2)

    def lora_step():
        return train_step(unet, vae, sched, opt_l, batch, generator=gd)
    torch.cuda.synchronize(); torch.cuda.reset_peak_memory_stats(dev)
    with torch.cuda.stream(st):
        for _ in range(2):
            lora_step()
    torch.cuda.synchronize()
    lora_peak = torch.cuda.max_memory_allocated(dev)
    held = torch.cuda.memory_allocated(dev)                           # the LoRA model, its arenas and the VAE stay resident below
    full = D.UNet2DConditionModel(device=dev)
    torch.cuda.synchronize(); torch.cuda.reset_peak_memory_stats(dev)
    opt_f = D.FusedAdamW(full, lr=1e-4, betas=(0.9, 0.999), weight_decay=1e-2, eps=1e-8, max_grad_norm=1.0)

    def full_step():
        return train_step(full, vae, sched, opt_f, batch, generator=gd)
    with torch.cuda.stream(st):
        for _ in range(2):
            full_step()
    torch.cuda.synchronize()
    full_raw = torch.cuda.max_memory_allocated(dev)
    full_peak = full_raw - held + shared                             # (the VAE and the batch count for both sides)
    tl, tf = [], []
    with torch.cuda.stream(st):
        for _ in range(args.windows):
            tl.append(sync_ms(lora_step)[0]); tf.append(sync_ms(full_step)[0])
    r = lora_step()

    med = lambda v: round(statistics.median(v), 2)     # noqa: E731
    res = dict(bench="lora", rank=args.rank, targets=len(unet._lora["a"].layers), windows=args.windows,
               lora_parameters=n_lora, base_parameters=n_base,
               switch_ms=med(sw), switch_host_ms=med(sw_host), switch_min_max_ms=[round(min(sw), 2), round(max(sw), 2)],
               full_repack_ms=med(rp), full_repack_load_state_dict_ms=med(rp_load), full_repack_min_max_ms=[round(min(rp), 2), round(max(rp), 2)],
               switch_arena_equals_repack=same,
               train_batch=B, lora_adamw_step_ms=med(tl), full_fused_adamw_step_ms=med(tf),
               lora_max_mem_gb=round(lora_peak / GB, 2), full_max_mem_gb=round(full_peak / GB, 2), full_max_mem_raw_gb=round(full_raw / GB, 2),
               resident_when_full_started_gb=round(held / GB, 2), shared_vae_and_batch_gb=round(shared / GB, 2),
               lora_loss=float(r["loss"]), adapter_file_mb=round(file_bytes / 1e6, 2))
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
