"""Restatement of the step cache (DeepCache-style reuse of the deep UNet features; Ma et al., CVPR 2024), built from the oracle's own
layer functions - test infrastructure, never the thing under test.

A full step is oracle.unet.unet_forward; the tensor it keeps is its tap "up2": the output of the last upsampler, what enters
up-block 3.  A shallow step runs conv_in, down-block 0 (without its downsampler: nothing reads that), up-block 3 on the kept tensor,
conv_norm_out and conv_out.  cached_denoise is oracle.pipeline.denoise with step i full iff i % cache_interval == 0.
"""
import torch
import torch.nn.functional as F

from oracle import schedulers as S
from oracle.unet import _conv, _gn, _q, resnet, timestep_embedding, transformer2d, unet_forward


@torch.no_grad()
def shallow_forward(P, cfg, sample, timestep, ctx, cache, emulate_bf16=False):
    """eps of a shallow step: `cache` is the "up2" tap [B, block_out_channels[1], h, w] of an earlier full forward."""
    em = emulate_bf16
    boc = cfg["block_out_channels"]; L = cfg["layers_per_block"]
    heads = cfg["attention_head_dim"]; G = cfg["norm_num_groups"]
    B = sample.shape[0]
    t = torch.as_tensor(timestep, dtype=torch.int64).reshape(-1)
    if t.numel() == 1:
        t = t.expand(B)
    sample = _q(sample.to(torch.float32), em)
    ctx = _q(ctx.to(torch.float32), em)
    temb = timestep_embedding(t, boc[0])
    emb = F.linear(temb, _q(P["time_embedding.linear_1.weight"], em), P["time_embedding.linear_1.bias"])
    emb = F.linear(F.silu(emb), _q(P["time_embedding.linear_2.weight"], em), P["time_embedding.linear_2.bias"])
    emb_act = F.silu(emb)
    h = _q(_conv(sample, P, "conv_in.", em), em)
    skips = [h]
    for j in range(L):
        h = resnet(h, emb_act, P, f"down_blocks.0.resnets.{j}.", G, 1e-5, em)
        if cfg["down_has_attn"][0]:
            h = transformer2d(h, ctx, P, f"down_blocks.0.attentions.{j}.", heads[0], G, em)
        skips.append(h)
    h = cache
    i = len(boc) - 1
    for j in range(L + 1):
        h = torch.cat([h, skips.pop()], dim=1)
        h = resnet(h, emb_act, P, f"up_blocks.{i}.resnets.{j}.", G, 1e-5, em)
        if cfg["up_has_attn"][i]:
            h = transformer2d(h, ctx, P, f"up_blocks.{i}.attentions.{j}.", heads[0], G, em)
    assert not skips
    h = _gn(h, P, "conv_norm_out.", G, 1e-5, True, em)
    return _conv(h, P, "conv_out.", em)


@torch.no_grad()
def cached_denoise(P, cfg, latents, mask, masked_latents, ctx, steps, cache_interval, scheduler="ddim", noise=None, emulate_bf16=False,
                   N=1000, refresh=None):
    """oracle.pipeline.denoise with the step cache: step i runs the full UNet and keeps its "up2" tap iff refresh(i) (default:
    i % cache_interval == 0), every other step is shallow_forward on the kept tap.  `refresh` lets a test inject a wrong schedule."""
    ac = S.make_tables(N)[2]
    ts = S.timesteps_ddim(steps, N) if scheduler == "ddim" else S.timesteps_ddpm(steps, N)
    if refresh is None:
        refresh = lambda i: i % cache_interval == 0      # noqa: E731
    x = latents.to(torch.float32).clone()
    cache = None
    for i, t in enumerate(ts):
        inp = torch.cat([x, mask.to(torch.float32), masked_latents.to(torch.float32)], dim=1)
        if cache is None or refresh(i):
            taps = {}
            eps = unet_forward(P, cfg, inp, torch.tensor(int(t)), ctx, emulate_bf16=emulate_bf16, taps=taps)
            cache = taps["up2"]
        else:
            eps = shallow_forward(P, cfg, inp, torch.tensor(int(t)), ctx, cache, emulate_bf16=emulate_bf16)
        if scheduler == "ddim":
            xn = S.ddim_step(ac, eps.numpy(), int(t), x.numpy(), steps, N)
        else:
            xn = S.ddpm_step(ac, eps.numpy(), int(t), x.numpy(), steps, N, noise=None if noise is None else noise[i].numpy())
        x = torch.from_numpy(xn)
    return x
