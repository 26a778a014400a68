"""One rank of the world-2 LoRA check (judged by tests/test_lora_world2_gpu.py from the JSON written here): a tiny UNet whose only trainable
Parameters are an adapter's A / B, through the real HIP backward with world_size = 2 - once under `set_gradient_sync` (one all-reduce of the
flat dA / dB tensor behind dmx_lora_grads) and once wrapped in torch's DistributedDataParallel.

Both ranks share cuda:0, so the group is gloo and the library is told that it does not have the device to itself (as tests/d1_world2_worker.py
does).  Per leg: the synchronised gradient is bit-equal on both ranks and within 4 * 2^-24 * max|g| per element of the fp64 mean of the two
single-rank gradients (1 / world is a power of two folded in before the backward or applied by DDP before its sum: exact; the fp32 sum of the
two halves is one rounding); a no_sync backward followed by a synchronised one delivers g0 + g1; after three AdamW steps on different inputs
per rank A and B are bit-equal on both ranks."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
TINY_UNET = dict(block_out_channels=(64, 128, 256, 256), attention_head_dim=(1, 2, 4, 4), cross_attention_dim=128)


def main():
    rank, world, port, out = int(sys.argv[1]), int(sys.argv[2]), sys.argv[3], sys.argv[4]
    os.environ.update(RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK="0", MASTER_ADDR="127.0.0.1", MASTER_PORT=port)
    res = {"rank": rank, "ok": False}
    try:
        from datetime import timedelta
        import torch
        import torch.distributed as dist
        import diffute_amd as D
        from diffute_amd.models import mse_loss
        from diffute_amd.synthetic import synth_inputs
        dev = torch.device("cuda:0")
        torch.cuda.set_device(dev)
        dist.init_process_group("gloo", rank=rank, world_size=world, timeout=timedelta(seconds=120))
        D.set_exclusive_device(False)

        def inputs(r):
            lat, mask, mlat, ctx = synth_inputs(1, 8, 8, 20, 128, seed=10 * r, device=dev)
            return torch.cat([lat, mask, mlat], 1), torch.tensor([321 + 111 * r], device=dev), ctx, torch.full((1, 4, 8, 8), 1.0 - 0.5 * r, device=dev)

        def gathered(t):
            bufs = [torch.empty_like(t) for _ in range(world)]
            dist.all_gather(bufs, t.contiguous())
            return bufs

        def same_on_all_ranks(t):
            b = gathered(t.contiguous().view(torch.int32))
            return all(torch.equal(x, b[0]) for x in b)

        def leg(wrap):
            torch.manual_seed(0)                                          # the same A on every rank (add_adapter draws from torch's RNG)
            model = D.UNet2DConditionModel(**TINY_UNET).cuda()
            model.add_adapter(D.LoraConfig(r=4, lora_alpha=8, target_modules=("to_q", "to_k", "to_v", "to_out.0", "ff.net.2")), adapter_name="a")
            g = torch.Generator().manual_seed(1)
            with torch.no_grad():
                for p in model.lora_parameters():
                    p.copy_((torch.randn(p.shape, generator=g) * 0.05).to(dev))
            params = model.lora_parameters()

            def flat_grad():
                return torch.cat([p.grad.reshape(-1) for p in params])

            def backward(net, r):
                x, t, ctx, target = inputs(r)
                loss = mse_loss(net(x, t, ctx).sample, target)
                loss.backward()
                torch.cuda.synchronize()

            refs = []
            for r in range(world):
                model.zero_grad(set_to_none=True)
                backward(model, r)
                refs.append(flat_grad().double())
            model.zero_grad(set_to_none=True)
            g0, g1 = refs
            mean = (g0 + g1) / 2
            o = {"n": int(mean.numel()), "refs_equal_across_ranks": same_on_all_ranks(g0.float()) and same_on_all_ranks(g1.float())}
            if wrap == "ddp":
                from torch.nn.parallel import DistributedDataParallel
                net = DistributedDataParallel(model)
                no_sync = net.no_sync
            else:
                model.set_gradient_sync(dist, mode="all_reduce")
                net, no_sync = model, model.no_sync
            backward(net, rank)
            gs = flat_grad().clone()
            o["sync_bit_equal_across_ranks"] = same_on_all_ranks(gs)
            o["sync_max_err"] = float((gs.double() - mean).abs().max())
            o["sync_allowed"] = 4 * 2.0 ** -24 * float(mean.abs().max())
            o["sync_differs_from_own"] = float((gs.double() - refs[rank]).norm() / mean.norm())
            net.zero_grad(set_to_none=True)
            with no_sync():
                backward(net, rank)
            o["no_sync_keeps_it_local"] = bool(params[0].grad is None or torch.equal(flat_grad().double(), refs[rank]))
            backward(net, rank)
            ga = flat_grad().clone()
            o["accum_bit_equal_across_ranks"] = same_on_all_ranks(ga)
            o["accum_max_err"] = float((ga.double() - (g0 + g1)).abs().max())
            o["accum_allowed"] = 4 * 2.0 ** -24 * float((g0 + g1).abs().max())
            net.zero_grad(set_to_none=True)
            opt = torch.optim.AdamW(params, lr=1e-3)
            before = torch.cat([p.detach().reshape(-1) for p in params]).clone()
            for step in range(3):
                backward(net, (rank + step) % world)
                opt.step(); opt.zero_grad(set_to_none=True)
            after = torch.cat([p.detach().reshape(-1) for p in params])
            o["params_moved"] = not torch.equal(after, before)
            o["params_equal_after_three_steps"] = same_on_all_ranks(after)
            base = [p for k, p in model.named_parameters() if not k.startswith("lora_adapters.")]
            o["base_has_no_grad"] = all(p.grad is None for p in base)
            if wrap != "ddp":
                model.set_gradient_sync(None)
            return o

        res["sync"] = leg("sync")
        res["ok"] = True
        try:
            res["ddp"] = leg("ddp")
        except Exception as e:                                            # noqa: BLE001 - reported to its own judging test
            import traceback
            res["ddp_error"] = f"{type(e).__name__}: {e}\n{traceback.format_exc()[-1500:]}"
        dist.barrier()
        dist.destroy_process_group()
    except Exception as e:                                                # noqa: BLE001 - reported to the judging test
        import traceback
        res["error"] = f"{type(e).__name__}: {e}\n{traceback.format_exc()[-1500:]}"
    path = out + f".rank{rank}.json"
    with open(path + ".tmp", "w") as f:
        json.dump(res, f)
    os.replace(path + ".tmp", path)


if __name__ == "__main__":
    main()
