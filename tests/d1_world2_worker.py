"""One rank of the world-2 composition check of D1 (train_diffute_v1.py:780,925): the in-backward, bucketed
gradient exchange (UNet2DConditionModel.set_gradient_sync) running through the REAL HIP backward with world_size = 2.

Both ranks share cuda:0 (the box has one GPU), so the group is gloo (RCCL refuses two ranks on one device) and the exchange
schedule is mode="all_reduce" (gloo has no CUDA reduce-scatter).  Started by tests/conftest.py at session start - before the
pytest process has touched the GPU - and judged by tests/test_dist_gpu.py from the JSON / tensor files written here.

Each rank: the single-rank gradients of BOTH ranks' inputs (no exchange), then one synchronised backward on its own input.
Expected: synchronised gradient == mean of the two single-rank gradients (to fp32 rounding: 1/world is folded into dLoss/dpred
before the backward instead of applied after the sum), bit-identical on both ranks, exposed_exchange_ms() populated.

After that, and independent of it (its own try, its own result fields), `ddp_leg`: the same model wrapped in torch's
DistributedDataParallel, as accelerate does across ranks.
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
TINY_UNET = dict(block_out_channels=(64, 128, 256, 256), attention_head_dim=(1, 2, 4, 4), cross_attention_dim=128)
DDP_PERTURBED = "mid_block.resnets.0.conv1.weight"


def write_result(out, rank, res):
    path = out + f".rank{rank}.json"
    with open(path + ".tmp", "w") as f:
        json.dump(res, f)
    os.replace(path + ".tmp", path)


def ddp_leg(D, torch, dist, model, inputs, rank, world):
    """torch.nn.parallel.DistributedDataParallel around the HIP model (what accelerate wraps the module in across ranks,
    train_diffute_v1.py:780), judged by test_ddp_wrap_world2_through_the_hip_backward.  On a gloo group of its own with a 120 s
    timeout; the two ranks share cuda:0, so the library is told that it does not have the device to itself, and the single-rank
    references are computed under that same setting.  Loss is torch's F.mse_loss (:918).  Returns the measured fields."""
    import time
    from datetime import timedelta
    import torch.nn.functional as F
    from torch.nn.parallel import DistributedDataParallel
    t_start = time.perf_counter()
    pg = dist.new_group(backend="gloo", timeout=timedelta(seconds=120))
    old_exclusive = D.set_exclusive_device(False)
    try:
        params = list(model.parameters())

        def flat_grad():
            return torch.cat([p.grad.reshape(-1) for p in params])

        def flat_state():
            return torch.cat([v.detach().reshape(-1).float() for v in model.state_dict().values()])

        def backward(net, r):
            x, t, ctx, target = inputs(r)
            loss = F.mse_loss(net(x, t, ctx).sample.float(), target.float())
            loss.backward()
            torch.cuda.synchronize()
            return loss.detach()

        def gathered(t):
            bufs = [torch.empty_like(t) for _ in range(world)]
            dist.all_gather(bufs, t.contiguous(), group=pg)
            return bufs

        def checksum(t):
            """exact: two integer sums over the bit patterns, the second position-weighted"""
            b = t.contiguous().view(torch.int32).to(torch.int64)
            w = torch.arange(b.numel(), device=b.device, dtype=torch.int64) % 65521 + 1
            return torch.stack([b.sum(), (b * w).sum()])

        def same_on_all_ranks(t):
            cs = gathered(checksum(t))
            return all(torch.equal(c, cs[0]) for c in cs)

        def rel(a, b):
            return float((a.double() - b.double()).norm() / b.double().norm())

        o = {}
        # single-rank references under the shared-device setting, on the weights every rank holds (nothing has stepped them)
        refs = []
        for r in range(world):
            model.zero_grad(set_to_none=True)
            l = backward(model, r)
            refs.append((l, flat_grad().clone()))
        model.zero_grad(set_to_none=True)
        (l0, g0), (l1, g1) = refs
        own = refs[rank][1]
        o["refs_equal_across_ranks"] = same_on_all_ranks(g0) and same_on_all_ranks(g1)
        l0_rank0 = gathered(l0.reshape(1))[0]
        # 1-3: rank 1 drifts, DDP's constructor broadcast brings it back
        if rank == 1:
            with torch.no_grad():
                dict(model.named_parameters())[DDP_PERTURBED].mul_(1.5)
        o["state_differs_before_wrap"] = not same_on_all_ranks(flat_state())
        ddp = DistributedDataParallel(model, process_group=pg)
        o["state_equal_after_wrap"] = same_on_all_ranks(flat_state())
        # 4: ... and the packed weights followed it: rank 0's reference loss on both ranks
        with ddp.no_sync():
            x, t, ctx, target = inputs(0)
            l4 = F.mse_loss(ddp(x, t, ctx).sample.float(), target.float()).detach().reshape(1)
        o["loss_after_wrap"] = float(l4); o["loss_rank0_reference"] = float(l0_rank0)
        o["loss_after_wrap_bit_equal"] = bool(torch.equal(l4, l0_rank0))
        # 5: synchronised backward on the rank's own input
        ddp.zero_grad(set_to_none=True)
        backward(ddp, rank)
        gs = flat_grad().clone()
        mean = (g0.double() + g1.double()) / 2
        o["sync_rel_err"] = rel(gs, mean)
        o["sync_differs_from_own"] = float((gs.double() - own.double()).norm() / mean.norm())
        o["sync_bit_equal_across_ranks"] = same_on_all_ranks(gs)
        # 6: no_sync keeps the gradient local
        ddp.zero_grad(set_to_none=True)
        with ddp.no_sync():
            backward(ddp, rank)
        o["no_sync_equals_own"] = bool(torch.equal(flat_grad(), own))
        o["no_sync_rel_err"] = rel(flat_grad(), own)
        # 7: the next synchronised backward exchanges what accumulated: (2 g_rank) / world summed over the ranks
        backward(ddp, rank)
        ga = flat_grad().clone()
        o["accum_rel_err"] = rel(ga, g0.double() + g1.double())
        o["accum_bit_equal_across_ranks"] = same_on_all_ranks(ga)
        o["grad_norm"] = float(mean.norm())
        torch.cuda.synchronize()
        o["seconds"] = time.perf_counter() - t_start
        return o
    finally:
        D.set_exclusive_device(old_exclusive)


def main():
    rank, world, port, out = int(sys.argv[1]), int(sys.argv[2]), sys.argv[3], sys.argv[4]
    os.environ.update(RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK="0", MASTER_ADDR="127.0.0.1", MASTER_PORT=port)
    res = {"rank": rank, "ok": False}
    try:
        import torch
        import torch.distributed as dist
        import diffute_amd as D
        from diffute_amd import dist as DD
        from diffute_amd.models import mse_loss
        from diffute_amd.synthetic import synth_inputs
        dev = torch.device("cuda:0")
        torch.cuda.set_device(dev)
        dist.init_process_group("gloo", rank=rank, world_size=world)
        model = D.UNet2DConditionModel(**TINY_UNET).cuda()              # seeded init: the same weights on every rank
        DD.broadcast_parameters(model.parameters(), dist, src=0, module=model)     # D3 anyway (train_diffute_v1.py:780)

        def inputs(r):
            lat, mask, mlat, ctx = synth_inputs(1, 8, 8, 20, 128, seed=10 * r, device=dev)
            return torch.cat([lat, mask, mlat], 1), torch.tensor([321 + 111 * r], device=dev), ctx, torch.full((1, 4, 8, 8), 1.0 - 0.5 * r, device=dev)

        def grads(r):
            x, t, ctx, target = inputs(r)
            model.zero_grad(set_to_none=True)
            loss = mse_loss(model(x, t, ctx).sample, target)
            loss.backward()
            torch.cuda.synchronize()
            return float(loss.detach()), torch.cat([p.grad.reshape(-1).double() for p in model.parameters()])

        l0, g0 = grads(0)
        l1, g1 = grads(1)
        want = (g0 + g1) / 2
        model.set_gradient_sync(dist, mode="all_reduce")
        lr, gs = grads(rank)
        res["exposed_ms"] = model.exposed_exchange_ms()
        model.set_gradient_sync(None)
        res["loss_mean"] = DD.gather_scalar(lr, dist, world)       # D2
        res["loss_expected"] = (l0 + l1) / 2
        res["rel_err"] = float((gs - want).norm() / want.norm())
        res["max_abs_err"] = float((gs - want).abs().max())
        res["differs_from_own"] = float((gs - (g0 if rank == 0 else g1)).norm() / want.norm())
        res["grad_norm"] = float(want.norm())
        torch.save(gs.float().cpu(), out + f".rank{rank}.pt")
        res["ok"] = True
        write_result(out, rank, res)        # the verdict of the exchange check stands whatever the DDP leg below does
        try:
            res["ddp"] = ddp_leg(D, torch, dist, model, inputs, rank, world)
        except Exception as e:                                            # noqa: BLE001 - reported to its own judging test
            import traceback
            res["ddp_error"] = f"{type(e).__name__}: {e}\n{traceback.format_exc()[-1500:]}"
        dist.barrier()
        dist.destroy_process_group()
    except Exception as e:                                                # noqa: BLE001 - reported to the judging test
        import traceback
        res["error"] = f"{type(e).__name__}: {e}\n{traceback.format_exc()[-1500:]}"
    write_result(out, rank, res)


if __name__ == "__main__":
    main()
