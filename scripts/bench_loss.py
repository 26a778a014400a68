"""Time of the loss stage of a training step, per call, v-prediction, B x 4 x 64 x 64: the weighted objective's one entry against the
composition the plain objective runs (scheduler.get_velocity + mse_loss + the multiply by the upstream gradient), at two levels -
`entry`: ops.diffusion_loss(grad_scale=g) against get_velocity + ops.mse_loss + a torch multiply; `autograd`: what train_step runs,
training.diffusion_loss(...).loss.backward() (with its four derived per-sample fields) against models.mse_loss(...).backward().

    python scripts/bench_loss.py [--batch 8] [--repeats 7] [--out profiles/diffusion_loss_line.json]

Each figure is the median of --repeats calls, each between two synchronisations, after three warm-up calls.  Both are launch-bound (a few small
kernels on 0.5 MB), so the figures are host time as much as device time; prints one JSON line."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "diffusion_loss_line.json"))
    args = ap.parse_args()
    import diffute_amd as D
    from diffute_amd.models import mse_loss
    from diffute_amd.training import diffusion_loss
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    B = args.batch
    gen = torch.Generator(device=dev).manual_seed(0)
    pred, lat, noise = (torch.randn(B, 4, 64, 64, device=dev, generator=gen) for _ in range(3))
    mask = torch.zeros(B, 1, 64, 64, device=dev); mask[:, :, 16:40, 8:56] = 1
    ts = torch.randint(0, 1000, (B,), device=dev, generator=gen)
    sched = D.DDPMScheduler(prediction_type="v_prediction")

    from diffute_amd import ops
    sa, sb = sched._coef_tables(dev)
    wt = sched._loss_weight_table(dev, 5.0)
    g = torch.tensor(1024.0, device=dev)

    def composed_entry():
        _, dp = ops.mse_loss(pred, sched.get_velocity(lat, noise, ts))
        return dp * g

    def fused_entry():
        return ops.diffusion_loss(pred, lat, noise, ts, sa, sb, wt, mask=mask, v_prediction=True, mask_weight=4.0, grad_scale=1024.0)

    def composed():
        p = pred.clone().requires_grad_(True)
        mse_loss(p, sched.get_velocity(lat, noise, ts)).backward()

    def fused():
        p = pred.clone().requires_grad_(True)
        diffusion_loss(p, lat, noise, ts, sched, mask=mask, snr_gamma=5.0, mask_weight=4.0).loss.backward()

    def median_us(fn):
        for _ in range(3):
            fn()
        times = []
        for _ in range(args.repeats):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            times.append((time.perf_counter() - t0) * 1e6)
        return round(statistics.median(times), 1)

    res = dict(bench="diffusion_loss", batch=B, shape=[B, 4, 64, 64], repeats=args.repeats, prediction_type="v_prediction",
               entry_composed_get_velocity_mse_multiply_us=median_us(composed_entry), entry_diffusion_loss_us=median_us(fused_entry),
               autograd_composed_us=median_us(composed), autograd_diffusion_loss_us=median_us(fused))
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
