"""D1 composed (train_diffute_v1.py:780,925): world_size = 2 through `set_gradient_sync` + the HIP backward.
The two ranks were started by conftest.py at session start (tests/d1_world2_worker.py says what each computes)."""
import json
import os

import pytest
import torch

pytestmark = pytest.mark.gpu


def test_gradient_sync_world2_through_the_hip_backward(cuda):
    from conftest import D1_WORLD2
    procs, prefix = D1_WORLD2["procs"], D1_WORLD2["prefix"]
    if not procs:
        pytest.skip("world-2 workers were not started (session not selected with -m gpu)")
    for p in procs:
        p.wait(timeout=600)
    res = []
    for r in range(2):
        path = f"{prefix}.rank{r}.json"
        assert os.path.exists(path), f"rank {r} wrote no result (exit code {procs[r].returncode})"
        with open(path) as f:
            res.append(json.load(f))
    for r in res:
        assert r["ok"], r.get("error")
    g0 = torch.load(f"{prefix}.rank0.pt"); g1 = torch.load(f"{prefix}.rank1.pt")
    assert torch.equal(g0, g1), "the two ranks hold different synchronised gradients"
    for r in res:
        # mean of the two single-rank gradients to fp32 rounding: 1/world = 1/2 is folded into dLoss/dpred before the backward,
        # a power of two commutes with every rounding of the backward, so only the final fp32 sum differs from the fp64 mean
        assert r["rel_err"] < 1e-5, r
        assert r["differs_from_own"] > 1e-2, "the synchronised gradient equals the rank's own: nothing was exchanged"
        assert r["exposed_ms"] is not None and r["exposed_ms"] >= 0.0
        assert abs(r["loss_mean"] - r["loss_expected"]) < 1e-5 * max(1.0, abs(r["loss_expected"]))
    print(f"D1 world 2: rel err vs mean of single-rank gradients {res[0]['rel_err']:.2e} / {res[1]['rel_err']:.2e}, "
          f"exposed exchange {res[0]['exposed_ms']:.3f} / {res[1]['exposed_ms']:.3f} ms, ranks bit-equal")


def test_ddp_wrap_world2_through_the_hip_backward(cuda):
    """torch's DistributedDataParallel around the HIP UNet, world 2 (what accelerate wraps the module in across ranks,
    train_diffute_v1.py:780; INTEGRATION.md "wrapping the module in torch DDP works"), computed by `ddp_leg` of
    tests/d1_world2_worker.py after the exchange check above, under set_exclusive_device(False) (the ranks share the GPU):
    the constructor's broadcast reaches the packed weights (a perturbed rank 1 gives rank 0's loss, bit for bit); a synchronised
    backward leaves the same bits on both ranks, within 1e-6 rel-L2 of the fp64 mean of the two single-rank gradients (DDP
    pre-divides by the world size - halving is exact - so one fp32 rounding of the sum remains, ~6e-8 per element) and more than
    1e-2 away from the rank's own; under no_sync() `.grad` IS the rank's own gradient; the synchronised backward after it, without
    zero_grad, delivers g0 + g1 to 1e-6."""
    from conftest import D1_WORLD2
    procs, prefix = D1_WORLD2["procs"], D1_WORLD2["prefix"]
    if not procs:
        pytest.skip("world-2 workers were not started (session not selected with -m gpu)")
    for p in procs:
        p.wait(timeout=600)
    res = []
    for r in range(2):
        path = f"{prefix}.rank{r}.json"
        assert os.path.exists(path), f"rank {r} wrote no result (exit code {procs[r].returncode})"
        with open(path) as f:
            res.append(json.load(f))
    for r in res:
        assert "ddp" in r, r.get("ddp_error") or r.get("error") or f"rank {r['rank']} never reached the DDP leg"
    for r in res:
        d = r["ddp"]
        assert d["refs_equal_across_ranks"], "the single-rank reference gradients differ between the ranks"
        assert d["state_differs_before_wrap"], "the perturbation of rank 1 did not register: the leg proves nothing"
        assert d["state_equal_after_wrap"], "state_dict differs between the ranks after DDP's constructor broadcast"
        assert d["loss_after_wrap_bit_equal"], \
            f"rank {r['rank']}: loss {d['loss_after_wrap']!r} after wrapping vs rank 0's reference {d['loss_rank0_reference']!r}: the packed weights missed DDP's broadcast"
        assert d["sync_bit_equal_across_ranks"], "the two ranks hold different gradients after a synchronised backward"
        assert d["sync_rel_err"] <= 1e-6, d
        assert d["sync_differs_from_own"] > 1e-2, "the synchronised gradient equals the rank's own: nothing was exchanged"
        assert d["no_sync_equals_own"], f"rank {r['rank']}: under no_sync() .grad differs from the rank's own gradient by {d['no_sync_rel_err']:.2e}"
        assert d["accum_bit_equal_across_ranks"], "the two ranks hold different gradients after no_sync + a synchronised backward"
        assert d["accum_rel_err"] <= 1e-6, d
    print(f"DDP world 2: synchronised gradient vs fp64 mean {res[0]['ddp']['sync_rel_err']:.2e} / {res[1]['ddp']['sync_rel_err']:.2e}, "
          f"no_sync + sync vs g0 + g1 {res[0]['ddp']['accum_rel_err']:.2e} / {res[1]['ddp']['accum_rel_err']:.2e}, "
          f"leg wall time {res[0]['ddp']['seconds']:.2f} / {res[1]['ddp']['seconds']:.2f} s")
