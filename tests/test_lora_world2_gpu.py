"""LoRA training with world_size = 2 through the HIP backward: under `set_gradient_sync` (one all-reduce of the flat dA / dB tensor) and under
torch's DistributedDataParallel.  tests/lora_world2_worker.py says what each rank computes.

The two ranks are separate processes.  A process that has touched the GPU must not start others, so they are started when this module is
IMPORTED - at collection, before any test of the session has run - and only when a GPU is visible, this process has not initialised it and the
session was not selected with `-m "not gpu"`.  The import waits for them: nothing else may hold the GPU while the other tests run."""
import json
import os
import subprocess
import sys
import tempfile

import pytest
import torch

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
WORLD2 = {"procs": None, "prefix": None, "why": "no GPU visible"}


def _markexpr():
    argv = sys.argv[1:]
    for i, a in enumerate(argv):
        if a == "-m" and i + 1 < len(argv):
            return argv[i + 1]
        if a.startswith("-m") and len(a) > 2 and not a.startswith("--"):
            return a[2:]
    return ""


def _start_workers():
    if "not gpu" in _markexpr():
        WORLD2["why"] = "session selected with -m 'not gpu'"
        return
    if torch.cuda.device_count() < 1:              # (does not initialise the device)
        return
    if torch.cuda.is_initialized():
        WORLD2["why"] = "this process had initialised the GPU before the module was imported"
        return
    import socket
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0)); port = sk.getsockname()[1]
    prefix = os.path.join(tempfile.mkdtemp(prefix="lora_world2_"), "res")
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    worker = os.path.join(HERE, "lora_world2_worker.py")
    WORLD2["procs"] = [subprocess.Popen([sys.executable, worker, str(r), "2", str(port), prefix], env=env,
                                        stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL) for r in range(2)]
    WORLD2["prefix"] = prefix
    for p in WORLD2["procs"]:
        try:
            p.wait(timeout=300)
        except subprocess.TimeoutExpired:
            p.kill()                                # the judging tests report the missing result


_start_workers()


@pytest.fixture(scope="module")
def results(cuda):
    procs, prefix = WORLD2["procs"], WORLD2["prefix"]
    assert procs, f"the world-2 LoRA workers were not started: {WORLD2['why']}"
    res = []
    for r in range(2):
        path = f"{prefix}.rank{r}.json"
        assert os.path.exists(path), f"rank {r} wrote no result (exit code {procs[r].returncode})"
        with open(path) as f:
            res.append(json.load(f))
    return res


def judge(res, leg):
    for r in res:
        assert leg in r, r.get(f"{leg}_error") or r.get("error") or f"rank {r['rank']} never reached the {leg} leg"
    for r in res:
        d = r[leg]
        assert d["refs_equal_across_ranks"], "the single-rank reference gradients differ between the ranks"
        assert d["sync_bit_equal_across_ranks"], "the two ranks hold different LoRA gradients after a synchronised backward"
        assert d["sync_max_err"] <= d["sync_allowed"], d
        assert d["sync_differs_from_own"] > 1e-2, "the synchronised gradient equals the rank's own: nothing was exchanged"
        assert d["no_sync_keeps_it_local"], d
        assert d["accum_bit_equal_across_ranks"], d
        assert d["accum_max_err"] <= d["accum_allowed"], d
        assert d["params_moved"] and d["params_equal_after_three_steps"], d
        assert d["base_has_no_grad"], d
    print(f"LoRA world 2 ({leg}): {res[0][leg]['n']} gradient elements, max err vs fp64 mean {res[0][leg]['sync_max_err']:.2e} "
          f"(allowed {res[0][leg]['sync_allowed']:.2e}), no_sync + sync vs g0 + g1 {res[0][leg]['accum_max_err']:.2e} (allowed {res[0][leg]['accum_allowed']:.2e})")


def test_lora_gradient_sync_world2(results):
    for r in results:
        assert r["ok"], r.get("error")
    judge(results, "sync")


def test_lora_ddp_world2(results):
    judge(results, "ddp")
