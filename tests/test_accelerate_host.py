"""The twin loop of tests/accelerate_loops.py is a faithful restatement of the reference's accelerate loop (train_diffute_v1.py:873-930):
on the CPU, on a small torch module whose forward returns a namespace with `.sample` as the product classes do, the two loops give
bit-identical losses, gradients, clip norms and parameters over two optimizer steps of two micro-steps, and the same sync_gradients
sequence.  This is the reference side of assertion (a) of tests/test_accelerate_gpu.py, which runs the same two functions on the HIP models."""
from types import SimpleNamespace

import pytest
import torch
from torch import nn

pytest.importorskip("accelerate")
import accelerate_loops as AL  # noqa: E402


class _Tiny(nn.Module):
    def __init__(self):
        super().__init__()
        g = torch.Generator().manual_seed(3)
        self.a = nn.Linear(12, 24); self.b = nn.Linear(24, 6)
        with torch.no_grad():
            for p in self.parameters():
                p.copy_(torch.randn(p.shape, generator=g) * 0.3)

    def forward(self, x, scale):
        return SimpleNamespace(sample=self.b(torch.tanh(self.a(x))) * scale)


def _batches(n):
    g = torch.Generator().manual_seed(5)
    return [((torch.randn(7, 12, generator=g), 1.0 + 0.25 * i), torch.randn(7, 6, generator=g)) for i in range(n)]


@pytest.fixture
def fresh_accelerate():
    AL.reset_accelerate_state()
    yield
    AL.reset_accelerate_state()


@pytest.mark.parametrize("mp", ["no", "bf16"])
def test_twin_loop_restates_the_accelerate_loop(fresh_accelerate, mp):
    predict = lambda m, x, s: m(x, s).sample                                      # noqa: E731
    a, b = _Tiny(), _Tiny()
    assert all(torch.equal(v, b.state_dict()[k]) for k, v in a.state_dict().items())
    batches = _batches(2 * AL.ACCUM)
    acc = AL.accelerate_loop(a, predict, batches, mp, max_norm=0.05, cpu=True)
    twin = AL.twin_loop(b, predict, batches, mp, max_norm=0.05, device_type="cpu", autocast=True)
    assert acc.sync == [False, True, False, True]
    AL.assert_same_run(acc, twin)
    AL.assert_step_accounting(acc); AL.assert_step_accounting(twin)
    assert acc.steps == 2 and not any(acc.skipped)
    assert all(float(n) > 0.05 for n in acc.norm), f"the clip never clipped: {[float(n) for n in acc.norm]}"
    if mp == "bf16":
        # the restatement is not vacuous: without autocast the same module computes something else
        c = _Tiny()
        plain = AL.twin_loop(c, predict, batches, "no", max_norm=0.05, device_type="cpu")
        assert not AL.bit_equal(plain.loss[0], acc.loss[0]), "bf16 autocast changed nothing on a torch module"
