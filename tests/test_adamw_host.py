"""Pins adamw_restatement.py on the CPU (no GPU, no kernel output involved).

  * step64 / full_step64 - the reference test_adamw_gpu.py holds the kernel to - against torch.optim.AdamW + clip_grad_norm_ in fp64 over
    5 steps (1e-12 relative), the EMA recurrence against ema_restatement.py, and the found_inf / inv_scale contract;
  * the per-element bound: an honest fp32 evaluation in the kernel's order (step32) stays inside it on every step of every configuration
    of the GPU test, and each fault of the table below - every one a plausible slip in dmx_adamw_kernel / dmx_clip_coef_kernel that the
    model-level tests cannot see (at step 1 Adam's update is lr * sign(g) whatever the betas and bias corrections are) - breaks it at some
    step >= 2.  The inputs are block 0 (2^20 elements) of the GPU test's: same generator, seed, steps, configurations (the GPU test zeroes
    the few row paddings among them, and its norm is the whole arena's; max_norm is a multiple of the norm in both); the state is carried
    by the honest evaluation and every variant starts each step from that state, as the GPU test restarts the reference from the
    kernel's own state."""
import math

import pytest
import torch

import adamw_restatement as A
import ema_restatement as E


def test_restatement_equals_torch_adamw_fp64():
    shapes = [(7, 5), (33,), (4, 3, 3, 3), (1,), (64, 9)]
    gen = torch.Generator().manual_seed(3)
    for max_norm, wd, decay in ((0.0, 0.0, None), (1e9, 1e-2, 0.0), (0.3, 1e-2, 0.9999), (0.3, 0.0, 0.5)):
        params = [torch.nn.Parameter(torch.randn(s, generator=gen, dtype=torch.float64) * 0.1) for s in shapes]
        opt = torch.optim.AdamW(params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=wd)
        flat = lambda ts: torch.cat([t.detach().reshape(-1) for t in ts])
        st = dict(p=flat(params).clone(), m=torch.zeros(flat(params).numel(), dtype=torch.float64), v=torch.zeros(flat(params).numel(), dtype=torch.float64), ema=None)
        shadows = None
        if decay is not None:
            shadows = [p.detach().clone() + 0.01 for p in params]
            st["ema"] = flat(shadows).clone()
        for t in range(1, 6):
            grads = [torch.randn(s, generator=gen, dtype=torch.float64) * 10.0 ** float(torch.randint(-4, 2, (1,), generator=gen)) for s in shapes]
            for p, g in zip(params, grads):
                p.grad = g.clone()
            norm_t = float(torch.nn.utils.clip_grad_norm_(params, max_norm)) if max_norm > 0 else float(flat(grads).norm())
            opt.step()
            if shadows is not None:
                E.step(shadows, params, decay)
            st, (norm, factor, found) = A.full_step64(st["p"], st["m"], st["v"], flat(grads), st["ema"], 1e-3, 0.9, 0.999, 1e-8, wd, t, max_norm, decay or 0.0)
            assert found == 0.0 and abs(norm - norm_t) <= 1e-12 * norm_t
            assert (factor == 1.0) == (max_norm == 0.0 or max_norm > norm)
            rel = lambda a, b: float((a - b).abs().max() / b.abs().max())
            assert rel(st["p"], flat(params)) <= 1e-12, f"step {t}: p"
            assert rel(st["m"], flat([opt.state[p]["exp_avg"] for p in params])) <= 1e-12, f"step {t}: exp_avg"
            assert rel(st["v"], flat([opt.state[p]["exp_avg_sq"] for p in params])) <= 1e-12, f"step {t}: exp_avg_sq"
            if shadows is not None:
                assert rel(st["ema"], flat(shadows)) <= 1e-12, f"step {t}: ema"


def test_inv_scale_and_found_inf_contract():
    gen = torch.Generator().manual_seed(5)
    n = 1000
    p, m, v = (torch.randn(n, generator=gen, dtype=torch.float64) for _ in range(3))
    v = v.abs(); e = p + 0.01
    g = torch.randn(n, generator=gen, dtype=torch.float64)
    a, sa = A.full_step64(p, m, v, g, e, 1e-3, 0.9, 0.999, 1e-8, 1e-2, 3, 0.5, 0.9999)
    b, sb = A.full_step64(p, m, v, g * 1024.0, e, 1e-3, 0.9, 0.999, 1e-8, 1e-2, 3, 0.5, 0.9999, inv_scale=1.0 / 1024.0)
    assert sa[0] == sb[0] and sb[1] == sa[1] / 1024.0 and sa[2] == sb[2] == 0.0          # the UNSCALED norm; powers of two: exact
    for k in "pmv":
        assert torch.equal(a[k], b[k])
    assert torch.equal(a["ema"], b["ema"])
    for bad in (float("inf"), float("-inf"), float("nan")):
        gb = g.clone(); gb[17] = bad
        c, sc = A.full_step64(p, m, v, gb, e, 1e-3, 0.9, 0.999, 1e-8, 1e-2, 3, 0.5, 0.9999, inv_scale=1.0 / 1024.0)
        assert sc[2] == 1.0 and all(c[k] is x for k, x in (("p", p), ("m", m), ("v", v), ("ema", e)))
    # no clipping when max_norm == 0, the coefficient exactly 1 when max_norm is above the norm
    assert A.clip_coef(3.0, 0.0) == 1.0 and A.clip_coef(3.0, 3.1) == 1.0 and abs(A.clip_coef(3.0, 0.15) - 0.15 / 3.000001) < 1e-15


@pytest.fixture(scope="module")
def trajectory():
    """the honest fp32 state before every step of every configuration, on block 0 of the GPU test's inputs"""
    n = A.BLOCK
    p0, e0 = A.gen_params(n)
    grads = {t: A.gen_grad(n, t) for t in A.STEPS}
    runs = {}
    for name, (mult, wd, decay, scale) in A.CONFIGS.items():
        hp = A.hyper(wd)
        st = dict(p=p0.clone(), m=torch.zeros(n), v=torch.zeros(n), ema=None if decay is None else e0.clone())
        steps = []
        for t in A.STEPS:
            inv_scale = 1.0 if scale is None else 1.0 / scale
            g = grads[t] if scale is None else grads[t] * scale                   # what the arena holds (a power of two: exact)
            norm_arena = A.grad_norm64(g)
            max_norm = A.f32(mult * norm_arena * inv_scale)
            restated = A.clip_coef(norm_arena * inv_scale, max_norm) * inv_scale
            dec = 0.0 if decay is None else A.f32(decay)
            steps.append(dict(t=t, pre=st, g=g, norm_arena=norm_arena, max_norm=max_norm, inv_scale=inv_scale, restated=restated, hp=hp, decay=dec))
            _, f = A.factor32(norm_arena, max_norm, inv_scale)
            st = A.step32(st["p"], st["m"], st["v"], g, st["ema"], f, hp["lr"], hp["b1"], hp["b2"], hp["eps"], hp["wd"], t, dec)
        runs[name] = steps
    return runs


def _ratios(s, fault):
    _, f = A.factor32(s["norm_arena"], s["max_norm"], s["inv_scale"], fault)
    hp = s["hp"]
    got = A.step32(s["pre"]["p"], s["pre"]["m"], s["pre"]["v"], s["g"], s["pre"]["ema"], f, hp["lr"], hp["b1"], hp["b2"], hp["eps"], hp["wd"], s["t"], s["decay"], fault)
    r, _, _ = A.check_step(got, s["pre"], s["g"], f, s["restated"], hp, s["t"], s["decay"])
    r["coef"] = (abs(f - s["restated"]) / (A.COEF_TOL * s["restated"]), 0)
    return r


def test_honest_fp32_stays_inside_the_bound(trajectory):
    for name, steps in trajectory.items():
        for s in steps:
            r = _ratios(s, None)
            print(f"{name} t={s['t']}: " + " ".join(f"{k} {v[0]:.3f}" for k, v in r.items()))
            for k, (ratio, i) in r.items():
                assert ratio <= 1.0, f"{name} step {s['t']}: honest fp32 {k} is {ratio:.3f} x its bound at element {i}"
            if A.CONFIGS[name][0] > 1.0:
                assert A.factor32(s["norm_arena"], s["max_norm"], s["inv_scale"])[1] == 1.0


@pytest.mark.parametrize("fault", A.FAULTS)
def test_injected_kernel_faults_are_caught(trajectory, fault):
    """every fault breaks a PER-ELEMENT bound (p, m, v, ema, or m around the restated coefficient) at some step >= 2"""
    caught = []
    for name, steps in trajectory.items():
        for s in steps:
            if s["t"] < 2:
                continue
            r = _ratios(s, fault)
            bad = {k: v for k, v in r.items() if k != "coef" and v[0] > 1.0}
            if bad:
                k = max(bad, key=lambda q: bad[q][0])
                caught.append(f"{name} t={s['t']}: {k} {bad[k][0]:.3g} x bound")
    print(f"{fault}: " + "; ".join(caught))
    assert caught, f"{fault}: no per-element bound broken at any step >= 2"
