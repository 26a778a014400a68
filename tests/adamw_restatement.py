"""Plain restatement of the fused AdamW step (csrc/optim.hip) in arena space: flat vectors p, m, v[, ema] and g, no parameter
structure.  Three things live here, shared by test_adamw_host.py (CPU) and test_adamw_gpu.py:

  * `step64` - ONE optimizer step in fp64: torch.optim.AdamW's single-tensor formulas after torch.nn.utils.clip_grad_norm_
    (clip = min(1, max_norm / (norm + 1e-6)), no clipping when max_norm == 0), GradScaler's contract (the arena holds g / inv_scale, the
    norm, the clipping and the update use g * inv_scale, a non-finite gradient skips the step as a whole: found_inf) and diffusers'
    EMAModel.step  s -= (1 - decay) * (s - p_new);
  * `bounds` - the per-element rounding bound of the kernel's fp32 evaluation of the same expressions (derivation below);
  * `step32` - the kernel's expression order in fp32, one rounding per operation, with the faults test_adamw_host.py injects.

The inputs of the GPU test (`gen_params`, `gen_grad`, `CONFIGS`, `STEPS`) are defined here so that the CPU test runs on the same ones.

Rounding bound.  The Makefile compiles with -ffp-contract=off (no fused multiply-add: every `*`, `+`, `-` of dmx_adamw_kernel rounds
once) and without fast-math or -fno-hip-fp32-correctly-rounded-divide-sqrt, so `/` and sqrtf are correctly rounded too: every operation
contributes one relative error of at most u = 2^-24 (half an ulp).  For an expression without cancellation inside a divisor the
computed value differs from the exact one by at most gamma_c = c u / (1 - c u) times the expression evaluated with the magnitudes of
its terms, c being the number of rounded operations on the longest path (the host's fp32 roundings of bc1, sqrt(bc2) and 1 - decay
count as operations; sqrt halves what it is handed, counted in full here).  With f = scalars[1] (the kernel's own factor, an input):
    gr = g * f                                                             1
    m' = m * b1 + gr * (1 - b1)                     5 = gr, m*b1, 1-b1, gr*(1-b1), +           terms |m b1| + |gr (1-b1)|
    v' = v * b2 + gr * gr * (1 - b2)                7 = gr twice, gr*gr, 1-b2, *, v*b2, +      terms v b2 + gr^2 (1-b2)
    denom = sqrtf(v') / sqrt(bc2) + eps             11 = v' (7), sqrtf, (float)sqrt(bc2), /, +
    U = (lr / bc1) * (m' / denom)                   20 = m' (5), denom (11), (float)bc1, lr/bc1, m'/denom, *
    p' = p * (1 - lr * wd) - U                      24 = U (20), lr*wd, 1 - lr*wd, p * (..), -
                                                    terms |p (1 - lr wd)| + (lr / bc1) (|m b1| + |gr (1-b1)|) / denom
    e' = e - (1 - decay) * (e - p')                 4 = 1-decay, e-p', *, -  on |e| + (1-decay)(|e| + |p'|), plus (1-decay) * bound(p')
                                                    (the kernel subtracts ITS p', the restatement the exact one)
(the two branches of p' are added, not maximised: simpler, and no tighter bound is needed to tell the faults of test_adamw_host.py apart).
"""
import math

import numpy as np
import torch

U = 2.0 ** -24
C_M, C_V, C_P, C_E = 5, 7, 24, 4
SEED = 20240611
STEPS = (1, 2, 3, 1000)
LR, BETAS, EPS = 1e-3, (0.9, 0.999), 1e-8
# name -> (max_norm as a multiple of the step's gradient norm; 0 = off, weight_decay, ema_decay or None, loss scale)
CONFIGS = {
    "plain": (0.0, 0.0, None, None),
    "noclip_wd_ema0": (2.0, 1e-2, 0.0, None),            # max_norm above the norm: the coefficient must be exactly 1
    "clip_wd_ema": (0.05, 1e-2, 0.9999, None),
    "scaled_clip_wd_ema": (0.05, 1e-2, 0.9999, 1024.0),
}


def f32(x):
    """the value a C float argument receives"""
    return float(torch.tensor(x, dtype=torch.float32))


def gamma(c):
    return c * U / (1.0 - c * U)


BLOCK = 1 << 20      # the inputs are generated in blocks of 2^20 elements, each from its own seed: the CPU test runs on block 0 alone


def _blocks(n, seed, fn):
    return torch.cat([fn(min(BLOCK, n - lo), torch.Generator().manual_seed(seed + 104729 * (lo // BLOCK))) for lo in range(0, n, BLOCK)])


def gen_params(n, seed=SEED):
    """master parameters and EMA shadow of n arena elements: N(0, 0.05^2), 3 % exact zeros, 1 % ones (biases and norm weights)"""
    def one(k, g):
        p = torch.randn(k, generator=g) * 0.05
        r = torch.rand(k, generator=g)
        p[r < 0.03] = 0.0
        p[r > 0.99] = 1.0
        return torch.stack([p, p + torch.randn(k, generator=g) * 1e-3])
    pe = torch.cat([one(min(BLOCK, n - lo), torch.Generator().manual_seed(seed + 104729 * (lo // BLOCK))) for lo in range(0, n, BLOCK)], 1)
    return pe[0].contiguous(), pe[1].contiguous()


def gen_grad(n, step, seed=SEED):
    """a gradient for optimizer step `step`: magnitudes log-uniform over 1e-8 .. 1e2, random signs, about 1 % exact zeros"""
    def one(k, g):
        mag = torch.pow(10.0, torch.rand(k, generator=g, dtype=torch.float64) * 10.0 - 8.0).to(torch.float32)
        r = torch.rand(k, generator=g)
        out = torch.where(r < 0.5, mag, -mag)
        out[r > 0.99] = 0.0
        return out
    return _blocks(n, seed + 7919 * step, one)


def grad_norm64(g, inv_scale=1.0):
    """fp64 norm of the unscaled gradient g * inv_scale"""
    return float(g.double().pow(2).sum().sqrt()) * inv_scale


def clip_coef(norm, max_norm):
    """torch.nn.utils.clip_grad_norm_: the factor the gradients are multiplied by"""
    if not max_norm > 0.0:
        return 1.0
    return min(1.0, max_norm / (norm + 1e-6))


def bias_corrections(b1, b2, t):
    return 1.0 - b1 ** t, 1.0 - b2 ** t


def step64(p, m, v, g, ema, factor, lr, b1, b2, eps, wd, t, ema_decay=0.0):
    """one step in fp64 from fp64 tensors; `factor` multiplies g (clip coefficient * inv_scale).  Returns the new (p, m, v, ema) and the
    magnitude sums the bounds are stated on."""
    bc1, bc2 = bias_corrections(b1, b2, t)
    gr = g * factor
    a, b = m * b1, gr * (1.0 - b1)
    m2 = a + b
    sm = a.abs() + b.abs()
    v2 = v * b2 + gr * gr * (1.0 - b2)
    denom = v2.sqrt() / math.sqrt(bc2) + eps
    pd = p * (1.0 - lr * wd)
    p2 = pd - (lr / bc1) * (m2 / denom)
    mags = dict(m=sm, v=v2, p=pd.abs() + (lr / bc1) * sm / denom)
    e2 = None
    if ema is not None:
        omd = 1.0 - ema_decay
        e2 = ema - omd * (ema - p2)
        mags["ema"] = ema.abs() + omd * (ema.abs() + p2.abs())
        mags["omd"] = omd
    return dict(p=p2, m=m2, v=v2, ema=e2), mags


def bounds(mags):
    """per-element absolute bounds of the kernel's fp32 results around step64's"""
    out = dict(m=gamma(C_M) * mags["m"], v=gamma(C_V) * mags["v"], p=gamma(C_P) * mags["p"])
    if "ema" in mags:
        out["ema"] = gamma(C_E) * mags["ema"] + mags["omd"] * out["p"]
    return out


def full_step64(p, m, v, g, ema, lr, b1, b2, eps, wd, t, max_norm, ema_decay=0.0, inv_scale=1.0):
    """the whole contract: -> (state, scalars = (norm, factor, found_inf)); a non-finite gradient leaves the state as it was"""
    if not bool(torch.isfinite(g).all()):
        return dict(p=p, m=m, v=v, ema=ema), (float("nan"), float("nan"), 1.0)
    norm = grad_norm64(g, inv_scale)
    factor = clip_coef(norm, max_norm) * inv_scale
    new, _ = step64(p, m, v, g, ema, factor, lr, b1, b2, eps, wd, t, ema_decay)
    return new, (norm, factor, 0.0)


FAULTS = ("betas_swapped", "bc2_for_sqrt_bc2", "eps_inside_root", "decay_after_update", "clip_from_scaled_norm", "bc1_dropped", "ema_reads_old_p")


def factor32(norm, max_norm, inv_scale, fault=None):
    """dmx_clip_coef_kernel's last lines in fp32 from the (fp64-accurate) norm of the ARENA's gradient: -> (scalars[0], scalars[1])"""
    t = lambda x: torch.tensor(x, dtype=torch.float32)
    nrm = t(norm) * t(inv_scale)
    c = t(1.0)
    if max_norm > 0.0:
        c = t(max_norm) / ((t(norm) if fault == "clip_from_scaled_norm" else nrm) + t(1e-6))
        c = torch.minimum(c, t(1.0))
    return float(nrm), float(c * t(inv_scale))


def sqrt32(x):
    """correctly rounded fp32 square root: numpy's on the CPU (torch's vectorised CPU sqrt is not: it is off by an ulp in ~0.7 % of the
    elements), torch's on the device"""
    return torch.sqrt(x) if x.is_cuda else torch.from_numpy(np.sqrt(x.numpy()))


def step32(p, m, v, g, ema, factor, lr, b1, b2, eps, wd, t, ema_decay=0.0, fault=None):
    """dmx_adamw_kernel's expression in its order, every operation rounded to fp32 (torch CPU / eager ops: one IEEE operation each, no
    contraction).  Scalars are fp32 tensors; bc1 and sqrt(bc2) are computed in double from the fp32 betas and rounded, as the host does."""
    dev = p.device
    s = lambda x: torch.tensor(x, dtype=torch.float32, device=dev)
    lr_, b1_, b2_, eps_, wd_, f_ = s(lr), s(b1), s(b2), s(eps), s(wd), s(factor)
    bc1, bc2 = bias_corrections(f32(b1), f32(b2), t)
    bc1_, bc2s_ = s(bc1), s(math.sqrt(bc2))
    if fault == "bc2_for_sqrt_bc2":
        bc2s_ = s(bc2)
    if fault == "betas_swapped":
        b1_, b2_ = b2_, b1_
    one = s(1.0)
    step_size = lr_ if fault == "bc1_dropped" else lr_ / bc1_
    decay = one - lr_ * wd_
    gr = g * f_
    pv = p if fault == "decay_after_update" else p * decay
    mv = m * b1_ + gr * (one - b1_)
    vv = v * b2_ + gr * gr * (one - b2_)
    denom = sqrt32(vv + eps_) / bc2s_ if fault == "eps_inside_root" else sqrt32(vv) / bc2s_ + eps_
    pv = pv - step_size * (mv / denom)
    if fault == "decay_after_update":
        pv = pv * decay
    e2 = None
    if ema is not None:
        omd = one - s(ema_decay)
        e2 = ema - omd * (ema - (p if fault == "ema_reads_old_p" else pv))
    return dict(p=pv, m=mv, v=vv, ema=e2)


def worst_ratios(got, ref, bnd):
    """-> {quantity: (max over elements of |got - ref| / bound, flat index)}; an element with a zero bound must be exact (ratio 0 or inf)"""
    out = {}
    for k in ("p", "m", "v", "ema"):
        if ref.get(k) is None:
            continue
        err = (got[k].double() - ref[k]).abs()
        r = torch.where(err == 0, torch.zeros_like(err), err / bnd[k])
        i = int(r.argmax())
        out[k] = (float(r[i]), i)
    return out


COEF_TOL = 1e-5      # the project's bar for the norm and the coefficient (scalars[0], scalars[1]) against fp64


def check_step(got, pre, g, factor_used, factor_restated, hp, t, ema_decay):
    """The per-element check of one step, the same on the CPU (step32 and its faults) and on the GPU (the kernel): `got` and `pre` are dicts
    of fp32 tensors (p, m, v, ema or None) after and before the step, `g` the gradient as the arena holds it, `factor_used` the factor the
    implementation multiplied it by (its scalars[1]) and `factor_restated` the fp64 one.  p, m, v, ema are held to `bounds` around step64
    fed with factor_used; m is held a second time around step64 fed with factor_restated, with COEF_TOL of the gradient term added - so a
    wrong coefficient shows per element too.  -> ({quantity: (worst |error| / bound, flat index)}, step64's state, the bounds); every ratio must be <= 1."""
    d = lambda x: None if x is None else x.double()
    ref, mags = step64(d(pre["p"]), d(pre["m"]), d(pre["v"]), d(g), d(pre.get("ema")), factor_used, hp["lr"], hp["b1"], hp["b2"], hp["eps"], hp["wd"], t, ema_decay)
    bnd_all = bounds(mags)
    out = worst_ratios(got, ref, bnd_all)
    gr = d(g) * factor_restated
    a, b = d(pre["m"]) * hp["b1"], gr * (1.0 - hp["b1"])
    err = (got["m"].double() - (a + b)).abs()
    bnd = gamma(C_M) * (a.abs() + b.abs()) + COEF_TOL * b.abs()
    r = torch.where(err == 0, torch.zeros_like(err), err / bnd)
    i = int(r.argmax())
    out["m_restated_factor"] = (float(r[i]), i)
    return out, ref, bnd_all


def hyper(wd):
    """the hyper-parameters as the C entry receives them (fp32 values, held as Python floats)"""
    return dict(lr=f32(LR), b1=f32(BETAS[0]), b2=f32(BETAS[1]), eps=f32(EPS), wd=f32(wd))
