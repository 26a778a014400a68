"""Test-local numpy restatement of the guided scheduler step (include/diffute_hip.h dmx_sched_step_guided): classifier-free guidance,
the guidance rescale of Lin et al. 2023 (diffusers' rescale_noise_cfg) and the scheduler update, per sample.  diffusers is not needed: the
formulas are written out from the header,

    g = eu + scale * (ec - eu)
    rescale == 0:  e = g          else  e = rescale * (g * k_b) + (1 - rescale) * g,   k_b = std_b(ec) / std_b(g)  (unbiased, per sample)

one rounding per op in that order, and the update on (x, e) is tests/inflight_restatement.row_update - the restatement the scalar and the
per-row scheduler kernels are already held to - so no scheduler arithmetic is written again here.

  eval32   numpy float32 throughout; the ratio k [B] is an ARGUMENT (None: its own fp32 ratio, mean first, then the centred squares)
  ref64    the same in float64 (row_update evaluated in float64 as well: the record's scalars are fp32 values either way)

`fault` injects the mistakes a guided kernel can make, so that the host test can show the comparisons would see each of them:
  "swap_halves"       the conditional and the unconditional half of the model output exchanged
  "scale_on_ec"       scale * ec - eu  in place of  scale * (ec - eu)
  "ratio_inverted"    k = std(g) / std(ec)
  "rescale_swapped"   rescale and 1 - rescale exchanged
  "mixed_bias"        std(ec) biased (/ n), std(g) unbiased (/ (n - 1))
  "batch_std"         the deviations over the whole batch instead of per sample
  "second_half"       rows [B, 2B) of the sample not written
"""
import contextlib

import numpy as np

import inflight_restatement as IR

f32, f64 = np.float32, np.float64
DDIM, DDPM, DPMPP = IR.DDIM, IR.DDPM, IR.DPMPP
FAULTS = ("swap_halves", "scale_on_ec", "ratio_inverted", "rescale_swapped", "mixed_bias", "batch_std", "second_half")


@contextlib.contextmanager
def _row_update_dtype(dt):
    """inflight_restatement.row_update casts through its module-level f32: float64 evaluates the same expressions in float64"""
    old = IR.f32
    IR.f32 = dt
    try:
        yield
    finally:
        IR.f32 = old


def combine(ec, eu, scale, dt, fault=None):
    s = dt(scale)
    if fault == "scale_on_ec":
        return (eu + (s * ec - eu)).astype(dt)
    return (eu + s * (ec - eu)).astype(dt)


def _std(v, dt, ddof=1):
    """mean first, then the centred squares; never E[x^2] - E[x]^2"""
    v = v.reshape(-1)
    n = v.size
    mean = v.sum(dtype=dt) / dt(n)
    d = v - mean
    return np.sqrt((d * d).sum(dtype=dt) / dt(n - ddof))


def ratios(ec, g, dt, fault=None):
    """k [B] for ec / g [B, per]"""
    B = ec.shape[0]
    if fault == "batch_std":
        return np.full(B, _std(ec, dt) / _std(g, dt), dtype=dt)
    k = np.empty(B, dtype=dt)
    for b in range(B):
        sc, sg = _std(ec[b], dt, 0 if fault == "mixed_bias" else 1), _std(g[b], dt)
        k[b] = sg / sc if fault == "ratio_inverted" else sc / sg
    return k


def _eval(dt, kind, rec, sample, eps, noise, hist, scale, rescale, vpred, k, fault):
    B = sample.shape[0] // 2
    sample, eps = sample.astype(dt), eps.astype(dt)
    ec, eu = (eps[B:], eps[:B]) if fault == "swap_halves" else (eps[:B], eps[B:])
    g = combine(ec, eu, scale, dt, fault)
    e, used = g, None
    if rescale != 0:
        used = ratios(ec, g, dt, fault) if k is None else np.asarray(k, dtype=dt)
        r, omr = (dt(f32(1 - rescale)), dt(f32(rescale))) if fault == "rescale_swapped" else (dt(f32(rescale)), dt(f32(1 - rescale)))
        e = (r * (g * used.reshape(B, 1)) + omr * g).astype(dt)
    out = sample.copy()
    h = None if hist is None else hist.astype(dt)
    with _row_update_dtype(dt):
        for b in range(B):
            m1 = h[rec.ring_m1, b].copy() if kind == DPMPP and rec.order >= 2 else None
            m2 = h[rec.ring_m2, b].copy() if kind == DPMPP and rec.order >= 3 else None
            prev, m0 = IR.row_update(kind, rec, sample[b], e[b], None if noise is None else noise[b].astype(dt), m1, m2, vpred)
            out[b] = prev
            if fault != "second_half":
                out[B + b] = prev
            if m0 is not None:
                h[rec.ring_w, b] = m0
    return out, h, used


def eval32(kind, rec, sample, eps, noise, hist, scale, rescale, vpred=False, k=None, fault=None):
    """sample / eps [2B, per], noise [B, per] or None (added when given AND the record asks for it: set rec.use_noise), hist
    [n_hist, B, per] or None -> (sample' [2B, per], hist', the ratios used [B] or None), float32"""
    return _eval(f32, kind, rec, sample, eps, noise, hist, scale, rescale, vpred, k, fault)


def ref64(kind, rec, sample, eps, noise, hist, scale, rescale, vpred=False, k=None, fault=None):
    return _eval(f64, kind, rec, sample, eps, noise, hist, scale, rescale, vpred, k, fault)


# ------------------------------------------------------------------------------------------------ the cases both test files run
PER_SAMPLE = (2, 5, 255, 256, 257, 1024, 1027, 4099, 16384)
BATCHES = (1, 3)
SCALES = (0.8, 3.0, 7.5)
RESCALES = (0.3, 1.0)


def inputs(B, per, seed=0):
    """sample, eps [2B, per], noise [B, per], hist [3, B, per] as float32: normal draws plus an offset, the unconditional half correlated
    with the conditional one, every row's deviation far from zero (and different from row to row, so that a batch-wide deviation shows)"""
    rng = np.random.default_rng([seed, B, per])
    amp = (1.0 + 0.5 * np.arange(B)).reshape(B, 1)
    ec = 0.3 + amp * rng.standard_normal((B, per))
    eu = 0.1 + 0.8 * ec + 0.35 * rng.standard_normal((B, per))
    x = rng.standard_normal((B, per)) * 1.2 - 0.1
    sample = np.concatenate([x, x], 0)
    return (sample.astype(f32), np.concatenate([ec, eu], 0).astype(f32), rng.standard_normal((B, per)).astype(f32),
            (0.7 * rng.standard_normal((3, B, per))).astype(f32))


def case_key(B, per, scale):
    return f"{per}/{B}/{scale:g}"


def ratio_floor(B, per, scale):
    """relative error of eval32's own ratio against ref64's, per sample, on inputs(B, per)"""
    _, eps, _, _ = inputs(B, per)
    k32 = ratios(eps[:B], combine(eps[:B], eps[B:], scale, f32), f32)
    e64 = eps.astype(f64)
    k64 = ratios(e64[:B], combine(e64[:B], e64[B:], scale, f64), f64)
    return [float(abs(f64(a) - b) / abs(b)) for a, b in zip(k32, k64)]


def bound(floor):
    """the GPU test's relative bound on ratio_out against ref64's ratio: 4 x the recorded error of the fp32 formulation for the case
    plus 2^-22 - the margin tests/test_metrics_gpu.py gives the SSIM: another valid summation order (the kernel's strided partials and
    tree against numpy's pairwise sum) moves the result by about the formulation's own error"""
    return 4.0 * floor + 2.0 ** -22


if __name__ == "__main__":
    print('"""Measured relative error of the fp32 formulation of the rescale ratio std_b(ec) / std_b(g) (guidance_restatement.eval32\'s own ratio)')
    print("against float64 (ref64), per case \"per_sample/B/scale\" and sample, on guidance_restatement.inputs: the bound of test_guidance_gpu.py is")
    print("guidance_restatement.bound(floor); test_guidance_host.py measures the figures again.")
    print('Regenerate: python tests/guidance_restatement.py > tests/guidance_floors.py"""')
    print("FLOORS = {")
    for per in PER_SAMPLE:
        for B in BATCHES:
            for s in SCALES:
                print(f'    "{case_key(B, per, s)}": [' + ", ".join(f"{v:.3e}" for v in ratio_floor(B, per, s)) + "],")
    print("}")
