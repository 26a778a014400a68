"""Test-local numpy restatement of the per-row scheduler update of the in-flight engine (dmx_sched_step_rows): fp32, one row at a
time, each row with the record its row_index names, idle rows (-1) and their history slices untouched.  The arithmetic is written in the
op order of diffusers' step() (as oracle/schedulers.py and tests/dpm_restatement.py write it), on the record's scalars.

`fault` injects one of three mistakes a per-row kernel can make, so the host test can show that the comparison would see them:
  "idle_updated"   an idle row is updated (with record 0)
  "neighbour_rec"  a row uses the record of the next active row
  "ring_next"      the DPM-Solver++ history-ring positions of step i + 1
"""
import numpy as np

f32 = np.float32
DDIM, DDPM, DPMPP = 0, 1, 2


def _x0(x, e, s_eps, s_x, vpred):
    return s_x * x - s_eps * e if vpred else (x - s_eps * e) / s_x


def row_update(kind, rec, x, e, nz, m1, m2, vpred):
    """one row: -> (prev_sample, m0 or None)"""
    x, e = x.astype(f32), e.astype(f32)
    if kind == DPMPP:
        d = rec.dpm
        m0 = _x0(x, e, f32(d.sigma_s0), f32(d.alpha_s0), vpred)
        prev = f32(d.c_x) * x - f32(d.c_m0) * m0
        if rec.order == 2:
            prev = prev + f32(d.c_d1) * (f32(d.inv_r0) * (m0 - m1))
        elif rec.order == 3:
            d10, d11 = f32(d.inv_r0) * (m0 - m1), f32(d.inv_r1) * (m1 - m2)
            dd = d10 - d11
            prev = (prev + f32(d.c_d1) * (d10 + f32(d.r0_over_r01) * dd)) - f32(d.c_d2) * (f32(d.inv_r01) * dd)
        return prev.astype(f32), m0.astype(f32)
    c = [f32(v) for v in rec.c]
    x0 = _x0(x, e, c[0], c[1], vpred)
    if kind == DDIM:
        pe = c[1] * e + c[0] * x if vpred else e
        prev = c[2] * x0 + c[3] * pe
    else:
        prev = c[2] * x0 + c[3] * x
    if rec.use_noise and nz is not None:
        prev = prev + c[4] * nz.astype(f32)
    return prev.astype(f32), None


def step_rows(kind, sample, eps, noise, hist, plan, row_index, vpred=False, fault=None):
    """sample / eps / noise [B, per], hist [n_hist, B, per] (or None), plan a list of records, row_index B ints -> (sample', hist') as
    new arrays"""
    out = sample.copy()
    h = None if hist is None else hist.copy()
    B = sample.shape[0]
    k = 0 if hist is None else hist.shape[0]
    active = [b for b in range(B) if row_index[b] >= 0]
    for b in range(B):
        idx = row_index[b]
        if idx < 0:
            if fault != "idle_updated":
                continue
            idx = 0
        if fault == "neighbour_rec" and len(active) > 1 and b in active:
            idx = row_index[active[(active.index(b) + 1) % len(active)]]
        rec = plan[idx]
        w, i1, i2 = rec.ring_w, rec.ring_m1, rec.ring_m2
        if fault == "ring_next" and k:
            w, i1, i2 = (w + 1) % k, (i1 + 1) % k, (i2 + 1) % k
        m1 = hist[i1, b] if kind == DPMPP and rec.order >= 2 else None
        m2 = hist[i2, b] if kind == DPMPP and rec.order >= 3 else None
        prev, m0 = row_update(kind, rec, sample[b], eps[b], None if noise is None else noise[b], m1, m2, vpred)
        out[b] = prev
        if m0 is not None:
            h[w, b] = m0
    return out, h
