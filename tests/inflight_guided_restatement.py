"""Test-local numpy restatement of the per-row guided scheduler step of the in-flight engine (include/diffute_hip.h
dmx_sched_step_rows_guided): fp32, one engine row at a time.  Nothing is written anew: a row's update is
tests/inflight_restatement.row_update, the classifier-free combination and the rescale ratio are tests/guidance_restatement.combine /
ratios, and the rescale expression is the one line of guidance_restatement._eval.

  idle row (row_index < 0)   untouched, whatever its guide entry says
  PLAIN                      row_update on the row's own record
  UNCOND                     nothing: its sample row is written by its partner, its noise / history slices are nobody's
  COND with partner p        e = the guided model output of (eps[b], eps[p]) with the row's OWN scale / rescale; row_update on the row's own
                             record, noise[b], hist[.][b]; the result goes to sample[b] and sample[p]
  a row that cannot be served (see `served`) is left alone

`fault` injects the mistakes such a kernel can make, so that the host test can show the comparisons would see each of them:
  "neighbour_scale"     a pair takes the scale / rescale of the next running pair
  "uncond_own_record"   the unconditional row is updated by its own record (as if PLAIN)
  "partner_history"     the history slices of the partner row are used
  "idle_cond"           an idle row whose guide entry says COND is updated (with record 0)
  "second_store"        the store to the partner's sample row is dropped
"""
import collections

import numpy as np

import guidance_restatement as G
import inflight_restatement as IR

f32 = np.float32
PLAIN, COND, UNCOND = 0, 1, 2
FAULTS = ("neighbour_scale", "uncond_own_record", "partner_history", "idle_cond", "second_store")
Row = collections.namedtuple("Row", "role partner scale rescale one_minus_rescale", defaults=(PLAIN, 0, 0.0, 0.0, 0.0))      # (PLAIN: the all-zero entry)


def pair(b, p, scale, rescale=0.0):
    """the two guide entries of the pair (b conditional, p unconditional), as dmx_rows_guide writes them"""
    omr = float(f32(1 - rescale))
    return Row(COND, p, scale, rescale, omr), Row(UNCOND, b, scale, rescale, omr)


def ring_ok(kind, rec, n_hist):
    if kind != IR.DPMPP:
        return True
    o = rec.order
    return (1 <= o <= min(n_hist, 3) and 0 <= rec.ring_w < n_hist and (o < 2 or (0 <= rec.ring_m1 < n_hist and rec.ring_m1 != rec.ring_w))
            and (o < 3 or (0 <= rec.ring_m2 < n_hist and rec.ring_m2 != rec.ring_w)))


def served(b, row_index, guide):
    """whether the COND row b names a partner the step can serve"""
    B, p = len(row_index), guide[b].partner
    return 0 <= p < B and p != b and row_index[p] == row_index[b] and guide[p].role == UNCOND and guide[p].partner == b


def step_rows_guided(kind, sample, eps, noise, hist, plan, row_index, guide, vpred=False, fault=None, k=None):
    """sample / eps / noise [B, per], hist [n_hist, B, per] (or None), plan a list of records, row_index B ints, guide B entries with
    .role .partner .scale .rescale .one_minus_rescale; k: the ratios to use per row (None: the restatement's own)
    -> (sample', hist', ratios [B], NaN where none was taken) as new arrays"""
    out = sample.copy()
    h = None if hist is None else hist.copy()
    B = sample.shape[0]
    n_hist = 0 if hist is None else hist.shape[0]
    ratio = np.full(B, np.nan, f32)
    running = [b for b in range(B) if row_index[b] >= 0 and guide[b].role == COND]
    for b in range(B):
        idx, g = row_index[b], guide[b]
        forced = False
        if idx < 0:
            if not (fault == "idle_cond" and g.role == COND):
                continue
            if not 0 <= g.partner < B:
                continue
            idx, forced = 0, True
        role = g.role
        if role == UNCOND and fault == "uncond_own_record":
            role = PLAIN
        if role not in (PLAIN, COND):
            continue
        if role == COND and not forced and not served(b, row_index, guide):
            continue
        rec = plan[idx]
        if not ring_ok(kind, rec, n_hist):
            continue
        p, hb = g.partner, b
        if role == PLAIN:
            e = eps[b]
        else:
            s = g
            if fault == "neighbour_scale" and len(running) > 1 and b in running:
                s = guide[running[(running.index(b) + 1) % len(running)]]
            ec, eu = eps[b:b + 1].astype(f32), eps[p:p + 1].astype(f32)
            gm = G.combine(ec, eu, s.scale, f32)
            e = gm[0]
            if s.rescale != 0:
                ratio[b] = G.ratios(ec, gm, f32)[0] if k is None else f32(k[b])
                e = (f32(s.rescale) * (gm * ratio[b]) + f32(s.one_minus_rescale) * gm).astype(f32)[0]      # (guidance_restatement._eval)
            if fault == "partner_history":
                hb = p
        m1 = hist[rec.ring_m1, hb] if kind == IR.DPMPP and rec.order >= 2 else None
        m2 = hist[rec.ring_m2, hb] if kind == IR.DPMPP and rec.order >= 3 else None
        prev, m0 = IR.row_update(kind, rec, sample[b], e, None if noise is None else noise[b], m1, m2, vpred)
        out[b] = prev
        if role == COND and fault != "second_store":
            out[p] = prev
        if m0 is not None:
            h[rec.ring_w, hb] = m0
    return out, h, ratio
