"""CPU-side checks of in-flight batching with classifier-free guidance (diffute_amd/inflight.py DenoiseEngine.submit(guidance=),
include/diffute_hip.h dmx_sched_step_rows_guided / dmx_rows_guide): the numpy restatement of the per-row guided step
(tests/inflight_guided_restatement.py) against the two restatements it is composed from - all rows PLAIN is inflight_restatement.step_rows,
one pair filling the batch is guidance_restatement.eval32 -, a staggered chain of two guided pairs and a plain row against each request
run alone, five injected faults that must each break an equality, and the layout of the guide table the host relies on."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest
import torch

import guidance_restatement as G
import inflight_guided_restatement as GR
import inflight_restatement as IR


def _same(a, b):
    """bit equality (NaN poison included)"""
    a, b = np.ascontiguousarray(a, dtype=np.float32), np.ascontiguousarray(b, dtype=np.float32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def _plans():
    import diffute_amd as D
    from diffute_amd.inflight import plan_records
    _, ddim = plan_records(D.DDIMScheduler(), 10, eta=0.5)
    _, ddpm = plan_records(D.DDPMScheduler(), 10)
    _, dpm = plan_records(D.DPMSolverMultistepScheduler(solver_order=3), 10)
    return {IR.DDIM: ddim, IR.DDPM: ddpm, IR.DPMPP: dpm}


# ------------------------------------------------------------------------------------------------ the two restatements it is made of
@pytest.mark.parametrize("kind", [IR.DDIM, IR.DDPM, IR.DPMPP])
def test_all_plain_rows_are_step_rows(kind):
    plan = _plans()[kind]
    rng = np.random.default_rng(kind)
    B, per = 4, 37
    x, e, nz = (rng.standard_normal((B, per)).astype(np.float32) for _ in range(3))
    hist = rng.standard_normal((3, B, per)).astype(np.float32) if kind == IR.DPMPP else None
    noise = None if kind == IR.DPMPP else nz
    idx = [2, -1, 7, 9]                                    # DPM-Solver++ orders 3, -, 3, 1
    guide = [GR.Row()] * B
    for vpred in (False, True):
        want = IR.step_rows(kind, x, e, noise, hist, plan, idx, vpred)
        got = GR.step_rows_guided(kind, x, e, noise, hist, plan, idx, guide, vpred)
        assert _same(got[0], want[0]) and (hist is None or _same(got[1], want[1])) and np.isnan(got[2]).all()
        # an idle row whose entry says COND stays idle; a role outside the enum leaves its row alone
        odd = [GR.Row(), GR.Row(GR.COND, 0, 3.0, 0.0, 1.0), GR.Row(7), GR.Row()]
        got = GR.step_rows_guided(kind, x, e, noise, hist, plan, idx, odd, vpred)
        assert _same(got[0][[0, 1, 3]], want[0][[0, 1, 3]]) and _same(got[0][2], x[2])


@pytest.mark.parametrize("B", [1, 2])
@pytest.mark.parametrize("kind", [IR.DDIM, IR.DDPM, IR.DPMPP])
def test_a_pair_filling_the_batch_is_eval32(kind, B):
    """rows [0, B) COND with partner b + B, rows [B, 2B) UNCOND: guidance_restatement.eval32 on the same arrays, sample, ring and ratios"""
    plan = _plans()[kind]
    per = 257
    x, eps, nz, hist = G.inputs(B, per)
    x[B:] = np.nan                                         # the unconditional sample rows are write-only
    for i, vpred, scale, rescale in ((2, False, 7.5, 0.7), (9, True, 3.0, 0.0), (1, False, 0.8, 1.0)):
        rec = plan[i]
        guide = [GR.pair(b, b + B, scale, rescale)[0] for b in range(B)] + [GR.pair(b, b + B, scale, rescale)[1] for b in range(B)]
        noise2 = None if kind == IR.DPMPP else np.concatenate([nz, np.full_like(nz, np.nan)], 0)
        hist2 = np.concatenate([hist, np.full_like(hist, np.nan)], 1) if kind == IR.DPMPP else None
        got_x, got_h, got_k = GR.step_rows_guided(kind, x, eps, noise2, hist2, plan, [i] * (2 * B), guide, vpred)
        want_x, want_h, want_k = G.eval32(kind, rec, x, eps, None if kind == IR.DPMPP else nz, hist if kind == IR.DPMPP else None, scale, rescale, vpred)
        assert _same(got_x, want_x), (kind, i)
        if kind == IR.DPMPP:
            assert _same(got_h[:, :B], want_h) and _same(got_h[:, B:], hist2[:, B:])
        assert (rescale == 0 and np.isnan(got_k).all()) or (_same(got_k[:B], want_k) and np.isnan(got_k[B:]).all())


def test_rows_that_cannot_be_served_are_left_alone():
    plan = _plans()[IR.DPMPP]
    rng = np.random.default_rng(3)
    B, per = 6, 19
    x, e = (rng.standard_normal((B, per)).astype(np.float32) for _ in range(2))
    hist = rng.standard_normal((3, B, per)).astype(np.float32)
    c, u = GR.pair(0, 1, 3.0, 0.5)
    good = GR.step_rows_guided(IR.DPMPP, x, e, None, hist, plan, [2] * B, [c, u] + [GR.Row()] * 4)
    cases = {
        "partner past the batch": ([GR.Row(GR.COND, 6, 3.0), GR.Row(GR.UNCOND, 2)], [2, 2]),
        "partner negative": ([GR.Row(GR.COND, -1, 3.0), GR.Row(GR.UNCOND, 2)], [2, 2]),
        "partner is the row": ([GR.Row(GR.COND, 2, 3.0), GR.Row(GR.UNCOND, 2)], [2, 2]),
        "partner on another plan row": ([GR.Row(GR.COND, 3, 3.0), GR.Row(GR.UNCOND, 2)], [2, 3]),
        "partner idle": ([GR.Row(GR.COND, 3, 3.0), GR.Row(GR.UNCOND, 2)], [2, -1]),
        "partner is PLAIN": ([GR.Row(GR.COND, 3, 3.0), GR.Row(GR.PLAIN, 2)], [2, 2]),
        "partner is COND": ([GR.Row(GR.COND, 3, 3.0), GR.Row(GR.COND, 2, 3.0)], [2, 2]),
        "partner names another row": ([GR.Row(GR.COND, 3, 3.0), GR.Row(GR.UNCOND, 0)], [2, 2]),
    }
    for what, (entries, idx23) in cases.items():
        guide = [c, u] + entries + [GR.Row(), GR.Row()]
        idx = [2, 2] + idx23 + [2, 2]
        got = GR.step_rows_guided(IR.DPMPP, x, e, None, hist, plan, idx, guide)
        assert _same(got[0][2], x[2]) and _same(got[1][:, 2], hist[:, 2]), what                   # the bad row: left alone
        if what != "partner is PLAIN":                                                             # (a PLAIN row 3 is updated as such)
            assert _same(got[0][3], x[3]) and _same(got[1][:, 3], hist[:, 3]), what
        assert _same(got[0][[0, 1, 4, 5]], good[0][[0, 1, 4, 5]]) and _same(got[1][:, [0, 4, 5]], good[1][:, [0, 4, 5]]), what


# ------------------------------------------------------------------------------------------------ a staggered chain
def _chain(vpred=False, n=10, per=37, seed=0):
    """five rows on one n-step DPM-Solver++ plan (order 3): the pair A (rows 0, 1; scale 7.5, rescale 0.7) from tick 0, a plain request (row 2)
    from tick 1, the pair C (rows 3, 4; scale 3.0) from tick 3.  A's guide entries are left in place after it has finished (idle rows whose
    entry says COND), C's rows are PLAIN and idle before it joins.  Tick by tick against each request run ALONE: the pairs through
    guidance_restatement.eval32 at B = 1, the plain row through inflight_restatement.step_rows -> the per-tick states for the fault test"""
    import diffute_amd as D
    from diffute_amd.inflight import plan_records
    s = D.DPMSolverMultistepScheduler(solver_order=3, prediction_type="v_prediction" if vpred else "epsilon")
    ts, plan = plan_records(s, n)
    g = torch.Generator().manual_seed(seed)
    B, k = 5, 3
    x = torch.randn(B, per, generator=g).numpy()
    x[1] = x[4] = np.nan                                   # never read before their partners have written them
    hist = np.full((k, B, per), 7.5, np.float32)
    pairs = {"A": (0, 1, 7.5, 0.7, 0), "C": (3, 4, 3.0, 0.0, 3)}            # name -> (cond row, uncond row, scale, rescale, first tick)
    alone = {name: [x[[b, p]].copy(), hist[:, b:b + 1].copy()] for name, (b, p, _, _, _) in pairs.items()}
    plain_x, plain_h, plain_start = x[2:3].copy(), hist[:, 2:3].copy(), 1
    states, seen_ratio = [], 0
    for tick in range(len(ts) + 4):
        at = lambda start: tick - start if 0 <= tick - start < len(ts) else -1
        idx = [at(0), at(0), at(plain_start), at(3), at(3)]
        guide = list(GR.pair(0, 1, 7.5, 0.7)) + [GR.Row()] + (list(GR.pair(3, 4, 3.0, 0.0)) if tick >= 3 else [GR.Row(), GR.Row()])
        e = torch.randn(B, per, generator=g).numpy()
        states.append((x.copy(), e, hist.copy(), list(idx), guide))
        x2, h2, ratio = GR.step_rows_guided(IR.DPMPP, x, e, None, hist, plan, idx, guide, vpred)
        for name, (b, p, scale, rescale, start) in pairs.items():
            i = at(start)
            if i < 0:
                assert _same(x2[[b, p]], x[[b, p]]) and _same(h2[:, [b, p]], hist[:, [b, p]]), f"tick {tick}: idle pair {name} changed"
                continue
            want_x, want_h, want_k = G.eval32(IR.DPMPP, plan[i], alone[name][0], e[[b, p]], None, alone[name][1], scale, rescale, vpred)
            alone[name] = [want_x, want_h]
            assert _same(x2[[b, p]], want_x), f"tick {tick}: pair {name} step {i} (order {plan[i].order})"
            assert _same(h2[:, b], want_h[:, 0]) and _same(h2[:, p], hist[:, p]), f"tick {tick}: pair {name}, the ring"
            if rescale:
                assert _same(ratio[b], want_k[0])
                seen_ratio += 1
            else:
                assert np.isnan(ratio[b])
        i = at(plain_start)
        if i < 0:
            assert _same(x2[2], x[2]) and _same(h2[:, 2], hist[:, 2])
        else:
            plain_x, plain_h = IR.step_rows(IR.DPMPP, plain_x, e[2:3], None, plain_h, plan, [i], vpred)
            assert _same(x2[2], plain_x[0]) and _same(h2[:, 2], plain_h[:, 0]), f"tick {tick}: the plain row, step {i}"
        x, hist = x2, h2
    assert seen_ratio == len(ts) and np.isfinite(x).all()
    return plan, states, vpred


@pytest.mark.parametrize("vpred", [False, True])
def test_staggered_chain_equals_each_request_alone(vpred):
    _chain(vpred, 10)
    _chain(vpred, 3, seed=1)


@pytest.mark.parametrize("fault", GR.FAULTS)
def test_restatement_faults_are_seen(fault):
    """each injected fault changes at least one tick of the staggered chain"""
    plan, states, vpred = _chain()
    hit = 0
    for (x, e, hist, idx, guide) in states:
        good = GR.step_rows_guided(IR.DPMPP, x, e, None, hist, plan, idx, guide, vpred)
        bad = GR.step_rows_guided(IR.DPMPP, x, e, None, hist, plan, idx, guide, vpred, fault=fault)
        hit += int(not (_same(good[0], bad[0]) and _same(good[1], bad[1])))
    assert hit > 0, f"the fault {fault!r} went unseen on the chain"


def test_noise_goes_to_the_conditional_row_only():
    """DDPM: the pair adds noise[b] where its record asks for it and never reads the unconditional row's noise; the last step adds none"""
    plan = _plans()[IR.DDPM]
    x, eps, nz, _ = G.inputs(1, 64)
    noise = np.concatenate([nz, np.full_like(nz, np.nan)], 0)
    guide = list(GR.pair(0, 1, 3.0, 0.3))
    for i in (3, 9):
        assert plan[i].use_noise == int(i != 9)
        got = GR.step_rows_guided(IR.DDPM, x, eps, noise, None, plan, [i, i], guide)[0]
        want = G.eval32(IR.DDPM, plan[i], x, eps, nz, None, 3.0, 0.3)[0]
        assert _same(got, want) and np.isfinite(got).all()
    without = GR.step_rows_guided(IR.DDPM, x, eps, None, None, plan, [3, 3], guide)[0]
    assert not _same(without, GR.step_rows_guided(IR.DDPM, x, eps, noise, None, plan, [3, 3], guide)[0])


# ------------------------------------------------------------------------------------------------ what the host relies on
def test_guide_table_layout_and_entries():
    from diffute_amd import _cabi
    R = _cabi.GuideRow
    assert ctypes.sizeof(R) == 20
    assert [(n, getattr(R, n).offset) for n, _ in R._fields_] == [("role", 0), ("partner", 4), ("scale", 8), ("rescale", 12), ("one_minus_rescale", 16)]
    assert (_cabi.GUIDE_PLAIN, _cabi.GUIDE_COND, _cabi.GUIDE_UNCOND) == (GR.PLAIN, GR.COND, GR.UNCOND) == (0, 1, 2)
    assert bytes(R()) == bytes(20)                          # a zeroed table is all PLAIN: what the engine allocates
    syms = set(_cabi.exported_symbols())
    assert {"dmx_sched_step_rows_guided", "dmx_rows_guide"} <= syms
    restype, argtypes = _cabi._PROTOS["dmx_sched_step_rows_guided"]
    assert restype is ctypes.c_int and len(argtypes) == 14 and argtypes[9] is ctypes.c_int and argtypes[10] is ctypes.c_size_t
    restype, argtypes = _cabi._PROTOS["dmx_rows_guide"]
    assert restype is ctypes.c_int and argtypes == [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_float, ctypes.c_float,
                                                    ctypes.c_float, ctypes.c_void_p]


def test_the_engine_takes_guidance_and_the_call_lives_in_schedulers():
    import diffute_amd
    from diffute_amd import inflight, schedulers
    sig = inspect.signature(inflight.DenoiseEngine.submit)
    assert sig.parameters["guidance"].default is None and list(sig.parameters)[-2:] == ["variance_noise", "guidance"]
    assert list(inspect.signature(inflight.Planner.submit).parameters) == ["self", "n", "steps", "plan_base"]      # the planner is as it was
    pat = re.compile(r"\bdmx_sched_step_rows_guided\s*\(")
    assert len(pat.findall(inspect.getsource(schedulers.launch_step_rows_guided))) == 1
    pkg = os.path.dirname(os.path.abspath(diffute_amd.__file__))
    for f in os.listdir(pkg):
        if f.endswith(".py"):
            assert len(pat.findall(open(os.path.join(pkg, f)).read())) == (1 if f == "schedulers.py" else 0), f
    assert "launch_step_rows_guided" in inspect.getsource(inflight.DenoiseEngine.tick)
    assert "dmx_sched_step_rows(" in inspect.getsource(inflight.DenoiseEngine.tick)            # the plain tick keeps its entry
