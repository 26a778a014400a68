"""CPU-side checks of the in-flight engine (diffute_amd/inflight.py): the planner (slots, FIFO queue, mirrored row counters), the plan
records against the scheduler classes, and the numpy restatement of the per-row update (tests/inflight_restatement.py) against the
existing restatements and goldens - with three injected faults that must each break the equality."""
import os
import random

import numpy as np
import pytest
import torch

import dpm_restatement as R
import inflight_restatement as IR

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


# --------------------------------------------------------------------------------------------------------------------- planner
def _simulate(capacity, seed, n_requests=14):
    """a seeded arrival sequence through the Planner, every rule checked at every tick -> (per-ticket tick lists, requests)"""
    from diffute_amd.inflight import Planner
    rng = random.Random(seed)
    pl = Planner(capacity)
    arrivals = sorted((rng.randrange(0, 12), k) for k in range(n_requests))         # (tick of arrival, request number)
    reqs = {}                                                                       # ticket -> dict
    order = []                                                                      # tickets in submit order
    ran = {}                                                                        # ticket -> ticks it ran in
    admitted = []
    dev_index, dev_left = [-1] * capacity, [0] * capacity                           # the device rule, restated here
    next_base = 0
    a = 0
    for _ in range(200):
        while a < len(arrivals) and arrivals[a][0] <= pl.ticks:
            n, T = rng.randint(1, min(3, capacity)), rng.randint(1, 6)
            t = pl.submit(n, T, next_base)
            reqs[t] = dict(n=n, T=T, base=next_base)
            order.append(t)
            next_base += T
            a += 1
        for (t, s0, n, T, base) in pl.admit():
            assert (n, T, base) == (reqs[t]["n"], reqs[t]["T"], reqs[t]["base"])
            assert all(dev_index[b] < 0 for b in range(s0, s0 + n)), "a slot was given to two requests at once"
            for b in range(s0, s0 + n):                                             # dmx_rows_admit
                dev_index[b], dev_left[b] = base, T
            reqs[t]["slots"] = list(range(s0, s0 + n))                              # rows of one submit: consecutive slots
            admitted.append(t)
        assert pl.row_index == dev_index and pl.row_left == dev_left
        # FIFO: what has been admitted is a prefix of the submit order
        assert admitted == order[:len(admitted)]
        if a == len(arrivals) and not pl.busy():
            break
        tick = pl.ticks
        expect_done = [t for t, (s0, n) in ((t, (reqs[t]["slots"][0], reqs[t]["n"])) for t in pl.running) if dev_left[s0] == 1]
        assert sorted(t for t, _, _ in pl.finishing()) == sorted(expect_done)
        for t in list(pl.running):
            s0 = reqs[t]["slots"][0]
            assert pl.step_of(t) == len(ran.get(t, []))
            assert all(dev_index[b] == reqs[t]["base"] + pl.step_of(t) for b in reqs[t]["slots"])      # the plan row of its own step
            ran.setdefault(t, []).append(tick)
        for b in range(capacity):                                                   # dmx_rows_advance
            if dev_index[b] >= 0:
                dev_left[b] -= 1
                dev_index[b] = dev_index[b] + 1 if dev_left[b] > 0 else -1
        done = pl.advance()
        assert sorted(done) == sorted(expect_done)
        assert pl.row_index == dev_index and pl.row_left == dev_left
        assert pl.ticks == tick + 1
    else:
        raise AssertionError("the planner never went idle")
    return ran, reqs


@pytest.mark.parametrize("capacity", [1, 2, 3, 4])
@pytest.mark.parametrize("seed", [0, 1, 2])
def test_planner_rules(capacity, seed):
    ran, reqs = _simulate(capacity, 100 * capacity + seed)
    assert set(ran) == set(reqs)
    for t, ticks in ran.items():
        assert len(ticks) == reqs[t]["T"], f"request {t} ran {len(ticks)} ticks, asked {reqs[t]['T']}"
        assert ticks == list(range(ticks[0], ticks[0] + len(ticks))), f"request {t}: its ticks are not consecutive"
        s = reqs[t]["slots"]
        assert s == list(range(s[0], s[0] + reqs[t]["n"]))
    # no slot holds two requests in the same tick
    for b in range(capacity):
        seen = {}
        for t, ticks in ran.items():
            if b in reqs[t]["slots"]:
                for k in ticks:
                    assert k not in seen, f"slot {b} held requests {seen[k]} and {t} in tick {k}"
                    seen[k] = t


def test_planner_refusals_and_head_of_line():
    from diffute_amd.inflight import Planner
    pl = Planner(3)
    with pytest.raises(ValueError):
        pl.submit(4, 2, 0)
    with pytest.raises(ValueError):
        pl.submit(0, 2, 0)
    with pytest.raises(ValueError):
        pl.submit(1, 0, 0)
    a = pl.submit(2, 3, 0)
    b = pl.submit(2, 1, 3)              # does not fit beside a: waits
    c = pl.submit(1, 1, 4)              # would fit, but may not overtake b
    assert [x[0] for x in pl.admit()] == [a]
    assert pl.advance() == [] and pl.admit() == []
    pl.advance()
    assert pl.advance() == [a]
    assert [(x[0], x[1]) for x in pl.admit()] == [(b, 0), (c, 2)]
    assert sorted(pl.advance()) == [b, c] and not pl.busy()


# ---------------------------------------------------------------------------------------------------------------- plan records
def _dpm_fields(c):
    from diffute_amd import _cabi
    return {k: getattr(c, k) for k, _ in _cabi.DpmCoefs._fields_}


@pytest.mark.parametrize("n", [1, 2, 3, 10])
def test_plan_records_ddim_ddpm(n):
    import diffute_amd as D
    from diffute_amd.inflight import plan_records
    for cls, eta in ((D.DDIMScheduler, 0.0), (D.DDIMScheduler, 0.5), (D.DDPMScheduler, 0.0)):
        ref = cls(); ref.set_timesteps(n)
        ts, recs = plan_records(cls(), n, eta)
        assert ts == ref.timesteps.tolist() and len(recs) == n
        for t, r in zip(ts, recs):
            want = ref.step_coefficients(t, eta) if cls is D.DDIMScheduler else ref.step_coefficients(t)
            assert [float(v) for v in r.c] == [float(np.float32(v)) for v in want]
            assert [np.float32(v) for v in r.c] == [np.float32(v) for v in want]
            assert r.timestep == t
            assert r.use_noise == (int(eta > 0) if cls is D.DDIMScheduler else int(t > 0))


@pytest.mark.parametrize("order", [1, 2, 3])
@pytest.mark.parametrize("n", [1, 2, 3, 10])
def test_plan_records_dpmpp(n, order):
    import diffute_amd as D
    from diffute_amd.inflight import plan_records
    ref = D.DPMSolverMultistepScheduler(solver_order=order); ref.set_timesteps(n)
    ts, recs = plan_records(D.DPMSolverMultistepScheduler(solver_order=order), n)
    assert ts == ref.timesteps.tolist() and len(recs) == len(ref._plan)
    assert [r.order for r in recs] == R.orders(len(ts), order)          # lower-order first and final steps included
    for i, (r, (o, c)) in enumerate(zip(recs, ref._plan)):
        assert r.order == o and _dpm_fields(r.dpm) == _dpm_fields(c)
        assert (r.ring_w, r.ring_m1, r.ring_m2) == (i % order, (i - 1) % order, (i - 2) % order)
        assert r.timestep == ts[i] and r.use_noise == 0


def _rec_fields(r):
    return (list(r.c), _dpm_fields(r.dpm), r.order, r.use_noise, r.ring_w, r.ring_m1, r.ring_m2, r.timestep)


@pytest.mark.parametrize("n", [1, 3, 10])
def test_scheduler_plan_equals_plan_records(n):
    """scheduler.plan(eta) after set_timesteps(n) is plan_records(a fresh scheduler, n, eta), field by field, for the three classes"""
    import diffute_amd as D
    from diffute_amd.inflight import plan_records
    cases = [(D.DDIMScheduler, {}, 0.0), (D.DDIMScheduler, {}, 0.5), (D.DDPMScheduler, {}, 0.0), (D.DPMSolverMultistepScheduler, {}, 0.0),
             (D.DPMSolverMultistepScheduler, dict(solver_order=3, solver_type="heun"), 0.0)]
    for cls, kw, eta in cases:
        s = cls(**kw)
        with pytest.raises(ValueError):
            s.plan(eta)                                                  # no grid yet
        s.set_timesteps(n)
        ts, recs = plan_records(cls(**kw), n, eta)
        got = s.plan(eta)
        assert ts == s.timesteps.tolist() and len(got) == len(recs) == len(ts)
        assert [_rec_fields(r) for r in got] == [_rec_fields(r) for r in recs]
        assert [r.timestep for r in got] == ts
        assert [_rec_fields(r) for r in s.iter_plan(eta)] == [_rec_fields(r) for r in got]      # the lazy walk denoise() takes


def test_launch_step_is_the_only_caller_of_the_scalar_step_entries():
    """in diffute_amd/*.py the three scalar entries are named inside schedulers.launch_step and nowhere else (their signatures come from
    include/diffute_hip.h: _cabi.py holds no table that names them)"""
    import inspect
    import re
    import diffute_amd
    from diffute_amd import schedulers
    pat = re.compile(r"dmx_sched_step_(ddim|ddpm|dpmpp)\b")
    pkg = os.path.dirname(os.path.abspath(diffute_amd.__file__))
    body = inspect.getsource(schedulers.launch_step)
    assert len(pat.findall(body)) == 3
    from diffute_amd import _cabi
    assert {"dmx_sched_step_ddim", "dmx_sched_step_ddpm", "dmx_sched_step_dpmpp"} <= set(_cabi.exported_symbols())
    for root, _, files in os.walk(pkg):
        for f in files:
            if not f.endswith(".py"):
                continue
            text = open(os.path.join(root, f)).read()
            hits = len(pat.findall(text))
            if f == "schedulers.py":
                assert text.count(body) == 1 and hits == 3, "schedulers.py names the entries outside launch_step"
            else:
                assert hits == 0, f"{f} names a scalar step entry: go through schedulers.launch_step"


def test_record_layout():
    """the record is 88 bytes with the timestep last (the kernel's struct, which a static_assert holds to the same size)"""
    import ctypes
    from diffute_amd import _cabi
    assert ctypes.sizeof(_cabi.SchedRowRec) == 88 and _cabi.SchedRowRec.timestep.offset == 80 and _cabi.SchedRowRec.dpm.offset == 20


# ---------------------------------------------------------------------------------------------------------------- restatement
def _ddim_ddpm_case():
    import diffute_amd as D
    from diffute_amd.inflight import plan_records
    g = np.load(os.path.join(GOLD, "sched.npz"))
    rng = np.random.default_rng(5)
    per = g["x"].size
    x = np.stack([g["x"].reshape(-1), rng.standard_normal(per).astype(np.float32), rng.standard_normal(per).astype(np.float32)])
    e = np.stack([g["eps"].reshape(-1), rng.standard_normal(per).astype(np.float32), rng.standard_normal(per).astype(np.float32)])
    nz = np.stack([g["noise"].reshape(-1)] * 3)
    return g, x, e, nz, plan_records(D.DDIMScheduler(), 50), plan_records(D.DDPMScheduler(), 50)


def test_restatement_ddim_ddpm_rows_equal_oracle_and_golden():
    from oracle import schedulers as OS
    g, x, e, nz, (ts_i, plan_i), (ts_p, plan_p) = _ddim_ddpm_case()
    # DDIM: row 0 at t = 981 (the golden's step), row 1 idle, row 2 at t = 1
    idx = [ts_i.index(981), -1, ts_i.index(1)]
    for vpred in (False, True):
        out, _ = IR.step_rows(IR.DDIM, x, e, None, None, plan_i, idx, vpred)
        for b in (0, 2):
            ref = OS.ddim_apply(tuple(plan_i[idx[b]].c), e[b], x[b], None, "v_prediction" if vpred else "epsilon")
            assert np.array_equal(out[b], ref)
        assert np.array_equal(out[1], x[1])
    out, _ = IR.step_rows(IR.DDIM, x, e, None, None, plan_i, idx)
    assert np.allclose(out[0], g["ddim_step_981_50"].reshape(-1), rtol=1e-5, atol=1e-6)      # (the bound test_models_gpu.py holds the product to)
    first = IR.step_rows(IR.DDIM, x[:1], e[:1], None, None, plan_i, [ts_i.index(1)])[0][0]
    assert np.allclose(first, g["ddim_step_1_50"].reshape(-1), rtol=1e-5, atol=1e-6)
    # DDPM: t = 980 with noise, idle, t = 0 without
    idx = [ts_p.index(980), -1, ts_p.index(0)]
    out, _ = IR.step_rows(IR.DDPM, x, e, nz, None, plan_p, idx)
    assert np.array_equal(out[0], OS.ddpm_apply(tuple(plan_p[idx[0]].c), e[0], x[0], nz[0]))
    assert np.array_equal(out[2], OS.ddpm_apply(tuple(plan_p[idx[2]].c), e[2], x[2], None))
    assert np.array_equal(out[1], x[1])
    assert np.allclose(out[0], g["ddpm_step_980_50"].reshape(-1), rtol=1e-5, atol=1e-6)
    last = IR.step_rows(IR.DDPM, x[:1], e[:1], nz[:1], None, plan_p, [ts_p.index(0)])[0][0]
    assert np.allclose(last, g["ddpm_step_0_50"].reshape(-1), rtol=1e-5, atol=1e-6)


def _dpm_chain(order, solver_type, vpred, n, per=37, seed=0):
    """three rows staggered on one n-step plan (row b starts at tick b; the middle row idles on odd ticks before it starts): the
    restatement tick by tick vs tests/dpm_restatement.py run on each row alone -> the list of per-tick states for the fault tests"""
    import diffute_amd as D
    from diffute_amd.inflight import plan_records
    s = D.DPMSolverMultistepScheduler(solver_order=order, solver_type=solver_type, prediction_type="v_prediction" if vpred else "epsilon")
    ts, plan = plan_records(s, n)
    tab = R.tables(s.alphas_cumprod)
    g = torch.Generator().manual_seed(seed)
    B, k = 3, order
    x = torch.randn(B, per, generator=g).numpy()
    hist = np.full((k, B, per), 7.5, np.float32)
    ref_x = [torch.from_numpy(x[b].copy()) for b in range(B)]
    ref_h = [[] for _ in range(B)]
    start = [0, 3, 1]
    states = []
    for tick in range(len(ts) + 3):
        idx = [tick - start[b] if 0 <= tick - start[b] < len(ts) else -1 for b in range(B)]
        e = torch.randn(B, per, generator=g).numpy()
        states.append((x.copy(), e, hist.copy(), list(idx)))
        x2, h2 = IR.step_rows(IR.DPMPP, x, e, None, hist, plan, idx, vpred)
        for b in range(B):
            if idx[b] < 0:
                assert np.array_equal(x2[b], x[b]) and np.array_equal(h2[:, b], hist[:, b])
                continue
            i = idx[b]
            rx, m0 = R.step(tab, ts, i, ref_x[b], torch.from_numpy(e[b]), ref_h[b], plan[i].order, solver_type, vpred)
            ref_x[b] = rx; ref_h[b].append(m0)
            assert np.array_equal(x2[b], rx.numpy()), f"row {b} step {i} (order {plan[i].order})"
            assert np.array_equal(h2[i % k, b], m0.numpy())
            others = [j for j in range(k) if j != i % k]
            assert np.array_equal(h2[others, b], hist[others, b])
        x, hist = x2, h2
    return plan, states, vpred


@pytest.mark.parametrize("vpred", [False, True])
@pytest.mark.parametrize("order,solver_type", [(1, "midpoint"), (2, "midpoint"), (2, "heun"), (3, "midpoint")])
def test_restatement_dpmpp_rows_equal_dpm_restatement(order, solver_type, vpred):
    _dpm_chain(order, solver_type, vpred, 10)
    _dpm_chain(order, solver_type, vpred, 3, seed=1)


@pytest.mark.parametrize("fault", ["idle_updated", "neighbour_rec", "ring_next"])
def test_restatement_faults_are_seen(fault):
    """each injected fault changes at least one tick of the staggered chain (and, where it applies, of the DDIM / DDPM rows)"""
    plan, states, vpred = _dpm_chain(3, "midpoint", False, 10)
    hit = 0
    for (x, e, hist, idx) in states:
        good = IR.step_rows(IR.DPMPP, x, e, None, hist, plan, idx, vpred)
        bad = IR.step_rows(IR.DPMPP, x, e, None, hist, plan, idx, vpred, fault=fault)
        hit += int(not (np.array_equal(good[0], bad[0]) and np.array_equal(good[1], bad[1])))
    assert hit > 0, f"the fault {fault!r} went unseen on the DPM-Solver++ chain"
    if fault != "ring_next":
        _, x, e, nz, (ts_i, plan_i), (ts_p, plan_p) = _ddim_ddpm_case()
        for kind, plan_k, idx in ((IR.DDIM, plan_i, [ts_i.index(981), -1, ts_i.index(1)]), (IR.DDPM, plan_p, [ts_p.index(980), -1, ts_p.index(0)])):
            good = IR.step_rows(kind, x, e, nz, None, plan_k, idx)[0]
            bad = IR.step_rows(kind, x, e, nz, None, plan_k, idx, fault=fault)[0]
            assert not np.array_equal(good, bad), f"the fault {fault!r} went unseen on kind {kind}"


def test_engine_module_imports_without_a_gpu():
    import diffute_amd as D
    from diffute_amd import inflight
    assert D.DenoiseEngine is inflight.DenoiseEngine
    assert inflight.scheduler_kind(D.DDIMScheduler()) == 0 and inflight.scheduler_kind(D.DDPMScheduler()) == 1
    assert inflight.scheduler_kind(D.DPMSolverMultistepScheduler()) == 2
    with pytest.raises(TypeError):
        inflight.scheduler_kind(object())
