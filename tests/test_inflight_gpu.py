"""In-flight batching on the GPU (diffute_amd/inflight.py, include/diffute_hip.h "in-flight batching"): the per-row scheduler launch
against the scalar entries, the admit / advance counters against the planner's mirror, the per-row time-embedding fetch, the row-wise
context projection, and the engine against denoise() and the oracle goldens.  The two loops share one step plan, one step kernel body, one
context projection and one time-embedding fetch, so the shared pieces are pinned on their own as well (sections 9-12): the scalar step
entries against the CPU restatement, denoise()'s C calls, the workspace query, and the scalar form of the time-embedding fetch."""
import ctypes
import functools
import os

import numpy as np
import pytest
import torch

from util import assert_close

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
TINY_UNET = dict(block_out_channels=(64, 128, 256, 256), attention_head_dim=(1, 2, 4, 4), cross_attention_dim=128)
E2E_EMU = 2.5e-2                 # tests/test_models_gpu.py: the tiny UNet's eps against tests/golden/tiny_unet.npz
SENT = 0x7A5A5A5A                # tests/util.py SENTINEL_BITS[float32]
GUARD = 64                       # floats of sentinel before and after every buffer


@pytest.fixture(scope="module", params=["bf16", "fp16"])
def tiny_unet(cuda, request):
    import diffute_amd as D
    u = D.UNet2DConditionModel(**TINY_UNET)
    u = u.to(cuda, dtype=torch.float16) if request.param == "fp16" else u.cuda()
    return u.requires_grad_(False)


@pytest.fixture(scope="module")
def tiny_unet_bf16(cuda):
    import diffute_amd as D
    return D.UNet2DConditionModel(**TINY_UNET).cuda().requires_grad_(False)


def _upload_plan(recs, dev):
    return torch.frombuffer(bytearray(b"".join(bytes(r) for r in recs)), dtype=torch.uint8).to(dev)


def _copy_rec(r):
    from diffute_amd import _cabi
    c = _cabi.SchedRowRec()
    ctypes.memmove(ctypes.byref(c), ctypes.byref(r), ctypes.sizeof(c))
    return c


# ------------------------------------------------------------------------------------------------ 1. dmx_sched_step_rows
def _guarded(n, offset, dev, gen, data=None):
    """n floats of seeded data (or of `data`) inside sentinel guard bands, `offset` floats past a 16-byte boundary -> (whole buffer, view)"""
    buf = torch.full((GUARD + offset + n + GUARD,), SENT, dtype=torch.int32, device=dev).view(torch.float32)
    view = buf[GUARD + offset:GUARD + offset + n]
    view.copy_(torch.randn(n, generator=gen).to(dev) if data is None else data)
    return buf, view


def _bits(t):
    return t.contiguous().view(torch.int32)


def _rows_case(lib, dev, kind, per, recs, idx, vpred, offset, seed, n_hist=0):
    """one dmx_sched_step_rows launch over B = len(idx) rows vs the scalar entry on every active row alone; the whole of every guarded
    buffer - idle rows, history slots nobody writes, guard bands - is compared bit for bit with what it should hold"""
    from diffute_amd import _cabi
    B = len(idx)
    gen = torch.Generator().manual_seed(seed)
    st = _cabi.current_stream()
    xb, x = _guarded(B * per, offset, dev, gen)
    eb, e = _guarded(B * per, offset, dev, gen)
    nb, nz = _guarded(B * per, offset, dev, gen)
    hb, h = _guarded(max(n_hist, 1) * B * per, offset, dev, gen)
    want_x, want_h = xb.clone(), hb.clone()
    wx = want_x[GUARD + offset:GUARD + offset + B * per].view(B, per)
    wh = want_h[GUARD + offset:GUARD + offset + max(n_hist, 1) * B * per].view(max(n_hist, 1), B, per)
    e_keep, n_keep = eb.clone(), nb.clone()
    xr, er, nr, hr = x.view(B, per), e.view(B, per), nz.view(B, per), h.view(max(n_hist, 1), B, per)
    for b, i in enumerate(idx):
        if i < 0:
            continue
        r = recs[i]
        xs, es, out = xr[b].clone(), er[b].clone(), torch.empty(per, device=dev)
        if kind == _cabi.SCHED_DPMPP:
            m1 = hr[r.ring_m1, b].clone() if r.order >= 2 else None
            m2 = hr[r.ring_m2, b].clone() if r.order >= 3 else None
            m0 = torch.empty(per, device=dev)
            _cabi.check(lib.dmx_sched_step_dpmpp(_cabi.ptr(xs), _cabi.ptr(es), _cabi.ptr(m1), _cabi.ptr(m2), _cabi.ptr(m0), _cabi.ptr(out), per,
                                                 r.order, r.dpm, vpred, st), "dpmpp", lib)
            wh[r.ring_w, b].copy_(m0)
        else:
            ns = nr[b].clone() if r.use_noise else None
            fn = lib.dmx_sched_step_ddim if kind == _cabi.SCHED_DDIM else lib.dmx_sched_step_ddpm
            _cabi.check(fn(_cabi.ptr(xs), _cabi.ptr(es), _cabi.ptr(ns), _cabi.ptr(out), per, *[float(v) for v in r.c], vpred, st), "scalar step", lib)
        wx[b].copy_(out)
    plan = _upload_plan(recs, dev)
    row_index = torch.tensor(idx, dtype=torch.int32, device=dev)
    _cabi.check(lib.dmx_sched_step_rows(_cabi.ptr(x), _cabi.ptr(e), _cabi.ptr(nz), _cabi.ptr(h) if n_hist else None, n_hist, _cabi.ptr(plan),
                                        _cabi.ptr(row_index), B, per, kind, vpred, st), "sched_step_rows", lib)
    torch.cuda.synchronize()
    what = f"kind {kind} per {per} vpred {vpred} offset {offset} rows {idx}"
    bad = (_bits(xb) != _bits(want_x)).nonzero()
    assert bad.numel() == 0, f"{what}: sample buffer differs at {bad.numel()} floats, first {int(bad[0]) - GUARD - offset} (row-major, guard excluded)"
    bad = (_bits(hb) != _bits(want_h)).nonzero()
    assert bad.numel() == 0, f"{what}: history buffer differs at {bad.numel()} floats, first {int(bad[0]) - GUARD - offset}"
    assert torch.equal(_bits(eb), _bits(e_keep)) and torch.equal(_bits(nb), _bits(n_keep)), f"{what}: an input was written"


@pytest.mark.parametrize("build", ["bf16", "fp16"])
@pytest.mark.parametrize("per", [37, 1024, 16384])
def test_sched_step_rows_ddim_ddpm(cuda, per, build):
    import diffute_amd as D
    from diffute_amd import _cabi
    from diffute_amd.inflight import plan_records
    lib = _cabi.lib(build)
    _, ddim = plan_records(D.DDIMScheduler(), 10, eta=0.5)
    ddim = [_copy_rec(r) for r in ddim]
    ddim[7].use_noise = 0                                   # noise on for one row, off for the other
    _, ddpm = plan_records(D.DDPMScheduler(), 10)           # t > 0: noise, the last step (t = 0): none
    for offset in (0, 1):
        for vpred in (0, 1):
            _rows_case(lib, cuda, _cabi.SCHED_DDIM, per, ddim, [2, -1, 7], vpred, offset, seed=per + vpred)
            _rows_case(lib, cuda, _cabi.SCHED_DDPM, per, ddpm, [9, -1, 3], vpred, offset, seed=per + 7 + vpred)
    _cabi.poll_device_error(lib)


@pytest.mark.parametrize("build", ["bf16", "fp16"])
@pytest.mark.parametrize("per", [37, 1024, 16384])
def test_sched_step_rows_dpmpp(cuda, per, build):
    import diffute_amd as D
    from diffute_amd import _cabi
    from diffute_amd.inflight import plan_records
    lib = _cabi.lib(build)
    _, recs = plan_records(D.DPMSolverMultistepScheduler(solver_order=3), 10)       # orders 1 2 3 3 3 3 3 3 2 1
    assert [r.order for r in recs] == [1, 2, 3, 3, 3, 3, 3, 3, 2, 1]
    for offset in (0, 1):
        for vpred in (0, 1):
            for idx in ([0, -1, 1], [4, -1, 9], [8, -1, 5]):                        # orders (1, 2), (3, 1), (2, 3); every ring position
                _rows_case(lib, cuda, _cabi.SCHED_DPMPP, per, recs, idx, vpred, offset, seed=per + vpred + idx[0], n_hist=3)
    _, r2 = plan_records(D.DPMSolverMultistepScheduler(solver_order=2, solver_type="heun"), 5)
    _rows_case(lib, cuda, _cabi.SCHED_DPMPP, per, r2, [1, -1, 4], 0, 0, seed=3, n_hist=2)
    _cabi.poll_device_error(lib)


# ------------------------------------------------------------------------------------------------ 2. admit / advance
@pytest.mark.parametrize("build", ["bf16", "fp16"])
def test_rows_admit_advance_follow_the_planner(cuda, build):
    from diffute_amd import _cabi
    from diffute_amd.inflight import Planner
    lib = _cabi.lib(build)
    B = 4
    pl = Planner(B)
    buf = torch.full((GUARD + 2 * B + GUARD,), SENT, dtype=torch.int32, device=cuda)
    row_index, row_left = buf[GUARD:GUARD + B], buf[GUARD + B:GUARD + 2 * B]
    row_index.fill_(-1); row_left.zero_()
    st = _cabi.current_stream()
    script = {0: [(2, 3, 0), (1, 1, 3)], 1: [(3, 2, 4)], 2: [(1, 4, 6)], 5: [(4, 1, 10)]}       # tick -> [(rows, steps, plan base)]
    for tick in range(12):
        for (n, T, base) in script.get(tick, []):
            pl.submit(n, T, base)
        for (_, s0, n, T, base) in pl.admit():
            for b in range(s0, s0 + n):
                _cabi.check(lib.dmx_rows_admit(_cabi.ptr(row_index), _cabi.ptr(row_left), b, base, T, st), "rows_admit", lib)
        assert row_index.tolist() == pl.row_index and row_left.tolist() == pl.row_left, f"tick {tick} after admit"
        _cabi.check(lib.dmx_rows_advance(_cabi.ptr(row_index), _cabi.ptr(row_left), B, st), "rows_advance", lib)
        pl.advance()
        assert row_index.tolist() == pl.row_index and row_left.tolist() == pl.row_left, f"tick {tick} after advance"
    assert not pl.busy() and row_index.tolist() == [-1] * B
    assert bool((buf[:GUARD] == SENT).all()) and bool((buf[GUARD + 2 * B:] == SENT).all())


# ------------------------------------------------------------------------------------------------ 3. temb rows
def test_temb_rows_equal_explicit_timesteps(cuda, tiny_unet):
    import diffute_amd as D
    from diffute_amd.inflight import plan_records
    from diffute_amd.synthetic import synth_inputs
    lat, mask, mlat, ctx = synth_inputs(3, 16, 16, 77, 128, device=cuda)
    ts, recs = plan_records(D.DDIMScheduler(), 4)
    ts_dev = torch.tensor(ts, dtype=torch.int64, device=cuda)
    table = tiny_unet.temb_table(ts_dev)
    plan = _upload_plan(recs, cuda)
    row_index = torch.tensor([2, -1, 0], dtype=torch.int32, device=cuda)
    tbuf = torch.full((3,), -7, dtype=torch.int64, device=cuda)
    tiny_unet.set_context(ctx, slot="t3")
    a = tiny_unet.forward_parts([lat, mask, mlat], tbuf, slot="t3", temb=(table, row_index, plan)).clone()
    assert tbuf.tolist() == [ts[2], ts[0], ts[0]]                    # the timesteps argument stays truthful (an idle row is served row 0)
    b = tiny_unet.forward_parts([lat, mask, mlat], torch.tensor([ts[2], ts[0], ts[0]], dtype=torch.int64, device=cuda), slot="t3")
    D.synchronize()
    assert torch.isfinite(a).all()
    assert torch.equal(a[0], b[0]) and torch.equal(a[2], b[2])
    with pytest.raises(ValueError):                                  # the per-row form wants [B] of each
        tiny_unet.forward_parts([lat, mask, mlat], tbuf[:1], slot="t3", temb=(table, row_index, plan))
    tiny_unet._slots.pop("t3")


# ------------------------------------------------------------------------------------------------ 4. set_context_rows
def _cache(unet, slot):
    return unet._slot(slot)["ctx_cache"]


def test_set_context_rows_all_rows_equal_set_context(cuda, tiny_unet):
    from diffute_amd.synthetic import synth_inputs
    _, _, _, ctx = synth_inputs(3, 16, 16, 77, 128, device=cuda)
    tiny_unet.set_context(ctx, slot="c4a")
    tiny_unet.reserve_context(3, 77, slot="c4b")
    tiny_unet.set_context_rows(ctx, 0, slot="c4b")
    torch.cuda.synchronize()
    a, b = _cache(tiny_unet, "c4a"), _cache(tiny_unet, "c4b")
    assert a.numel() == b.numel() and torch.equal(a, b)
    for bad in (lambda: tiny_unet.set_context_rows(ctx, 1, slot="c4b"),                         # rows [1, 4) of 3
                lambda: tiny_unet.set_context_rows(ctx[:1, :40].contiguous(), 0, slot="c4b")):   # another context length
        with pytest.raises(ValueError):
            bad()
    tiny_unet._slots.pop("c4a"); tiny_unet._slots.pop("c4b")


def test_set_context_rows_replaces_one_row_only(cuda, tiny_unet):
    """Row 1 of a set_context cache is replaced by context A and, from the same snapshot, by -A.  The projection has no bias and rounds
    symmetrically, so the two results are each other's negation: every 16-bit element of row 1 that is not an exact zero differs between
    them, and an element they share is an exact zero both times (the padded context rows, which the snapshot holds as zeros too).  Hence
    "changed against the snapshot" must be a subset of "differs between the two results", at the cache's element granularity, and that set
    is bounded by the size of one row's slabs."""
    from diffute_amd import _cabi
    from diffute_amd.synthetic import synth_inputs
    lat, mask, mlat, ctx = synth_inputs(3, 16, 16, 77, 128, device=cuda)
    _, _, _, other = synth_inputs(1, 16, 16, 77, 128, device=cuda, seed=5)
    t = torch.tensor([981, 500, 3], dtype=torch.int64, device=cuda)
    slot = "c4"
    tiny_unet.set_context(ctx, slot=slot)
    cache = _cache(tiny_unet, slot)
    snap = cache.clone()
    eps0 = tiny_unet.forward_parts([lat, mask, mlat], t, slot=slot).clone()
    tiny_unet.set_context_rows(other, 1, slot=slot)
    res_a = cache.clone()
    eps_a = tiny_unet.forward_parts([lat, mask, mlat], t, slot=slot).clone()
    cache.copy_(snap)
    tiny_unet.set_context_rows(-other, 1, slot=slot)
    res_b = cache.clone()
    torch.cuda.synchronize()
    n16 = cache.numel() // 2
    s16, a16, b16 = (x[:2 * n16].view(torch.int16) for x in (snap, res_a, res_b))
    differ = a16 != b16
    for name, r16 in (("A", a16), ("-A", b16)):
        changed = r16 != s16
        assert bool(changed.any()), f"context {name}: nothing was written"
        assert not bool((changed & ~differ).any()), f"context {name}: {int((changed & ~differ).sum())} elements outside the replaced row changed"
    assert torch.equal(res_a[2 * n16:], snap[2 * n16:]) and torch.equal(res_b[2 * n16:], snap[2 * n16:])
    # the region: one row's [sp][2C] slab of every cross-attention layer, sum of sp * 2C * 2 bytes - what a cache for ONE row holds (the
    # slabs are multiples of its 256-byte alignment)
    bound = int(tiny_unet._lib.dmx_unet_context_bytes(tiny_unet._h, 1, 77))
    assert bound == sum(128 * 2 * c * 2 for c in (64, 64, 128, 128, 256, 256, 256, 256, 256, 256, 128, 128, 128, 64, 64, 64))
    assert 2 * int(differ.sum()) <= bound, f"{2 * int(differ.sum())} bytes differ, one row holds {bound}"
    assert torch.equal(eps_a[0], eps0[0]) and torch.equal(eps_a[2], eps0[2])
    assert not torch.equal(eps_a[1], eps0[1])
    _cabi.poll_device_error()
    tiny_unet._slots.pop(slot)


def test_cache_built_row_by_row(cuda, tiny_unet_bf16):
    """(c): the cache projected one row at a time (GEMMs of M = sp instead of M = B*sp).  Measured on the MI355X it is the set_context cache
    bit for bit (the projection's tile plan does not split K, so a row's sums do not depend on M) - which is asserted, with eps, in place
    of the looser golden bound; the bounds tests/test_models_gpu.py holds the set_context path to then follow, and are kept as a check of
    the fixture."""
    from diffute_amd.synthetic import synth_inputs
    unet = tiny_unet_bf16
    g = np.load(os.path.join(GOLD, "tiny_unet.npz"))
    lat, mask, mlat, ctx = synth_inputs(2, 16, 16, 77, 128, device=cuda)
    t = torch.tensor([981], dtype=torch.int64, device=cuda)
    unet.reserve_context(2, 77, slot="c4c")
    for b in range(2):
        unet.set_context_rows(ctx[b:b + 1], b, slot="c4c")
    y = unet.forward_parts([lat, mask, mlat], t, slot="c4c").clone()
    unet.set_context(ctx, slot="c4d")
    y_ref = unet.forward_parts([lat, mask, mlat], t, slot="c4d").clone()
    torch.cuda.synchronize()
    assert torch.equal(_cache(unet, "c4c"), _cache(unet, "c4d")), "the row-by-row cache differs from set_context's"
    assert torch.equal(y, y_ref)
    assert_close(y, torch.from_numpy(g["eps_bf16emu"]), E2E_EMU, "tiny unet over a row-by-row context cache vs bf16emu")
    assert_close(y, torch.from_numpy(g["eps_fp32"]), 5e-2, "tiny unet over a row-by-row context cache vs fp32")
    unet._slots.pop("c4c"); unet._slots.pop("c4d")


# ------------------------------------------------------------------------------------------------ 5. aligned engine == denoise()
@pytest.mark.parametrize("sched", ["ddim", "ddpm", "dpmpp"])
def test_aligned_engine_equals_denoise(cuda, tiny_unet, sched):
    import diffute_amd as D
    from diffute_amd.init import normal
    from diffute_amd.synthetic import synth_inputs
    lat, mask, mlat, ctx = synth_inputs(2, 16, 16, 77, 128, device=cuda)
    make = {"ddim": D.DDIMScheduler, "ddpm": D.DDPMScheduler, "dpmpp": D.DPMSolverMultistepScheduler}[sched]
    nz = normal(3, 31, 4 * 2 * 4 * 16 * 16, cuda).reshape(4, 2, 4, 16, 16) if sched == "ddpm" else None
    ref = D.denoise(tiny_unet, make(), lat, mask, mlat, ctx, 4, variance_noise=nz).clone()
    caller = make()
    before = caller.timesteps.clone()
    eng = D.DenoiseEngine(tiny_unet, caller, capacity=2, latent_shape=(4, 16, 16), ctx_len=77)
    tk = eng.submit(lat, mask, mlat, ctx, 4, variance_noise=nz)
    done = [eng.tick() for _ in range(4)]
    assert done == [[], [], [], [tk]] and not eng.planner.busy()
    out = eng.result(tk)
    D.synchronize()
    assert torch.equal(out, ref), f"{sched}: max abs diff {float((out - ref).abs().max()):.3e}"
    assert torch.equal(caller.timesteps, before) and caller.num_inference_steps is None       # the caller's scheduler was not touched
    with pytest.raises(KeyError):
        eng.result(tk)
    eng.close()


# ------------------------------------------------------------------------------------------------ 6. rows do not interact
def test_rows_do_not_interact(cuda, tiny_unet):
    import diffute_amd as D
    from diffute_amd.inflight import Planner
    from diffute_amd.synthetic import synth_inputs
    A = synth_inputs(1, 16, 16, 77, 128, device=cuda, seed=0)
    W = synth_inputs(3, 16, 16, 77, 128, device=cuda, seed=20)
    Bq = synth_inputs(1, 16, 16, 77, 128, device=cuda, seed=30)
    Cq = synth_inputs(1, 16, 16, 77, 128, device=cuda, seed=40)
    Dq = synth_inputs(1, 16, 16, 77, 128, device=cuda, seed=50)
    eng = D.DenoiseEngine(tiny_unet, D.DDIMScheduler(), capacity=3, latent_shape=(4, 16, 16), ctx_len=77)
    w = eng.submit(*W, 1)                          # every slot has held another context before
    assert eng.run_until_idle() == [w]
    # run 1: A alone, slot 0
    a1 = eng.submit(*A, 4)
    assert eng.planner.running[a1][0] == 0
    assert eng.run_until_idle() == [a1]
    alone = eng.result(a1).clone()
    # run 2: A in slot 0 again; a 3-step request joins at tick 1, a 2-step one at tick 2, a 1-step one queues for the first free slot
    pl = Planner(3)                                # the prediction: the same script through a planner of its own
    script = {0: [("a", A, 4)], 1: [("b", Bq, 3)], 2: [("c", Cq, 2), ("d", Dq, 1)]}
    tickets, names, predicted, got = {}, {}, {}, {}
    for tick in range(5):
        for name, q, T in script.get(tick, []):
            tickets[name] = eng.submit(*q, T)
            names[pl.submit(1, T, 0)] = name
        pl.admit()
        for t in pl.advance():
            predicted[names[t]] = tick
        for t in eng.tick():
            got[[k for k, v in tickets.items() if v == t][0]] = tick
    assert predicted == {"a": 3, "b": 3, "c": 3, "d": 4} and got == predicted
    assert not eng.planner.busy()
    together = eng.result(tickets["a"])
    others = [eng.result(tickets[k]) for k in "bcd"]
    D.synchronize()
    assert torch.equal(together, alone), f"A changed with neighbours: max abs diff {float((together - alone).abs().max()):.3e}"
    assert all(torch.isfinite(o).all() for o in others) and torch.isfinite(eng.eps).all()       # idle rows: finite eps
    eng.close()


# ------------------------------------------------------------------------------------------------ 7. staggered run vs the oracle
def test_staggered_run_against_the_oracle(cuda, tiny_unet_bf16):
    import diffute_amd as D
    from diffute_amd.synthetic import synth_inputs
    g = np.load(os.path.join(GOLD, "tiny_loop.npz"))
    lat, mask, mlat, ctx = synth_inputs(2, 16, 16, 77, 128, device=cuda)
    F = synth_inputs(1, 16, 16, 77, 128, device=cuda, seed=9)
    row = lambda b: (lat[b:b + 1], mask[b:b + 1], mlat[b:b + 1], ctx[b:b + 1])
    eng = D.DenoiseEngine(tiny_unet_bf16, D.DDIMScheduler(), capacity=3, latent_shape=(4, 16, 16), ctx_len=77)
    s0 = eng.submit(*row(0), 4)                    # slot 0, ticks 0..3
    x1 = eng.submit(*F, 1)                         # slot 1, tick 0 only
    f3 = eng.submit(*F, 3)                         # the third slot, ticks 0..2
    assert [eng.planner.running[t][0] for t in (s0, x1, f3)] == [0, 1, 2]
    assert eng.tick() == [x1] and eng.tick() == []
    s1 = eng.submit(*row(1), 4)                    # arrives at tick 2: slot 1, ticks 2..5
    assert eng.planner.running[s1][0] == 1 and eng.planner.ticks == 2
    assert eng.tick() == [f3] and eng.tick() == [s0] and eng.tick() == [] and eng.tick() == [s1]
    out = torch.cat([eng.result(s0), eng.result(s1)], 0)
    D.synchronize()
    for b in range(2):
        e16 = assert_close(out[b:b + 1], torch.from_numpy(g["ddim_bf16emu"][b:b + 1]), 2e-2, f"staggered engine, sample {b} vs bf16emu")
        e32 = assert_close(out[b:b + 1], torch.from_numpy(g["ddim_fp32"][b:b + 1]), 5e-2, f"staggered engine, sample {b} vs fp32")
        print(f"staggered engine sample {b} rel-L2: vs bf16emu {e16:.2e}, vs fp32 {e32:.2e}")
    eng.close()


# ------------------------------------------------------------------------------------------------ 8. refusals
def test_refusals_leave_the_engine_usable(cuda, tiny_unet_bf16):
    import diffute_amd as D
    from diffute_amd.synthetic import synth_inputs
    unet = tiny_unet_bf16
    lat, mask, mlat, ctx = synth_inputs(3, 16, 16, 77, 128, device=cuda)
    with pytest.raises(ValueError):
        D.DenoiseEngine(unet, D.DPMSolverMultistepScheduler(), capacity=2, latent_shape=(4, 16, 16), ctx_len=77, eta=0.5)
    eng = D.DenoiseEngine(unet, D.DPMSolverMultistepScheduler(), capacity=2, latent_shape=(4, 16, 16), ctx_len=77)
    two = lambda t: t[:2].contiguous()
    with pytest.raises(ValueError):
        eng.submit(lat, mask, mlat, ctx, 4)                                                   # 3 rows, capacity 2
    with pytest.raises(ValueError):
        eng.submit(two(lat)[:, :, :8].contiguous(), two(mask), two(mlat), two(ctx), 4)        # a wrong latent shape
    with pytest.raises(ValueError):
        eng.submit(two(lat), two(mask), two(mlat), two(ctx)[:, :40].contiguous(), 4)          # a wrong context length
    with pytest.raises(ValueError):
        eng.submit(two(lat), two(mask), two(mlat), two(ctx), 4, variance_noise=torch.zeros(4, 2, 4, 16, 16, device=cuda))
    assert not eng.planner.busy()
    tk = eng.submit(two(lat), two(mask), two(mlat), two(ctx), 4)
    assert eng.run_until_idle() == [tk]
    ref = D.denoise(unet, D.DPMSolverMultistepScheduler(), two(lat), two(mask), two(mlat), two(ctx), 4)
    out = eng.result(tk)
    D.synchronize()
    assert torch.equal(out, ref)
    eng.close()


# ------------------------------------------------------------------------------------------------ 9. the scalar step entries
# dmx_sched_step_rows is compared with the scalar entries above, and both run one kernel body: here the scalar entries stand against the
# numpy restatement (tests/inflight_restatement.row_update, which the host tests hold to oracle/schedulers.py and tests/dpm_restatement.py),
# bit for bit.  The scalar launcher caps its grid at 2048 blocks of 256 threads; the last size is one full grid of float4s, four more blocks'
# worth and a tail of three, so the grid-stride loop runs and ends in a partial float4.
STEP_GRID_CAP = 2048 * 256
STEP_SIZES = [3, 37, 1024, STEP_GRID_CAP * 4 + 1024 + 3]


@functools.lru_cache(maxsize=1)
def _step_reference(n):
    """inputs (numpy, fp32) and, per case, the restatement's (prev_sample, m0): computed once per size, shared by both builds, only read"""
    import diffute_amd as D
    import inflight_restatement as IR
    from diffute_amd import _cabi
    from diffute_amd.inflight import plan_records
    rng = np.random.default_rng(n)
    data = {k: rng.standard_normal(n).astype(np.float32) for k in ("x", "e", "nz", "m1", "m2", "out", "x0")}
    ddim = plan_records(D.DDIMScheduler(), 10, eta=0.5)[1][2]
    ddpm = plan_records(D.DDPMScheduler(), 10)[1][3]
    assert ddim.use_noise == 1 and ddpm.use_noise == 1 and all(float(v) != 0 for v in list(ddim.c) + list(ddpm.c))
    dpm = plan_records(D.DPMSolverMultistepScheduler(solver_order=3), 10)[1]
    heun = plan_records(D.DPMSolverMultistepScheduler(solver_order=2, solver_type="heun"), 5)[1][1]
    assert [dpm[i].order for i in range(3)] == [1, 2, 3] and heun.order == 2
    cases = []                          # (name, kind, record, noise given)
    for noise in (True, False):
        cases += [("ddim", _cabi.SCHED_DDIM, ddim, noise), ("ddpm", _cabi.SCHED_DDPM, ddpm, noise)]
    cases += [(f"dpm{i + 1}", _cabi.SCHED_DPMPP, dpm[i], False) for i in range(3)] + [("dpm2heun", _cabi.SCHED_DPMPP, heun, False)]
    want = {}
    for name, kind, rec, noise in cases:
        for vpred in (0, 1):
            m1 = data["m1"] if rec.order >= 2 else None
            m2 = data["m2"] if rec.order >= 3 else None
            want[(name, noise, vpred)] = IR.row_update(kind, rec, data["x"], data["e"], data["nz"] if noise else None, m1, m2, bool(vpred))
    for v in data.values():
        v.setflags(write=False)
    return data, cases, want


@pytest.mark.parametrize("n,build", [(n, b) for n in STEP_SIZES for b in ("bf16", "fp16")])
def test_scalar_step_entries_equal_the_restatement(cuda, n, build):
    """Every case of every scalar entry, per size: all pointers aligned / all one float past a 16-byte boundary / exactly one operand
    misaligned (the noise, else eps, for DDIM and DDPM; for DPM-Solver++ the oldest operand its order reads: x0_out, m1, m2); in place and
    out of place; noise given and NULL; both prediction types; orders 1, 2, 3 (midpoint) and 2 (heun).  The whole of every buffer - guard
    bands, inputs, operands an order does not read - is compared bit for bit."""
    from diffute_amd import _cabi
    lib = _cabi.lib(build)
    st = _cabi.current_stream()
    data, cases, want = _step_reference(n)
    dev_data = {k: torch.from_numpy(v.copy()).to(cuda) for k, v in data.items()}
    for name, kind, rec, noise in cases:
        dpm = kind == _cabi.SCHED_DPMPP
        odd = ("x0", "m1", "m2")[rec.order - 1] if dpm else ("nz" if noise else "e")
        for vpred in (0, 1):
            prev, m0 = want[(name, noise, vpred)]
            prev_dev = torch.from_numpy(prev).to(cuda)
            m0_dev = torch.from_numpy(m0).to(cuda) if dpm else None
            for align in ("all0", "all1", "one"):
                for inplace in (True, False):
                    off = {k: (1 if align == "all1" or (align == "one" and k == odd) else 0) for k in dev_data}
                    bufs = {k: _guarded(n, off[k], cuda, None, dev_data[k]) for k in dev_data}
                    expect = {k: b.clone() for k, (b, _) in bufs.items()}
                    view = {k: v for k, (_, v) in bufs.items()}
                    out_key = "x" if inplace else "out"
                    expect[out_key][GUARD + off[out_key]:GUARD + off[out_key] + n] = prev_dev
                    if dpm:
                        expect["x0"][GUARD + off["x0"]:GUARD + off["x0"] + n] = m0_dev
                        rc = lib.dmx_sched_step_dpmpp(_cabi.ptr(view["x"]), _cabi.ptr(view["e"]), _cabi.ptr(view["m1"]) if rec.order >= 2 else None,
                                                      _cabi.ptr(view["m2"]) if rec.order >= 3 else None, _cabi.ptr(view["x0"]), _cabi.ptr(view[out_key]),
                                                      n, rec.order, rec.dpm, vpred, st)
                    else:
                        fn = lib.dmx_sched_step_ddim if kind == _cabi.SCHED_DDIM else lib.dmx_sched_step_ddpm
                        rc = fn(_cabi.ptr(view["x"]), _cabi.ptr(view["e"]), _cabi.ptr(view["nz"]) if noise else None, _cabi.ptr(view[out_key]), n,
                                *[float(v) for v in rec.c], vpred, st)
                    _cabi.check(rc, name, lib)
                    for k, (b, _) in bufs.items():
                        bad = (_bits(b) != _bits(expect[k])).nonzero()
                        assert bad.numel() == 0, (f"{name} n {n} vpred {vpred} noise {noise} {align} {'in place' if inplace else 'out of place'}: buffer {k!r} "
                                                  f"differs at {bad.numel()} floats, first {int(bad[0]) - GUARD - off[k]} (guard excluded)")
    _cabi.poll_device_error(lib)


# ------------------------------------------------------------------------------------------------ 10. denoise() reaches the same entries
# recorded on the commit before the denoise paths were unified (same recorder, same inputs, both builds alike): the table of the loop's
# timesteps, the context, then per step one graph forward with its table set and unset around it and one scheduler entry
DENOISE_CALLS = {
    "ddim_eta0": [
        "dmx_unet_temb_table_floats", "dmx_unet_temb_table_workspace_bytes", "dmx_unet_temb_table", "dmx_unet_context_bytes",
        "dmx_unet_workspace_bytes", "dmx_unet_set_context", "dmx_plan_epoch", "dmx_unet_workspace_bytes", "dmx_unet_use_temb_table",
        "dmx_unet_forward_graph", "dmx_unet_use_temb_table", "dmx_sched_step_ddim", "dmx_plan_epoch", "dmx_unet_use_temb_table",
        "dmx_unet_forward_graph", "dmx_unet_use_temb_table", "dmx_sched_step_ddim", "dmx_plan_epoch", "dmx_unet_use_temb_table",
        "dmx_unet_forward_graph", "dmx_unet_use_temb_table", "dmx_sched_step_ddim"
    ],
    "ddim_eta05": [
        "dmx_unet_temb_table_floats", "dmx_unet_temb_table_workspace_bytes", "dmx_unet_temb_table", "dmx_unet_context_bytes",
        "dmx_unet_workspace_bytes", "dmx_unet_set_context", "dmx_plan_epoch", "dmx_unet_workspace_bytes", "dmx_unet_use_temb_table",
        "dmx_unet_forward_graph", "dmx_unet_use_temb_table", "dmx_sched_step_ddim", "dmx_plan_epoch", "dmx_unet_use_temb_table",
        "dmx_unet_forward_graph", "dmx_unet_use_temb_table", "dmx_sched_step_ddim", "dmx_plan_epoch", "dmx_unet_use_temb_table",
        "dmx_unet_forward_graph", "dmx_unet_use_temb_table", "dmx_sched_step_ddim"
    ],
    "ddpm": [
        "dmx_unet_temb_table_floats", "dmx_unet_temb_table_workspace_bytes", "dmx_unet_temb_table", "dmx_unet_context_bytes",
        "dmx_unet_workspace_bytes", "dmx_unet_set_context", "dmx_plan_epoch", "dmx_unet_workspace_bytes", "dmx_unet_use_temb_table",
        "dmx_unet_forward_graph", "dmx_unet_use_temb_table", "dmx_sched_step_ddpm", "dmx_plan_epoch", "dmx_unet_use_temb_table",
        "dmx_unet_forward_graph", "dmx_unet_use_temb_table", "dmx_sched_step_ddpm", "dmx_plan_epoch", "dmx_unet_use_temb_table",
        "dmx_unet_forward_graph", "dmx_unet_use_temb_table", "dmx_sched_step_ddpm"
    ],
    "dpmpp2": [
        "dmx_unet_temb_table_floats", "dmx_unet_temb_table_workspace_bytes", "dmx_unet_temb_table", "dmx_unet_context_bytes",
        "dmx_unet_workspace_bytes", "dmx_unet_set_context", "dmx_plan_epoch", "dmx_unet_workspace_bytes", "dmx_unet_use_temb_table",
        "dmx_unet_forward_graph", "dmx_unet_use_temb_table", "dmx_sched_step_dpmpp", "dmx_plan_epoch", "dmx_unet_use_temb_table",
        "dmx_unet_forward_graph", "dmx_unet_use_temb_table", "dmx_sched_step_dpmpp", "dmx_plan_epoch", "dmx_unet_use_temb_table",
        "dmx_unet_forward_graph", "dmx_unet_use_temb_table", "dmx_sched_step_dpmpp"
    ],
}


@pytest.mark.parametrize("case", ["ddim_eta0", "ddim_eta05", "ddpm", "dpmpp2"])
def test_denoise_makes_the_same_calls(cuda, tiny_unet, case, monkeypatch):
    import diffute_amd as D
    from diffute_amd import _cabi
    from diffute_amd.synthetic import synth_inputs
    from test_prepost_pages_gpu import _Recorder
    lat, mask, mlat, ctx = synth_inputs(2, 16, 16, 77, 128, device=cuda)
    sched, eta = {"ddim_eta0": (D.DDIMScheduler(), 0.0), "ddim_eta05": (D.DDIMScheduler(), 0.5), "ddpm": (D.DDPMScheduler(), 0.0),
                  "dpmpp2": (D.DPMSolverMultistepScheduler(solver_order=2), 0.0)}[case]
    tiny_unet._ensure_packed()
    tiny_unet._slots.pop(0, None)                    # the loop's execution slot starts empty, whatever ran before
    names, real = [], _cabi.lib
    monkeypatch.setattr(_cabi, "lib", lambda elem="bf16": _Recorder(real(elem), names))      # (unet._lib is _cabi.lib(the model's build))
    out = D.denoise(tiny_unet, sched, lat, mask, mlat, ctx, 3, eta=eta)
    monkeypatch.undo()
    D.synchronize()
    assert torch.isfinite(out).all()
    assert names == DENOISE_CALLS[case], f"{case}: {names}"


# ------------------------------------------------------------------------------------------------ 11. the workspace query
WORKSPACE_BYTES = [284672, 8722432]      # (B, H, W, ctx_len) = (1, 8, 8, 5), (3, 16, 16, 77), either build, recorded on that commit too


def test_workspace_bytes_unchanged(cuda, tiny_unet):
    """dmx_unet_workspace_bytes covers the forward and the context projection (whose dry walk is the projection's own function): the values
    recorded before the two were unified"""
    tiny_unet._ensure_packed()
    got = [int(tiny_unet._lib.dmx_unet_workspace_bytes(tiny_unet._h, *shape)) for shape in ((1, 8, 8, 5), (3, 16, 16, 77))]
    assert got == WORKSPACE_BYTES, got



# ------------------------------------------------------------------------------------------------ 12. temb fetch, scalar form
def test_temb_scalar_form_equals_explicit_timestep(cuda, tiny_unet):
    """forward_parts(..., temb=(table, step index)) is forward_parts with that step's timestep, bit for bit: eager, and through the graph
    path, whose third call is a replay (it reads a step index changed on the device in between).  A per-row call on the same slot and
    buffers then runs its own walk: it writes the timesteps the scalar form never writes, and equals the explicit per-row timesteps."""
    import diffute_amd as D
    from diffute_amd.inflight import plan_records
    from diffute_amd.synthetic import synth_inputs
    ts, recs = plan_records(D.DDIMScheduler(), 4)
    table = tiny_unet.temb_table(torch.tensor(ts, dtype=torch.int64, device=cuda))
    plan = _upload_plan(recs, cuda)
    for B in (3, 1):          # B = 1: the two forms take the same t_count, buffers and index tensor - only the plan tells their graph keys apart
        lat, mask, mlat, ctx = synth_inputs(B, 16, 16, 77, 128, device=cuda)
        parts = [lat, mask, mlat]
        slot = f"t12_{B}"
        tiny_unet.set_context(ctx, slot=slot)
        explicit = {i: tiny_unet.forward_parts(parts, torch.tensor([ts[i]], dtype=torch.int64, device=cuda), slot=slot).clone() for i in (1, 2)}
        tbuf = torch.full((B,), -7, dtype=torch.int64, device=cuda)
        index = torch.full((B,), 2, dtype=torch.int32, device=cuda)
        eager = tiny_unet.forward_parts(parts, tbuf[:1], slot=slot, temb=(table, index[:1])).clone()
        assert torch.equal(eager, explicit[2])
        side = torch.cuda.Stream(device=cuda)
        side.wait_stream(torch.cuda.current_stream(cuda))
        with torch.cuda.stream(side):
            out = torch.empty_like(eager)
            for call, i in enumerate((2, 2, 1)):                 # seen, captured, replayed
                index.fill_(i)
                tiny_unet.forward_parts(parts, tbuf[:1], out=out, graph=True, slot=slot, temb=(table, index[:1]))
                assert torch.equal(out, explicit[i]), f"B {B} graph call {call}"
            assert tbuf.tolist() == [-7] * B                     # the scalar form leaves the timesteps alone
            rows = list(range(B))                                # row b on step b
            index.copy_(torch.tensor(rows, dtype=torch.int32, device=cuda))
            tiny_unet.forward_parts(parts, tbuf, out=out, graph=True, slot=slot, temb=(table, index, plan))
            assert tbuf.tolist() == [ts[i] for i in rows], "the per-row call did not run its own walk (a replay of the scalar graph?)"
            want = tiny_unet.forward_parts(parts, torch.tensor([ts[i] for i in rows], dtype=torch.int64, device=cuda), slot=slot)
            assert torch.equal(out, want)
        torch.cuda.current_stream(cuda).wait_stream(side)
        D.synchronize()
        tiny_unet._slots.pop(slot)
