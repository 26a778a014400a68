"""In-flight batching with classifier-free guidance on the GPU (include/diffute_hip.h dmx_sched_step_rows_guided / dmx_rows_guide,
diffute_amd/inflight.py DenoiseEngine.submit(guidance=)): the per-row guided step against the entries it is made of - every pair
dmx_sched_step_guided on that pair alone, the plain row dmx_sched_step_rows, bit for bit, everything else untouched -, its refusals, the
guide-table writer, and the engine against denoise(guidance=), against itself with neighbours, and against today's engine where the
guidance is inactive.  The numpy restatement of the step is held to the same properties on the CPU (tests/test_inflight_guided_host.py)."""
import ctypes

import numpy as np
import pytest
import torch

from test_guidance_gpu import _launches
from test_inflight_gpu import GUARD, SENT, TINY_UNET, _bits, _copy_rec, _guarded, _upload_plan

pytestmark = pytest.mark.gpu
ERR_ARG = -1
PLAIN, COND, UNCOND = 0, 1, 2


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


def _row(role=PLAIN, partner=-1, scale=1.0, rescale=0.0):
    """a guide entry as dmx_rows_guide writes it (PLAIN: the all-zero entry)"""
    from diffute_amd import _cabi
    if role == PLAIN:
        return _cabi.GuideRow()
    return _cabi.GuideRow(role=role, partner=partner, scale=scale, rescale=rescale, one_minus_rescale=float(1 - rescale))


def _table(entries, dev):
    return torch.frombuffer(bytearray(b"".join(bytes(e) for e in entries)), dtype=torch.uint8).to(dev)


def _sentinels(n, dev):
    """n sentinel floats inside sentinel guard bands -> (whole buffer, view)"""
    buf = torch.full((GUARD + n + GUARD,), SENT, dtype=torch.int32, device=dev).view(torch.float32)
    return buf, buf[GUARD:GUARD + n]


def _differs(a, b):
    return (_bits(a) != _bits(b)).nonzero()


# ------------------------------------------------------------------------------------------------ 1. the entry against the existing entries
def _pair_alone(lib, dev, kind, rec, x_b, ec, eu, nz_b, hist_b, scale, rescale, vpred, align):
    """dmx_sched_step_guided at B = 1 on copies of one pair: the sample row duplicated (clean), the model outputs `align` floats past a
    16-byte boundary like the rows they are copies of (the ratio's summation order follows the alignment of its two inputs)
    -> (sample' [2, per], hist' [3, 1, per] or None, ratio [1])"""
    from diffute_amd import _cabi
    per = x_b.numel()
    s = torch.cat([x_b, x_b]).clone()
    _, e = _guarded(2 * per, align, dev, None, torch.cat([ec, eu]))
    n = nz_b.clone() if nz_b is not None and rec.use_noise else None
    h = hist_b.clone().reshape(hist_b.shape[0], 1, per).contiguous() if hist_b is not None else None
    k = torch.full((1,), float("nan"), device=dev)
    rc = lib.dmx_sched_step_guided(_cabi.ptr(s), _cabi.ptr(e), _cabi.ptr(n), _cabi.ptr(h), 0 if h is None else h.shape[0], rec, kind, vpred,
                                   float(scale), float(rescale), float(1 - rescale), _cabi.ptr(k), 1, per, _cabi.current_stream())
    _cabi.check(rc, "sched_step_guided", lib)
    return s.view(2, per), h, k


PAIRS = ((0, 1, 7.5, 0.7), (2, 3, 3.0, 0.0))              # (conditional row, unconditional row, scale, rescale)


def _entry_case(lib, dev, kind, per, recs, plan_rows, vpred, offset, seed, n_hist=0):
    """one launch over B = 6 rows - the pair (0, 1) at scale 7.5 with rescale 0.7, the pair (2, 3) at scale 3.0 on another plan row, a PLAIN
    row and an idle row whose guide entry says COND - vs each pair through dmx_sched_step_guided alone and the plain row through
    dmx_sched_step_rows alone.  The whole of every guarded buffer is compared bit for bit with what it should hold: the idle row, the
    unconditional rows' noise and history slices, the history slots no record writes, ratio_out of the rows without a rescale, the guard
    bands.  The unconditional sample rows (and noise rows) hold NaN beforehand; a second run from the same inputs gives the same bits."""
    from diffute_amd import _cabi
    from diffute_amd.schedulers import launch_step_rows_guided
    B, dpm = 6, kind == _cabi.SCHED_DPMPP
    iA, iB, iP = plan_rows
    idx = [iA, iA, iB, iB, iP, -1]
    guide = _table([_row(COND, 1, 7.5, 0.7), _row(UNCOND, 0, 7.5, 0.7), _row(COND, 3, 3.0), _row(UNCOND, 2, 3.0), _row(), _row(COND, 0, 7.5, 0.7)], dev)
    gen = torch.Generator().manual_seed(seed)
    st = _cabi.current_stream()
    nh = max(n_hist, 1)
    xb, x = _guarded(B * per, offset, dev, gen)
    eb, e = _guarded(B * per, offset, dev, gen)
    nb, nz = _guarded(B * per, offset, dev, gen)
    hb, h = _guarded(nh * B * per, offset, dev, gen)
    rb, ratio = _sentinels(B, dev)
    xr, er, nr, hr = x.view(B, per), e.view(B, per), nz.view(B, per), h.view(nh, B, per)
    for p in (1, 3):
        xr[p] = float("nan"); nr[p] = float("nan")
    x_in, h_in, r_in = xb.clone(), hb.clone(), rb.clone()
    want_x, want_h, want_r = xb.clone(), hb.clone(), rb.clone()
    wx = want_x[GUARD + offset:GUARD + offset + B * per].view(B, per)
    wh = want_h[GUARD + offset:GUARD + offset + nh * B * per].view(nh, B, per)
    wr = want_r[GUARD:GUARD + B]
    e_keep, n_keep = eb.clone(), nb.clone()
    for b, p, scale, rescale in PAIRS:
        r = recs[idx[b]]
        s, hh, k = _pair_alone(lib, dev, kind, r, xr[b], er[b], er[p], None if dpm else nr[b], hr[:, b] if dpm else None, scale, rescale, vpred,
                               (offset + b * per) % 4)
        wx[b].copy_(s[0]); wx[p].copy_(s[1])
        if dpm:
            wh[r.ring_w, b].copy_(hh[r.ring_w, 0])
        if rescale:
            wr[b] = k[0]
    r = recs[iP]
    xs, es, ns, hs = xr[4:5].clone(), er[4:5].clone(), None if dpm else nr[4:5].clone(), hr[:, 4:5].clone().contiguous() if dpm else None
    plan = _upload_plan(recs, dev)
    _cabi.check(lib.dmx_sched_step_rows(_cabi.ptr(xs), _cabi.ptr(es), _cabi.ptr(ns), _cabi.ptr(hs), n_hist, _cabi.ptr(plan),
                                        _cabi.ptr(torch.tensor([iP], dtype=torch.int32, device=dev)), 1, per, kind, vpred, st), "sched_step_rows", lib)
    wx[4].copy_(xs[0])
    if dpm:
        wh[r.ring_w, 4].copy_(hs[r.ring_w, 0])
    assert torch.isfinite(wx[:5]).all()
    row_index = torch.tensor(idx, dtype=torch.int32, device=dev)
    what = f"kind {kind} per {per} vpred {vpred} offset {offset} plan rows {plan_rows}"
    for run in range(2):
        if run:
            xb.copy_(x_in); hb.copy_(h_in); rb.copy_(r_in)
        launch_step_rows_guided(kind, xr, er, None if dpm else nr, hr if dpm else None, plan, row_index, guide, vpred, st, ratio_out=ratio, lib=lib)
        torch.cuda.synchronize()
        bad = _differs(xb, want_x)
        assert bad.numel() == 0, f"{what} run {run}: sample buffer differs at {bad.numel()} floats, first {int(bad[0]) - GUARD - offset} (row-major, guard excluded)"
        bad = _differs(hb, want_h)
        assert bad.numel() == 0, f"{what} run {run}: history buffer differs at {bad.numel()} floats, first {int(bad[0]) - GUARD - offset}"
        bad = _differs(rb, want_r)
        assert bad.numel() == 0, f"{what} run {run}: ratio_out differs at {(bad.reshape(-1) - GUARD).tolist()}"
        assert torch.equal(_bits(eb), _bits(e_keep)) and torch.equal(_bits(nb), _bits(n_keep)), f"{what}: an input was written"


@pytest.mark.parametrize("build", ["bf16", "fp16"])
@pytest.mark.parametrize("per", [3, 37, 1024, 4119])
def test_entry_equals_the_existing_entries(cuda, per, build):
    """per 4119 = 4 * 1024 + 20 + 3: some of the block's 1024 threads take a second float4 trip and a scalar tail follows"""
    import diffute_amd as D
    from diffute_amd import _cabi
    from diffute_amd.inflight import plan_records
    lib = _cabi.lib(build)
    ddim = [_copy_rec(r) for r in plan_records(D.DDIMScheduler(), 10, eta=0.5)[1]]
    ddim[7].use_noise = 0                                   # the second pair adds no noise
    _, ddpm = plan_records(D.DDPMScheduler(), 10)           # the last step (t = 0) adds none
    _, dpm = plan_records(D.DPMSolverMultistepScheduler(solver_order=3), 10)
    assert [r.order for r in dpm] == [1, 2, 3, 3, 3, 3, 3, 3, 2, 1]
    for offset in (0, 1):
        for vpred in (0, 1):
            _entry_case(lib, cuda, _cabi.SCHED_DDIM, per, ddim, (2, 7, 5), vpred, offset, seed=per + vpred)
            _entry_case(lib, cuda, _cabi.SCHED_DDPM, per, ddpm, (3, 9, 6), vpred, offset, seed=per + 7 + vpred)
            for rows in ((4, 1, 0), (8, 9, 5), (0, 5, 1)):  # orders (3, 2, 1), (2, 1, 3), (1, 3, 2); every ring position
                _entry_case(lib, cuda, _cabi.SCHED_DPMPP, per, dpm, rows, vpred, offset, seed=per + vpred + rows[0], n_hist=3)
    _cabi.poll_device_error(lib)


# ------------------------------------------------------------------------------------------------ 2. refusals, bad partners, the table writer
def test_refusals_write_nothing(cuda):
    import diffute_amd as D
    from diffute_amd import _cabi
    from diffute_amd.inflight import plan_records
    lib = _cabi.lib()
    B, per = 2, 8
    gen = torch.Generator().manual_seed(0)
    _, recs = plan_records(D.DPMSolverMultistepScheduler(solver_order=3), 10)
    bufs = {"sample": _guarded(B * per, 0, cuda, gen), "eps": _guarded(B * per, 0, cuda, gen), "noise": _guarded(B * per, 0, cuda, gen),
            "hist": _guarded(3 * B * per, 0, cuda, gen), "ratio": _sentinels(B, cuda), "table": _sentinels(5 * 4, cuda)}
    plan = _upload_plan(recs, cuda)
    row_index = torch.tensor([4, 4], dtype=torch.int32, device=cuda)
    guide = _table([_row(COND, 1, 3.0, 0.5), _row(UNCOND, 0, 3.0, 0.5)], cuda)
    before = {k: b.clone() for k, (b, _) in bufs.items()}
    st = _cabi.current_stream()
    P = _cabi.ptr

    def step(**kw):
        a = dict(sample=bufs["sample"][1], eps=bufs["eps"][1], noise=None, hist=bufs["hist"][1], n_hist=3, plan=plan, row_index=row_index, guide=guide,
                 ratio=bufs["ratio"][1], B=B, per=per, kind=_cabi.SCHED_DPMPP, vpred=0)
        a.update(kw)
        return lib.dmx_sched_step_rows_guided(P(a["sample"]), P(a["eps"]), P(a["noise"]), P(a["hist"]), a["n_hist"], P(a["plan"]), P(a["row_index"]),
                                              P(a["guide"]), P(a["ratio"]), a["B"], a["per"], a["kind"], a["vpred"], st)
    ddim = dict(kind=_cabi.SCHED_DDIM, hist=None, n_hist=0)
    bad = {
        "B = 0": dict(B=0), "B < 0": dict(B=-2), "per_sample 0": dict(per=0), "per_sample 1": dict(per=1), "per_sample 1, DDIM": dict(per=1, **ddim),
        "NULL sample": dict(sample=None), "NULL model_output": dict(eps=None), "NULL plan": dict(plan=None), "NULL row_index": dict(row_index=None),
        "NULL guide": dict(guide=None), "NULL guide, DDIM": dict(guide=None, **ddim), "kind 3": dict(kind=3), "kind -1": dict(kind=-1),
        "dpm with noise": dict(noise=bufs["noise"][1]), "dpm without a ring": dict(hist=None), "n_hist 0": dict(n_hist=0), "n_hist 4": dict(n_hist=4),
    }
    for what, kw in bad.items():
        assert step(**kw) == ERR_ARG, what
        assert lib.dmx_last_error()
    nan, inf = float("nan"), float("inf")
    table = bufs["table"][1]
    ok_guide = dict(guide=table, b0=0, n=1, guided=1, scale=3.0, rescale=0.5, omr=0.5)
    bad_guide = {
        "NULL guide": dict(guide=None), "b0 < 0": dict(b0=-1), "n = 0": dict(n=0), "n < 0": dict(n=-3), "guided 2": dict(guided=2), "guided -1": dict(guided=-1),
        "scale NaN": dict(scale=nan), "scale inf": dict(scale=inf), "rescale NaN": dict(rescale=nan), "rescale < 0": dict(rescale=-0.1),
        "rescale > 1": dict(rescale=1.5), "1 - rescale inf": dict(omr=-inf), "1 - rescale NaN": dict(omr=nan), "PLAIN with a NaN scale": dict(guided=0, scale=nan),
    }
    for what, kw in bad_guide.items():
        a = dict(ok_guide); a.update(kw)
        assert lib.dmx_rows_guide(P(a["guide"]), a["b0"], a["n"], a["guided"], a["scale"], a["rescale"], a["omr"], st) == ERR_ARG, what
        assert lib.dmx_last_error()
    torch.cuda.synchronize()
    for k, (b, _) in bufs.items():
        assert torch.equal(_bits(b), _bits(before[k])), f"a refused call wrote to {k}"
    # ... and the same buffers are accepted once the arguments are right
    assert step() == 0 and step(noise=bufs["noise"][1], **ddim) == 0
    torch.cuda.synchronize()
    assert not torch.equal(_bits(bufs["sample"][0]), _bits(before["sample"]))
    for k, (b, v) in bufs.items():
        lo = GUARD
        assert torch.equal(_bits(b[:lo]), _bits(before[k][:lo])) and torch.equal(_bits(b[lo + v.numel():]), _bits(before[k][lo + v.numel():])), k
    _cabi.poll_device_error(lib)


def test_rows_guide_writes_its_rows_only(cuda):
    from diffute_amd import _cabi
    lib = _cabi.lib()
    st = _cabi.current_stream()
    n_rows, words = 8, ctypes.sizeof(_cabi.GuideRow) // 4
    buf, view = _sentinels(n_rows * words, cuda)
    want = buf.clone()
    wv = want[GUARD:GUARD + n_rows * words].view(torch.int32).view(n_rows, words)

    def put(b, entry):
        wv[b].copy_(torch.frombuffer(bytearray(bytes(entry)), dtype=torch.int32))
    _cabi.check(lib.dmx_rows_guide(_cabi.ptr(view), 1, 2, 1, 7.5, 0.7, float(1 - 0.7), st), "rows_guide", lib)
    _cabi.check(lib.dmx_rows_guide(_cabi.ptr(view), 6, 1, 0, 9.0, 0.5, 0.5, st), "rows_guide", lib)
    for b in (1, 2):
        put(b, _row(COND, b + 2, 7.5, 0.7)); put(b + 2, _row(UNCOND, b, 7.5, 0.7))
    put(6, _row())
    torch.cuda.synchronize()
    assert torch.equal(_bits(buf), _bits(want)), "rows [1, 5) as two pairs, row 6 PLAIN, rows 0, 5, 7 and the guard bands untouched"
    _cabi.check(lib.dmx_rows_guide(_cabi.ptr(view), 1, 4, 0, 1.0, 0.0, 1.0, st), "rows_guide", lib)      # what the engine does when the request leaves
    for b in range(1, 5):
        put(b, _row())
    torch.cuda.synchronize()
    assert torch.equal(_bits(buf), _bits(want))


def test_rows_that_cannot_be_served_are_left_alone(cuda):
    """one launch: a good pair (rows 0, 1) and eight pairs the step cannot serve; each of those keeps its sample, noise and history bits"""
    import diffute_amd as D
    from diffute_amd import _cabi
    from diffute_amd.inflight import plan_records
    from diffute_amd.schedulers import launch_step_rows_guided
    lib = _cabi.lib()
    recs = [_copy_rec(r) for r in plan_records(D.DPMSolverMultistepScheduler(solver_order=3), 10)[1]]
    bad_ring = _copy_rec(recs[4]); bad_ring.ring_w = 3
    recs.append(bad_ring)                                   # plan row 10
    B, per, kind = 18, 37, _cabi.SCHED_DPMPP
    entries = [_row(COND, 1, 7.5, 0.7), _row(UNCOND, 0, 7.5, 0.7),
               _row(COND, B, 3.0), _row(UNCOND, 2, 3.0),            # the partner is outside the batch
               _row(COND, 4, 3.0), _row(UNCOND, 4, 3.0),            # ... is the row itself
               _row(COND, 7, 3.0), _row(UNCOND, 6, 3.0),            # ... is on another plan row
               _row(COND, 9, 3.0), _row(COND, 8, 3.0),              # ... is not UNCOND
               _row(COND, 11, 3.0), _row(7, 10, 3.0),               # ... has a role outside the enum
               _row(COND, 13, 3.0), _row(UNCOND, 12, 3.0),          # a record the ring cannot serve
               _row(COND, -1, 3.0), _row(UNCOND, 14, 3.0),          # the partner is negative
               _row(COND, 17, 3.0), _row(UNCOND, 0, 3.0)]           # the partner names another row
    idx = [4] * B
    idx[7], idx[12], idx[13] = 5, 10, 10
    gen = torch.Generator().manual_seed(11)
    xb, x = _guarded(B * per, 0, cuda, gen)
    eb, e = _guarded(B * per, 0, cuda, gen)
    hb, h = _guarded(3 * B * per, 0, cuda, gen)
    rb, ratio = _sentinels(B, cuda)
    xr, er, hr = x.view(B, per), e.view(B, per), h.view(3, B, per)
    want_x, want_h, want_r, e_keep, x_in = xb.clone(), hb.clone(), rb.clone(), eb.clone(), xb.clone()
    s, hh, k = _pair_alone(lib, cuda, kind, recs[4], xr[0], er[0], er[1], None, hr[:, 0], 7.5, 0.7, 0, 0)
    want_x[GUARD:GUARD + 2 * per].copy_(s.reshape(-1))
    want_h[GUARD:GUARD + 3 * B * per].view(3, B, per)[recs[4].ring_w, 0].copy_(hh[recs[4].ring_w, 0])
    want_r[GUARD] = k[0]
    launch_step_rows_guided(kind, xr, er, None, hr, _upload_plan(recs, cuda), torch.tensor(idx, dtype=torch.int32, device=cuda), _table(entries, cuda), 0,
                            _cabi.current_stream(), ratio_out=ratio, lib=lib)
    torch.cuda.synchronize()
    bad = _differs(xb, want_x)
    assert bad.numel() == 0, f"sample rows {sorted(set(((bad.reshape(-1) - GUARD) // per).tolist()))} differ"
    bad = _differs(hb, want_h)
    assert bad.numel() == 0, f"history differs at {bad.numel()} floats, first {int(bad[0]) - GUARD}"
    assert torch.equal(_bits(rb), _bits(want_r)) and torch.equal(_bits(eb), _bits(e_keep))
    assert not torch.equal(_bits(want_x), _bits(x_in)) and torch.equal(_bits(xr[0]), _bits(xr[1]))      # (the good pair was updated)
    _cabi.poll_device_error(lib)


# ------------------------------------------------------------------------------------------------ 3. a filled engine is denoise(guidance=)
def _make(sched):
    import diffute_amd as D
    return {"ddim": D.DDIMScheduler, "ddpm": D.DDPMScheduler, "dpmpp": D.DPMSolverMultistepScheduler}[sched]


def _uncond(cuda, n=2):
    from diffute_amd.init import normal
    return normal(2, 29, n * 77 * 128, cuda).reshape(n, 77, 128)


@pytest.mark.parametrize("rescale", [0.0, 0.7])
@pytest.mark.parametrize("sched", ["ddim", "ddpm", "dpmpp"])
def test_filled_engine_equals_guided_denoise(cuda, tiny_unet, sched, rescale):
    import diffute_amd as D
    from diffute_amd.init import normal
    from diffute_amd.synthetic import synth_inputs
    lat, mask, mlat, ctx = synth_inputs(2, 16, 16, 77, 128, device=cuda)
    g = D.Guidance(7.5, rescale=0.7, uncond=_uncond(cuda)) if rescale else D.Guidance(7.5)
    nz = normal(3, 31, 4 * 2 * 4 * 16 * 16, cuda).reshape(4, 2, 4, 16, 16) if sched == "ddpm" else None
    ref = D.denoise(tiny_unet, _make(sched)(), lat, mask, mlat, ctx, 4, variance_noise=nz, guidance=g).clone()
    eng = D.DenoiseEngine(tiny_unet, _make(sched)(), capacity=4, latent_shape=(4, 16, 16), ctx_len=77)
    tk = eng.submit(lat, mask, mlat, ctx, 4, variance_noise=nz, guidance=g)
    assert eng.planner.running[tk][:2] == (0, 4)
    done = [eng.tick() for _ in range(4)]
    assert done == [[], [], [], [tk]] and not eng.planner.busy()
    out = eng.result(tk)
    D.synchronize()
    assert out.shape == lat.shape and torch.equal(out, ref), f"{sched} rescale {rescale}: max abs diff {float((out - ref).abs().max()):.3e}"
    assert not torch.equal(out, D.denoise(tiny_unet, _make(sched)(), lat, mask, mlat, ctx, 4, variance_noise=nz))
    assert bool((eng.guide == 0).all()) and bool((eng.x == 0).all())       # the rows went back to PLAIN, zeroed
    eng.close()


# ------------------------------------------------------------------------------------------------ 4. rows do not interact
def test_guided_rows_do_not_interact(cuda, tiny_unet):
    import diffute_amd as D
    from diffute_amd.inflight import Planner
    from diffute_amd.synthetic import synth_inputs
    A = synth_inputs(1, 16, 16, 77, 128, device=cuda, seed=0)
    W = synth_inputs(6, 16, 16, 77, 128, device=cuda, seed=20)
    Pq = synth_inputs(1, 16, 16, 77, 128, device=cuda, seed=30)
    Cq = synth_inputs(1, 16, 16, 77, 128, device=cuda, seed=40)
    gA, gC = D.Guidance(7.5), D.Guidance(3.0, rescale=0.7, uncond=_uncond(cuda, 1))
    eng = D.DenoiseEngine(tiny_unet, D.DDIMScheduler(), capacity=6, latent_shape=(4, 16, 16), ctx_len=77)
    w = eng.submit(*W, 1)                          # every slot has held another context before
    assert eng.run_until_idle() == [w]
    # A alone in rows 0-1
    a1 = eng.submit(*A, 4, guidance=gA)
    assert eng.planner.running[a1][:2] == (0, 2)
    assert eng.run_until_idle() == [a1]
    a_alone = eng.result(a1).clone()
    # the plain request alone in slot 2: rows 0-1 are held back from the planner (idle, nobody's) while it is admitted
    eng.planner.owner[0] = eng.planner.owner[1] = "held"
    p1 = eng.submit(*Pq, 3)
    eng.planner.owner[0] = eng.planner.owner[1] = None
    assert eng.planner.running[p1][:2] == (2, 1)
    assert eng.run_until_idle() == [p1]
    p_alone = eng.result(p1).clone()
    # together: A in rows 0-1 again, the plain 3-step request joins at tick 1, a guided 2-step one (another scale, a rescale) at tick 2
    pl = Planner(6)                                # the prediction: the same script through a planner of its own
    script = {0: [("a", A, 4, gA)], 1: [("p", Pq, 3, None)], 2: [("c", Cq, 2, gC)]}
    tickets, names, predicted, got, slots = {}, {}, {}, {}, {}
    for tick in range(4):
        for name, q, T, g in script.get(tick, []):
            tickets[name] = eng.submit(*q, T, guidance=g)
            names[pl.submit(1 if g is None else 2, T, 0)] = name
            slots[name] = eng.planner.running[tickets[name]][:2]
        pl.admit()
        for t in pl.advance():
            predicted[names[t]] = tick
        for t in eng.tick():
            got[[k for k, v in tickets.items() if v == t][0]] = tick
    assert slots == {"a": (0, 2), "p": (2, 1), "c": (3, 2)}
    assert predicted == {"a": 3, "p": 3, "c": 3} and got == predicted and not eng.planner.busy()
    a2, p2, c2 = (eng.result(tickets[k]) for k in "apc")
    D.synchronize()
    assert torch.equal(a2, a_alone), f"A changed with neighbours: max abs diff {float((a2 - a_alone).abs().max()):.3e}"
    assert torch.equal(p2, p_alone), f"the plain request changed beside guided rows: max abs diff {float((p2 - p_alone).abs().max()):.3e}"
    assert c2.shape == (1, 4, 16, 16) and all(torch.isfinite(o).all() for o in (a2, p2, c2)) and torch.isfinite(eng.eps).all()
    assert bool((eng.guide == 0).all())
    eng.close()


# ------------------------------------------------------------------------------------------------ 5. inactive guidance is today's engine
def test_inactive_guidance_is_the_plain_engine(cuda, tiny_unet_bf16, monkeypatch):
    import diffute_amd as D
    from diffute_amd import _cabi
    from diffute_amd.synthetic import synth_inputs
    from test_prepost_pages_gpu import _Recorder
    unet = tiny_unet_bf16
    lat, mask, mlat, ctx = synth_inputs(2, 16, 16, 77, 128, device=cuda)
    eng = D.DenoiseEngine(unet, D.DDIMScheduler(), capacity=2, latent_shape=(4, 16, 16), ctx_len=77)      # (a guided request would not even fit)
    tk = eng.submit(lat, mask, mlat, ctx, 3)
    assert eng.run_until_idle() == [tk]
    plain = eng.result(tk).clone()
    names, real = [], _cabi.lib
    monkeypatch.setattr(_cabi, "lib", lambda elem="bf16": _Recorder(real(elem), names))
    outs = []
    for g in (None, D.Guidance(1.0), D.Guidance(1.0, 0.0, uncond=_uncond(cuda))):
        tk = eng.submit(lat, mask, mlat, ctx, 3, guidance=g)
        assert eng.planner.running[tk][:2] == (0, 2)
        assert eng.run_until_idle() == [tk]
        outs.append(eng.result(tk))
    monkeypatch.undo()
    D.synchronize()
    assert all(torch.equal(o, plain) for o in outs)
    assert names.count("dmx_sched_step_rows") == 9 and names.count("dmx_rows_advance") == 9
    assert "dmx_rows_guide" not in names and "dmx_sched_step_rows_guided" not in names
    with pytest.raises(TypeError, match="Guidance"):
        eng.submit(lat, mask, mlat, ctx, 3, guidance=(7.5, 0.0))
    eng.close()


# ------------------------------------------------------------------------------------------------ 6. launches
@pytest.mark.parametrize("graph", [False, True], ids=["eager", "graph"])
def test_a_guided_tick_launches_what_a_plain_tick_launches(cuda, tiny_unet_bf16, graph):
    """the fourth tick of a 6-step run (no admission, nobody finishing, the forward's graph long captured): two plain rows vs a guided pair
    beside a plain row, on one engine"""
    import diffute_amd as D
    from diffute_amd import _cabi
    from diffute_amd.synthetic import synth_inputs
    lib = _cabi.lib()
    Q = [synth_inputs(1, 16, 16, 77, 128, device=cuda, seed=s) for s in (1, 2)]
    eng = D.DenoiseEngine(tiny_unet_bf16, D.DDIMScheduler(), capacity=4, latent_shape=(4, 16, 16), ctx_len=77, use_graph=graph)
    counts = {}
    for name, gs in (("plain", (None, None)), ("guided", (D.Guidance(7.5, rescale=0.7), None))):
        for q, g in zip(Q, gs):
            eng.submit(*q, 6, guidance=g)
        for _ in range(3):
            assert eng.tick() == []
        counts[name], done = _launches(lib, eng.tick)
        assert done == [] and len(eng.run_until_idle()) == 2
    D.synchronize()
    assert sum(counts["guided"]) == sum(counts["plain"]) > 0, counts
    print(f"launches of one tick ({'graph' if graph else 'eager'}): plain rows {sum(counts['plain'])}, with a guided pair {sum(counts['guided'])}")
    eng.close()


# ------------------------------------------------------------------------------------------------ 7. host refusals
def test_host_refusals_leave_the_engine_usable(cuda, tiny_unet_bf16):
    import diffute_amd as D
    from diffute_amd.synthetic import synth_inputs
    unet = tiny_unet_bf16
    lat, mask, mlat, ctx = synth_inputs(2, 16, 16, 77, 128, device=cuda)
    unc = _uncond(cuda)
    eng = D.DenoiseEngine(unet, D.DPMSolverMultistepScheduler(), capacity=2, latent_shape=(4, 16, 16), ctx_len=77)
    one = lambda t: t[:1].contiguous()
    with pytest.raises(ValueError, match="capacity"):
        eng.submit(lat, mask, mlat, ctx, 4, guidance=D.Guidance(7.5))                                     # 2n = 4 rows, capacity 2
    with pytest.raises(ValueError, match="uncond"):
        eng.submit(one(lat), one(mask), one(mlat), one(ctx), 4, guidance=D.Guidance(7.5, uncond=unc[:, :40].contiguous()))
    with pytest.raises(ValueError, match="uncond"):
        eng.submit(one(lat), one(mask), one(mlat), one(ctx), 4, guidance=D.Guidance(7.5, uncond=unc))     # [2,S,D] for one row
    with pytest.raises(ValueError, match="uncond"):
        eng.submit(one(lat), one(mask), one(mlat), one(ctx), 4, guidance=D.Guidance(7.5, uncond=unc[:1].half()))
    with pytest.raises(ValueError, match="deterministic"):
        eng.submit(one(lat), one(mask), one(mlat), one(ctx), 4, variance_noise=torch.zeros(4, 1, 4, 16, 16, device=cuda), guidance=D.Guidance(7.5))
    assert not eng.planner.busy() and not eng._pending and not eng._guided
    g = D.Guidance(7.5, 0.7, unc[:1])
    tk = eng.submit(one(lat), one(mask), one(mlat), one(ctx), 4, guidance=g)
    assert eng.run_until_idle() == [tk]
    ref = D.denoise(unet, D.DPMSolverMultistepScheduler(), one(lat), one(mask), one(mlat), one(ctx), 4, guidance=g)
    out = eng.result(tk)
    D.synchronize()
    assert torch.equal(out, ref), f"max abs diff {float((out - ref).abs().max()):.3e}"
    eng.close()
