"""Classifier-free guidance without a GPU: the restatement of the guided step (tests/guidance_restatement.py) against float64 and against
the mistakes it must see, the recorded floors of the ratio, the Guidance value object and the selection of the plain path, the context
dropout of the training batches, and the new entry in the header."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import guidance_restatement as G
from guidance_floors import FLOORS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# Measured here (test_restatement_against_float64 prints them): eval32 with its own fp32 ratio against ref64, per element relative to the
# row's max |ref64|, the worst over every kind / order / v-prediction / noise / B / per_sample / scale of the cases, rescale 0.7:
#   DDIM 1.57e-6, DDPM 7.4e-7, DPM-Solver++ order 1 / 2 / 3: 2.0e-7 / 1.4e-7 / 2.3e-7
# (DDIM / DDPM at t ~ 500 divide by sqrt(abar_t) ~ 0.5 and scale 7.5 spreads g over several times the row's final range).
# The bound is NOT those figures: each of the at most 25 fp32 ops between (ec, eu, x, m1, m2) and prev_sample rounds by 2^-24 relative to
# its own result, which the guidance scale (<= 7.5) and the records' coefficients (< 2 each) keep within about 8 x the row's max, so
# 25 * 8 * 2^-24 = 1.2e-5 bounds the fp32 formulation; a wrong formula is off by 1e-2 or more (test_injected_faults).
F64_BOUND = 25 * 8 * 2.0 ** -24


def _records():
    """one record per (kind, order): real scalars from the schedulers' own plans"""
    import diffute_amd as D
    ddim = D.DDIMScheduler(); ddim.set_timesteps(50)
    ddpm = D.DDPMScheduler(); ddpm.set_timesteps(50)
    dpm = D.DPMSolverMultistepScheduler(solver_order=3); dpm.set_timesteps(20)
    p = dpm.plan()
    assert [r.order for r in p[:3]] == [1, 2, 3]
    return [("ddim", G.DDIM, ddim.plan(0.5)[24]), ("ddpm", G.DDPM, ddpm.plan()[24]), ("dpm1", G.DPMPP, p[0]), ("dpm2", G.DPMPP, p[1]),
            ("dpm3", G.DPMPP, p[2])]


def _with_noise(rec, on):
    from diffute_amd import _cabi
    r = _cabi.SchedRowRec.from_buffer_copy(bytes(rec))
    r.use_noise = int(on)
    return r


def test_restatement_against_float64():
    worst = {}
    for name, kind, rec in _records():
        for vpred in (False, True):
            for with_noise in ((False,) if kind == G.DPMPP else (False, True)):
                r = _with_noise(rec, with_noise)
                for B in G.BATCHES:
                    for per in G.PER_SAMPLE:
                        x, eps, nz, hist = G.inputs(B, per)
                        for scale in G.SCALES:
                            a = dict(noise=nz if with_noise else None, hist=hist if kind == G.DPMPP else None, scale=scale, rescale=0.7, vpred=vpred)
                            o32, h32, k32 = G.eval32(kind, r, x, eps, **a)
                            o64, h64, k64 = G.ref64(kind, r, x, eps, **a)
                            err = float((np.abs(o32 - o64) / np.abs(o64).max(axis=1, keepdims=True)).max())
                            worst[name] = max(worst.get(name, 0.0), err)
                            assert err < F64_BOUND, (name, vpred, with_noise, B, per, scale, err)
                            assert np.array_equal(o32[:B], o32[B:]) and o32.dtype == np.float32
    print("eval32 vs ref64, per element relative to the row's max:", {k: f"{v:.2e}" for k, v in worst.items()})


def test_recorded_floors_are_what_the_restatement_measures():
    assert sorted(FLOORS) == sorted(G.case_key(B, per, s) for per in G.PER_SAMPLE for B in G.BATCHES for s in G.SCALES)
    for per in G.PER_SAMPLE:
        for B in G.BATCHES:
            for s in G.SCALES:
                got, rec = G.ratio_floor(B, per, s), FLOORS[G.case_key(B, per, s)]
                assert len(got) == len(rec) == B
                assert all(abs(a - b) <= 5e-4 * b + 1e-12 for a, b in zip(got, rec)), (per, B, s, got, rec)      # (3 printed digits)
                assert max(rec) < 1e-6


def _kernel_order_ratio(ec, eu, scale, threads=1024, vector=True):
    """the ratio in a kernel-like summation order - per-thread strided partials (float4 lanes in turn), a butterfly inside each wave of 64,
    the waves in order -, every op fp32: another valid order, which must stay within bound(floor) of float64 as well"""
    f32 = np.float32
    g = G.combine(ec, eu, scale, f32)

    def total(v):
        n = v.size
        acc = np.zeros(threads, dtype=f32)
        n4 = n // 4 if vector else 0
        for i0 in range(0, n4, threads):
            idx = np.arange(i0, min(i0 + threads, n4))
            for lane in range(4):
                acc[:idx.size] = acc[:idx.size] + v[idx * 4 + lane]
        for i0 in range(n4 * 4, n, threads):
            idx = np.arange(i0, min(i0 + threads, n))
            acc[:idx.size] = acc[:idx.size] + v[idx]
        w = acc.reshape(-1, 64).copy()
        o = 32
        while o:
            w = w + w[:, np.arange(64) ^ o]
            o >>= 1
        s = f32(0)
        for p in w[:, 0]:
            s = f32(s + p)
        return s

    def std(v):
        mean = f32(total(v) / f32(v.size))
        d = (v - mean).astype(f32)
        return np.sqrt(f32(total((d * d).astype(f32)) / f32(v.size - 1)))
    return f32(std(ec) / std(g))


@pytest.mark.parametrize("per", [5, 257, 1027, 16384])
def test_a_kernel_like_summation_order_stays_within_the_bound(per):
    for B in G.BATCHES:
        _, eps, _, _ = G.inputs(B, per)
        e64 = eps.astype(np.float64)
        for s in G.SCALES:
            k64 = G.ratios(e64[:B], G.combine(e64[:B], e64[B:], s, np.float64), np.float64)
            for b in range(B):
                for vector in (True, False):
                    k = float(_kernel_order_ratio(eps[b], eps[B + b], s, vector=vector))
                    assert abs(k - k64[b]) <= G.bound(FLOORS[G.case_key(B, per, s)][b]) * abs(k64[b]), (per, B, s, b, vector, k, k64[b])


@pytest.mark.parametrize("fault", G.FAULTS)
def test_injected_faults(fault):
    """each mistake breaks what the GPU test asserts: bit-equality of the outputs (with the reference's own ratio handed in, as the GPU
    test hands the kernel's in) or, for the mistakes that live in the ratio, the ratio bound"""
    B, per, scale = 3, 257, 3.0
    x, eps, nz, hist = G.inputs(B, per)
    in_ratio = fault in ("ratio_inverted", "mixed_bias", "batch_std")
    seen = 0
    for name, kind, rec in _records():
        a = dict(noise=None, hist=hist if kind == G.DPMPP else None, scale=scale, vpred=False)
        for rescale in (0.0, 0.3):
            good, gh, gk = G.eval32(kind, rec, x, eps, rescale=rescale, **a)
            if in_ratio:
                if rescale == 0.0:
                    continue
                _, _, bk = G.eval32(kind, rec, x, eps, rescale=rescale, fault=fault, **a)
                _, _, k64 = G.ref64(kind, rec, x, eps, rescale=rescale, **a)
                for b in range(B):
                    tol = G.bound(FLOORS[G.case_key(B, per, scale)][b]) * abs(k64[b])
                    assert abs(float(gk[b]) - k64[b]) <= tol
                    assert abs(float(bk[b]) - k64[b]) > 10 * tol, (fault, name, b, bk[b], k64[b])
                seen += 1
                continue
            if fault == "rescale_swapped" and rescale == 0.0:
                continue
            bad, bh, _ = G.eval32(kind, rec, x, eps, rescale=rescale, k=gk, fault=fault, **a)
            assert not np.array_equal(bad, good), (fault, name, rescale)
            if fault == "second_half":
                assert np.array_equal(bad[:B], good[:B]) and np.array_equal(bad[B:], x[B:])
            seen += 1
    assert seen >= 5


# ------------------------------------------------------------------------------------------------ Guidance and the plain path
def test_guidance_validation():
    import diffute_amd as D
    from diffute_amd.schedulers import Guidance
    assert D.Guidance is Guidance and "Guidance" in D.__all__
    g = D.Guidance(3.0)
    assert (g.scale, g.rescale, g.uncond, g.active) == (3.0, 0.0, None, True)
    assert not D.Guidance(1.0).active and not D.Guidance(1.0, 0.0).active and D.Guidance(1.0, 0.5).active and D.Guidance(0.0).active
    for bad in (float("nan"), float("inf"), -float("inf")):
        with pytest.raises(ValueError, match="scale"):
            D.Guidance(bad)
    for bad in (-0.1, 1.5, float("nan")):
        with pytest.raises(ValueError, match="rescale"):
            D.Guidance(2.0, bad)
    for bad in (torch.zeros(77, 128), torch.zeros(1, 1, 77, 128), [[0.0]], torch.zeros(0, 77, 128)):
        with pytest.raises(ValueError, match="uncond"):
            D.Guidance(2.0, uncond=bad)
    with pytest.raises(ValueError, match="dtype"):
        D.Guidance(2.0, uncond=torch.zeros(1, 77, 128, dtype=torch.int64))
    ctx = torch.zeros(3, 77, 128)
    D.Guidance(2.0, uncond=torch.zeros(1, 77, 128)).check_context(ctx)
    D.Guidance(2.0, uncond=torch.zeros(3, 77, 128)).check_context(ctx)
    for bad in (torch.zeros(2, 77, 128), torch.zeros(1, 76, 128), torch.zeros(3, 77, 64), torch.zeros(1, 77, 128, dtype=torch.float16)):
        with pytest.raises(ValueError, match="uncond"):
            D.Guidance(2.0, uncond=bad).check_context(ctx)
    # a per-row context follows its rows; a shared one and the zero context are nobody's rows
    u = torch.arange(3 * 2 * 2, dtype=torch.float32).reshape(3, 2, 2)
    g = D.Guidance(2.0, 0.25, u)
    assert torch.equal(g.rows(slice(1, 3)).uncond, u[1:3]) and torch.equal(g.rows([2, 2, 0]).uncond, u[[2, 2, 0]])
    assert (g.rows(slice(1, 3)).scale, g.rows(slice(1, 3)).rescale) == (2.0, 0.25)
    one = D.Guidance(2.0, uncond=u[:1])
    assert one.rows(slice(1, 3)) is one and D.Guidance(2.0).rows([1]).uncond is None
    c = torch.ones(2, 2, 2)
    assert torch.equal(D.Guidance(2.0).uncond_for(c), torch.zeros(2, 2, 2)) and torch.equal(one.uncond_for(c), u[:1].expand(2, -1, -1))


def test_wrong_guidance_is_refused_before_anything_touches_the_device():
    """CPU tensors and no models: every refusal below comes before the first device call (which would raise RuntimeError / AttributeError)"""
    import diffute_amd as D
    lat, mask, ctx = torch.zeros(2, 4, 8, 8), torch.zeros(2, 1, 8, 8), torch.zeros(2, 77, 128)
    with pytest.raises(TypeError, match="Guidance"):
        D.denoise(None, None, lat, mask, lat, ctx, 2, guidance=3.0)
    with pytest.raises(ValueError, match="uncond"):
        D.denoise(None, None, lat, mask, lat, ctx, 2, guidance=D.Guidance(3.0, uncond=torch.zeros(3, 77, 128)))
    with pytest.raises(ValueError, match="uncond"):
        D.edit_latents(None, None, None, None, None, None, ctx, 2, guidance=D.Guidance(3.0, uncond=torch.zeros(1, 77, 64)))
    img = torch.zeros(64, 64, 3, dtype=torch.uint8)
    with pytest.raises(ValueError, match="uncond"):
        D.edit_boxes(None, None, None, img, [(8, 8, 40, 24), (8, 30, 40, 44)], ctx, 2, guidance=D.Guidance(3.0, uncond=torch.zeros(3, 77, 128)))
    with pytest.raises(TypeError, match="Guidance"):
        D.edit_pages(None, None, None, [img], [[(8, 8, 40, 24), (8, 30, 40, 44)]], ctx, 2, guidance=(3.0, 0.0))


@pytest.mark.parametrize("guidance", ["none", "one", "one_zero"])
def test_the_plain_path_never_reaches_the_guided_launch(monkeypatch, guidance):
    """None and Guidance(1.0) / Guidance(1.0, 0.0) build the plain chain: no unconditional rows, launch_step, never launch_step_guided"""
    import diffute_amd as D
    from diffute_amd import _cabi, pipeline
    g = {"none": None, "one": D.Guidance(1.0), "one_zero": D.Guidance(1.0, 0.0, uncond=torch.zeros(1, 3, 8))}[guidance]
    assert pipeline._check_guidance(g, torch.zeros(2, 3, 8)) is None
    calls = []
    monkeypatch.setattr(pipeline, "launch_step", lambda *a: calls.append("plain"))
    monkeypatch.setattr(pipeline, "launch_step_guided", lambda *a, **k: calls.append("guided"))
    monkeypatch.setattr(_cabi, "current_stream", lambda: None)
    run = object.__new__(pipeline._Run)
    run.guidance, run.cache, run.temb_table, run.use_graph, run.slot, run.stream = pipeline._check_guidance(g), None, None, False, 0, None
    run.kind, run.vpred, run.hist = _cabi.SCHED_DDIM, 0, []
    run.x = run.eps = run.m = run.ml = torch.zeros(2, 4, 2, 2)
    run.t_cur, run.ts_dev = torch.zeros(1, dtype=torch.int64), torch.zeros(3, dtype=torch.int64)

    class _U:
        def forward_parts(self, parts, t, **kw):
            assert parts[0].shape[0] == 2            # (no second half)
    run.unet = _U()
    monkeypatch.setattr(torch.cuda, "stream", lambda s: __import__("contextlib").nullcontext())
    run.step(0, _cabi.SchedRowRec(), None)
    assert calls == ["plain"]
    run.guidance = D.Guidance(3.0)
    run.step(0, _cabi.SchedRowRec(), None)
    assert calls == ["plain", "guided"]


def test_launch_step_guided_is_the_only_caller_of_the_entry():
    import inspect
    import diffute_amd
    from diffute_amd import _cabi, schedulers
    assert "dmx_sched_step_guided" in _cabi.exported_symbols()
    assert inspect.getsource(schedulers.launch_step_guided).count("dmx_sched_step_guided") == 2        # (the docstring and the call)
    pkg = os.path.dirname(os.path.abspath(diffute_amd.__file__))
    for f in os.listdir(pkg):
        if f.endswith(".py"):
            n = open(os.path.join(pkg, f)).read().count("dmx_sched_step_guided")
            assert n == (2 if f == "schedulers.py" else 0), f
    restype, argtypes = _cabi._PROTOS["dmx_sched_step_guided"]
    assert restype is ctypes.c_int and len(argtypes) == 15 and argtypes[5] is _cabi.SchedRowRec and ctypes.sizeof(_cabi.SchedRowRec) == 88
    assert not re.search(r"dmx_sched_step_(ddim|ddpm|dpmpp)\b", "dmx_sched_step_guided")


# ------------------------------------------------------------------------------------------------ context dropout
class _Fake:
    """training_batch's two device calls, on the CPU: the crops are not what is under test"""

    def __init__(self, monkeypatch, B):
        from diffute_amd import data
        self.ctx = torch.arange(B * 3 * 4, dtype=torch.float32).reshape(B, 3, 4) + 1.0
        monkeypatch.setattr(data.prepost, "preprocess_pages", lambda *a: dict(image=torch.zeros(B, 1), masked_image=torch.zeros(B, 1), mask=torch.zeros(B, 1)))
        monkeypatch.setattr(data.glyphs, "glyph_contexts", lambda texts, *g: self.ctx.clone())


class _NoDraws:
    def __getattr__(self, name):
        raise AssertionError(f"drop_rng.{name} was touched with context_dropout = 0")


def test_context_dropout_of_a_batch(monkeypatch):
    from diffute_amd import data
    B = 6
    fake = _Fake(monkeypatch, B)
    args = ([None] * B, [None] * B, [None] * B, ["a"] * B, (None, None, None))
    plain = data.training_batch(*args)
    zero = data.training_batch(*args, context_dropout=0.0, drop_rng=_NoDraws())
    assert sorted(plain) == sorted(zero) == ["masked_images", "masks", "ocr_embeddings", "pixel_values"]
    assert all(torch.equal(plain[k], zero[k]) for k in plain) and torch.equal(plain["ocr_embeddings"], fake.ctx)
    full = data.training_batch(*args, context_dropout=1.0, drop_rng=np.random.default_rng(0))
    assert torch.equal(full["ocr_embeddings"], torch.zeros_like(fake.ctx)) and torch.equal(full["pixel_values"], plain["pixel_values"])
    half = data.training_batch(*args, context_dropout=0.5, drop_rng=np.random.default_rng(7))
    drop = np.random.default_rng(7).random(B) < 0.5
    assert 0 < drop.sum() < B
    for b in range(B):
        assert torch.equal(half["ocr_embeddings"][b], torch.zeros(3, 4) if drop[b] else fake.ctx[b])
    with pytest.raises(ValueError, match="drop_rng"):
        data.training_batch(*args, context_dropout=0.5)
    for bad in (-0.1, 1.1, float("nan")):
        with pytest.raises(ValueError, match="context_dropout"):
            data.training_batch(*args, context_dropout=bad, drop_rng=np.random.default_rng(0))


def test_dropped_rows_are_a_function_of_the_batch_index(monkeypatch):
    """SyntheticDocuments.batches: the rows dropped from the batch that starts at page i depend on (seed, i) alone - not on the rng that
    draws the boxes, not on where the iterator started; context_dropout = 0 leaves the batches and the box rng's stream as they were"""
    from diffute_amd import data
    B = 4
    fake = _Fake(monkeypatch, B)
    ds = object.__new__(data.SyntheticDocuments)
    ds.seed, ds.glyph = 5, (None, None, None)
    monkeypatch.setattr(data.SyntheticDocuments, "__getitem__", lambda self, i: {"i": i})
    monkeypatch.setattr(data.SyntheticDocuments, "compose", lambda self, records: [None] * len(records))
    draws = []

    def boxes(records, rng, crop_scale):
        draws.append(float(rng.random()))
        return [None] * B, [None] * B, ["a"] * B
    monkeypatch.setattr(data, "sample_boxes", boxes)

    def dropped(start, n, box_seed, p):
        it = ds.batches(B, np.random.default_rng(box_seed), context_dropout=p, start=start)
        return [tuple(bool((b["ocr_embeddings"][r] == 0).all()) for r in range(B)) for b in (next(it) for _ in range(n))]
    a = dropped(0, 6, 1, 0.5)
    assert dropped(0, 6, 2, 0.5) == a                       # another box rng: the same rows
    assert dropped(2 * B, 4, 3, 0.5) == a[2:]               # started later: batch i is batch i
    assert len(set(a)) > 1 and any(any(r) for r in a) and not all(all(r) for r in a)
    want = [tuple((np.random.default_rng([5, i * B, 1]).random(B) < 0.5).tolist()) for i in range(6)]
    assert a == want
    del draws[:]
    dropped(0, 3, 9, 0.0)
    zero = list(draws)
    del draws[:]
    dropped(0, 3, 9, 0.5)
    assert draws == zero and dropped(0, 3, 9, 0.0) == [(False,) * B] * 3      # the box rng's stream does not see the dropout
