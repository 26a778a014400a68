"""ff.net.2 + proj_out as one GEMM over the composed weights (dmx_set_ff_fold; fold.hip, unet.hip Fwd::xformer), both builds.

1. the composition kernel per element (dmx_test_compose_linear) into poisoned, guarded outputs: C = 64, 128 and 88 (no multiple of any tile edge);
2. the folded block tail - [g | h3] [W' | Wpo]^T + b' + x through the two-segment GEMM the walk launches - against fp64, per slice, at M = 64 and
   192 rows, C = 64 and 128, once with a forced split-K (reduce pass: bias, residual); and on the executor (dmx_test_folded_tail_gn) with the GroupNorm
   behind it: reduce pass left to the GroupNorm / run by the GEMM / forced by releasing the residual early - the same bits;
3. the tiny UNet with the switch on and off: both inside the tap bounds against the bf16-emulating oracle, and the folded walk no farther from the
   fp32 instantiation than the two-launch walk by more than the tail's per-slice bound (once, at every tap);
4. launch accounting: one GEMM launch less per transformer block, and with a forced split on ff.net.2 fewer reduce launches (the deferral happened);
5. freshness: after mark_parameters_changed(), a FusedAdamW step and EMAModel.copy_to the folded walk runs the new weights - and the optimizer
   step launches no composition;
6. eager == replayed graph bit for bit, the switch is part of the graph key.
References, bounds and floors: fold_refs.py / fold_floors.py (test_ff_fold_host.py pins them on the CPU)."""
import ctypes

import pytest
import torch

import fold_refs as R
from test_train_small_gpu import call
from test_weight_pack_gpu import assert_bits, flat_poisoned
from util import assert_close, assert_close_slices, assert_guard_intact, poisoned, rel_l2, slice_err

pytestmark = pytest.mark.gpu
ELEMS = ["bf16", "fp16"]
DT = R.ELEMS
PROF_SPLITK, PROF_GEMM0, PROF_GEMM1 = 2, 10, 26      # kernels.h ProfClass: the reduce pass, the GEMM instances [10, 26)


def two_walks_bound():
    """the issue's "bound 3" for two walks on the same weights: each meets TAP_TOL[tap] against the one oracle tensor (test 3, test_models_gpu.py),
    so by the triangle inequality they lie within 2 x TAP_TOL[tap] of each other; the model output sits behind the last tap, up3"""
    from test_models_gpu import TAP_TOL
    return 2 * TAP_TOL["up3"]


@pytest.fixture(scope="module")
def cuda():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda")


def compose_on_gpu(inputs, C, elem, dev):
    """-> (guarded buffers, wfpo [C][5C], bfpo [C]) of dmx_test_compose_linear on the case's weights (inside ops.element_type(elem))"""
    dt = DT[elem]
    buf, span = flat_poisoned(C * 5 * C, dt, dev)
    bbuf, bspan = flat_poisoned(C, torch.float32, dev)
    call("dmx_test_compose_linear", inputs["wpo"].to(dt).to(dev), inputs["wf2"].to(dt).to(dev), inputs["bf2"].float().to(dev), inputs["bpo"].float().to(dev),
         span, bspan, C, 4 * C)
    torch.cuda.synchronize()
    return (buf, bbuf), span.view(C, 5 * C), bspan


# ---------------------------------------------------------------------------------------------- 1. the composition kernel
@pytest.mark.parametrize("elem", ELEMS)
@pytest.mark.parametrize("C", R.COMPOSE_C)
def test_compose_linear_per_element(cuda, C, elem):
    from diffute_amd import ops
    key = f"compose/{C}/{elem}"
    inputs, qty, (ref_w, _) = R.compose_eval(C, elem)
    with ops.element_type(elem):
        (buf, bbuf), w, b = compose_on_gpu(inputs, C, elem, cuda)
    assert_guard_intact(buf, w, name=key + ":w"); assert_guard_intact(bbuf, b, name=key + ":b")
    got = w.cpu().double()
    assert torch.isfinite(got).all(), f"{key}: non-finite composed weight"
    err, bound = (got[:, :4 * C] - ref_w[:, :4 * C]).abs(), R.compose_bound(inputs["wpo"], inputs["wf2"])
    print(f"{key}:w worst |got - ref| / bound {float((err / bound).max()):.3f}, max |W'| {float(got[:, :4 * C].abs().max()):.3f}")
    assert bool((err <= bound).all()), f"{key}: {int((err > bound).sum())} elements of W' outside the per-element bound"
    assert_bits(w[:, 4 * C:], inputs["wpo"].to(DT[elem]), key + ": the Wpo segment")
    q = qty["b"]; wt, st = R.bounds(key, qty)["b"]
    gb = b.cpu().double()
    e, s = R.measure(q._replace(model=gb))
    print(f"{key}:b whole {e:.3e}/{wt:.2e} slice {s:.3e}/{st:.2e}")
    assert e <= wt and s <= st, f"{key}: composed bias outside the fp32 bound"


# ---------------------------------------------------------------------------------------------- 2. the folded tail
TAIL_RUNS = [(c, False) for c in R.TAIL_CASES] + [((192, 128), True), ((64, 64), True)]


@pytest.mark.parametrize("elem", ELEMS)
@pytest.mark.parametrize("case,split", TAIL_RUNS, ids=[f"{c[0]}x{c[1]}{'_splitk' if s else ''}" for c, s in TAIL_RUNS])
def test_folded_tail_vs_fp64(cuda, case, split, elem):
    from diffute_amd import _cabi, ops
    M, C = case
    key = f"tail/{M}x{C}/{elem}"
    inputs, qty = R.tail_eval(case, elem)
    dt = DT[elem]
    dev = lambda t, c: t.to(dt).to(cuda).view(1, 1, M, c)
    with ops.element_type(elem):
        lib = ops.lib()
        _, w, b = compose_on_gpu(inputs, C, elem, cuda)
        ybuf, y = poisoned((1, 1, M, C), dt, cuda)
        try:
            if split:                                                   # the 128x64x32 instance, K split in two: 5C / 32 = 10 or 20 K-tiles
                lib.dmx_gemm_plan_override(M, C, 5 * C, 1, 0, 1, 2)
            torch.cuda.synchronize()
            lib.dmx_profile_begin()
            ops.conv_gemm(dev(inputs["g"], 4 * C), w, C, x1=dev(inputs["h3"], C), ksize=1, pad=0, bias=b, res=dev(inputs["x"], C), out=y)
            prof = (ctypes.c_double * (4 * 32))()
            _cabi.check(lib.dmx_profile_end(prof, len(prof)), "profile_end")
        finally:
            lib.dmx_gemm_plan_override(0, 0, 0, 0, 0, -1, 0)
    if split:
        assert int(prof[4 * PROF_SPLITK]) == 1, "the forced split-K plan did not run"
    assert_guard_intact(ybuf, y, name=key)
    q = qty["y"]; wt, st = R.bounds(key, qty)["y"]
    got = y.reshape(M, C).cpu().double()
    e = rel_l2(got, q.whole_ref); s = max(slice_err(got, q.ref, d)[0] for d in q.dims)
    print(f"{key}:y{' split-K' if split else ''} whole {e:.3e}/{wt:.2e} slice {s:.3e}/{st:.2e}")
    assert e <= wt, f"{key}: whole-tensor rel-L2 {e:.3e} > {wt:.1e}"
    assert_close_slices(got, q.ref, st, q.dims, key)


@pytest.mark.parametrize("elem", ELEMS)
def test_deferred_reduce_of_the_folded_tail_is_bit_identical(cuda, elem):
    """the folded GEMM on a forced split-K plan with the GroupNorm behind it, on the executor as the walk runs them (dmx_test_folded_tail_gn): the reduce
    pass summed by the GroupNorm - which then adds bfpo and the residual x and writes y - gives the bits of the GEMM's own reduce launch, in y and in
    the normalised tensor; so does releasing x before the GroupNorm (Exec::drop must complete y while x is alive).  y also meets the tail's fp64 bounds."""
    from diffute_amd import _cabi, ops
    B, HW, C, G = 2, 96, 128, 32                                        # M = 192: one whole row tile and a ragged one
    M = B * HW
    key = f"tail/{M}x{C}/{elem}"
    inputs, qty = R.tail_eval((M, C), elem)
    dt = DT[elem]
    d16 = lambda t: t.to(dt).to(cuda).contiguous()
    gamma = (1.0 + 0.1 * R.seeded((C,), 21)).float().to(cuda); beta = (0.1 * R.seeded((C,), 22)).float().to(cuda)
    g, h3, x = d16(inputs["g"]), d16(inputs["h3"]), d16(inputs["x"])
    got, reduces = {}, {}
    with ops.element_type(elem):
        lib = ops.lib()
        _, w, b = compose_on_gpu(inputs, C, elem, cuda)
        try:
            lib.dmx_gemm_plan_override(M, C, 5 * C, 1, 0, 1, 2)
            for mode in (0, 1, 2):
                ws = torch.empty(int(lib.dmx_test_folded_tail_gn_workspace_bytes(B, HW, C, G, mode)), dtype=torch.uint8, device=cuda)
                (ybuf, y), (tbuf, t) = flat_poisoned(M * C, dt, cuda), flat_poisoned(M * C, dt, cuda)
                torch.cuda.synchronize()
                lib.dmx_profile_begin()
                call("dmx_test_folded_tail_gn", g, h3, x, w, b, gamma, beta, B, HW, C, G, mode, y, t, ws, ws.numel())
                prof = (ctypes.c_double * (4 * 32))()
                _cabi.check(lib.dmx_profile_end(prof, len(prof)), "profile_end")
                assert_guard_intact(ybuf, y, name=f"{key} mode {mode}: y"); assert_guard_intact(tbuf, t, name=f"{key} mode {mode}: t")
                got[mode], reduces[mode] = (y.clone(), t.clone()), int(prof[4 * PROF_SPLITK])
        finally:
            lib.dmx_gemm_plan_override(0, 0, 0, 0, 0, -1, 0)
    print(f"{key}: reduce launches own / deferred / residual released first: {reduces[0]} / {reduces[1]} / {reduces[2]}")
    assert reduces == {0: 1, 1: 0, 2: 1}, reduces
    for mode in (1, 2):
        assert_bits(got[mode][0], got[0][0], f"{key} mode {mode}: y"); assert_bits(got[mode][1], got[0][1], f"{key} mode {mode}: GroupNorm(y)")
    q = qty["y"]; wt, st = R.bounds(key, qty)["y"]
    y64 = got[1][0].view(M, C).cpu().double()
    e = rel_l2(y64, q.whole_ref)
    print(f"{key}:y deferred whole {e:.3e}/{wt:.2e}")
    assert e <= wt
    assert_close_slices(y64, q.ref, st, q.dims, key)
    assert torch.isfinite(got[1][1].float()).all()


# ---------------------------------------------------------------------------------------------- tiny UNet
def tiny(seed=None):
    import diffute_amd as D
    from test_models_gpu import TINY_UNET
    return D.UNet2DConditionModel(**TINY_UNET, **({} if seed is None else dict(seed=seed))).cuda()


def n_blocks(unet):
    """transformer blocks of the model (none of the tiny config's runs as a chain: they are C = 320 kernels)"""
    L = unet.config.layers_per_block
    return sum(L for t in unet.config.down_block_types if t.startswith("CrossAttn")) + 1 + sum(L + 1 for t in unet.config.up_block_types if t.startswith("CrossAttn"))


class fold:
    """with fold(lib, on): the switch at `on`, restored afterwards"""
    def __init__(self, lib, on): self.lib, self.on = lib, on
    def __enter__(self): self.old = self.lib.dmx_set_ff_fold(self.on)
    def __exit__(self, *a): self.lib.dmx_set_ff_fold(self.old)


def profiled(lib, fn):
    """fn() inside a profiler bracket -> (result, GEMM launches, reduce launches, launches of the composition kernel)"""
    from diffute_amd import _cabi
    torch.cuda.synchronize()
    lib.dmx_profile_begin()
    out = fn()
    buf = (ctypes.c_double * (4 * 32))()
    _cabi.check(lib.dmx_profile_end(buf, len(buf)), "profile_end")
    sbuf = ctypes.create_string_buffer(1 << 16)
    nb = lib.dmx_profile_symbols(sbuf, len(sbuf))
    composed = sum(float(l.split("\t")[1]) for l in sbuf.raw[:nb].decode().splitlines() if "dmx_compose_linear_kernel" in l)
    return out, sum(int(buf[4 * c]) for c in range(PROF_GEMM0, PROF_GEMM1)), int(buf[4 * PROF_SPLITK]), int(composed)


def test_tiny_unet_taps_fold_on_and_off(cuda):
    """both walks meet the tap bounds of test_models_gpu.py against the bf16-emulating oracle.  Against the fp32 instantiation of the same graph the
    folded walk may be farther than the two-launch walk by ONE application of the tail's per-slice bound (fold_refs.tol_of: the block output against
    fp64), at every tap, however many folded blocks lie upstream of it."""
    from diffute_amd import _cabi
    from diffute_amd.synthetic import synth_inputs
    from test_models_gpu import TAP_TOL, _load_taps
    lib = _cabi.lib()
    _, b16 = _load_taps()
    unet = tiny().requires_grad_(False)
    lat, mask, mlat, ctx = synth_inputs(2, 16, 16, 77, 128, device=cuda)
    x = torch.cat([lat, mask, mlat], 1)
    _, t32 = unet.forward_fp32([lat, mask, mlat], torch.tensor(981), ctx, taps=True)
    dist = {}
    for on in (1, 0):
        with fold(lib, on):
            _, taps = unet.forward_taps(x, torch.tensor(981), ctx)
        errs = {k: assert_close(taps[k], b16[k], TAP_TOL[k], f"ff_fold {on}: block tap {k} vs bf16-emulating oracle") for k in taps}
        dist[on] = {k: rel_l2(taps[k], t32[k]) for k in taps}
        print(f"ff_fold {on}: taps vs oracle " + " ".join(f"{k} {e:.1e}" for k, e in errs.items()))
        print(f"ff_fold {on}: taps vs fp32 path " + " ".join(f"{k} {e:.2e}" for k, e in dist[on].items()))
    st = max(R.tol_of(R.tail_eval(c, "bf16")[1]["y"], R.FLOORS[f"tail/{c[0]}x{c[1]}/bf16:y"])[1] for c in R.TAIL_CASES)
    for k in dist[1]:
        assert dist[1][k] <= dist[0][k] + st, f"tap {k}: folded walk {dist[1][k]:.3e} from the fp32 path, two-launch walk {dist[0][k]:.3e}"


def test_launch_accounting(cuda):
    """the fold takes one GEMM launch per transformer block out of the forward; with ff.net.2 forced onto a split-K plan the folded walk also runs
    fewer reduce launches - the GroupNorm behind the block sums the planes (the deferral happened) - and computes the same thing within the tap bound"""
    from diffute_amd import _cabi
    from diffute_amd.synthetic import synth_inputs
    lib = _cabi.lib()
    unet = tiny().requires_grad_(False)
    lat, mask, mlat, ctx = synth_inputs(2, 16, 16, 77, 128, device=cuda)
    unet.set_context(ctx)
    t = torch.tensor([501], device=cuda)
    run = lambda: unet.forward_parts([lat, mask, mlat], t).clone()
    try:
        res = {}
        for forced in (False, True):
            if forced:
                for lvl, C in enumerate(unet.config.block_out_channels):      # (level 3: the mid block's, 2 x 2 pixels)
                    M = 2 * (16 >> lvl) ** 2
                    lib.dmx_gemm_plan_override(M, C, 4 * C, 1, 0, 1, 2)      # ff.net.2 alone ...
                    lib.dmx_gemm_plan_override(M, C, 5 * C, 1, 0, 1, 2)      # ... and with proj_out folded in: 128x64x32 tiles, K split in two
            for on in (1, 0):
                with fold(lib, on):
                    run()                                                     # (the first call after a switch composes / sizes the workspace)
                    res[forced, on] = profiled(lib, run)
        nb = n_blocks(unet)
        for forced in (False, True):
            (y1, g1, r1, c1), (y0, g0, r0, c0) = res[forced, 1], res[forced, 0]
            print(f"forced split {forced}: GEMM launches {g0} -> {g1} ({nb} blocks), reduce launches {r0} -> {r1}")
            assert g0 - g1 == nb, (g0, g1, nb)
            assert c1 == 0 and c0 == 0, "the composition ran in a steady-state forward"
            assert rel_l2(y1, y0) <= two_walks_bound()
        assert res[True, 0][2] >= nb, "the forced split-K plans did not run"
        assert res[True, 1][2] < res[True, 0][2], "no reduce pass was left to a GroupNorm"
    finally:
        lib.dmx_gemm_plan_override(0, 0, 0, 0, 0, -1, 0)


def test_folded_walk_follows_the_weights(cuda):
    """the composed weights are derived data that lag the raw ones: after each kind of weight change the folded forward must equal - within
    two_walks_bound() - the two-launch forward of a FRESH model loaded from the changed model's state_dict();
    the optimizer step itself launches no composition (it only marks the fold stale)."""
    import diffute_amd as D
    from diffute_amd import _cabi
    from diffute_amd.models import mse_loss
    from diffute_amd.synthetic import synth_inputs
    from diffute_amd.training_utils import EMAModel
    lib = _cabi.lib()
    lat, mask, mlat, ctx = synth_inputs(2, 16, 16, 77, 128, device=cuda)
    x = torch.cat([lat, mask, mlat], 1); t = torch.tensor([500, 40], device=cuda)
    bound = two_walks_bound()

    def infer(m):
        with torch.no_grad():
            return m(x, t, ctx).sample.clone()

    def check(unet, before, what):
        with fold(lib, 1):
            got = infer(unet)
        fresh = tiny(seed=99)
        fresh.load_state_dict(unet.state_dict())
        with fold(lib, 0):
            want = infer(fresh)
        moved = rel_l2(want, before)
        e = rel_l2(got, want)
        print(f"{what}: folded forward vs two-launch forward of a reloaded model {e:.2e} (bound {bound:.1e}); the change moved the output by {moved:.2e}")
        assert moved > 4 * bound, f"{what}: the weight change is too small to tell stale weights from fresh ones"
        assert e <= bound, f"{what}: the folded forward does not follow the new weights"
        return got

    unet = tiny()
    with fold(lib, 1):
        y = infer(unet)
        # 1. an in-place write torch does not record
        other = tiny(seed=7)
        with torch.no_grad():
            for p, q in zip(unet.parameters(), other.parameters()):
                p.data.copy_(q.data)
        unet.mark_parameters_changed()
        y = check(unet, y, "mark_parameters_changed")
        # 2. one fused optimizer step
        opt = D.FusedAdamW(unet, lr=2e-2)
        mse_loss(unet(x, t, ctx).sample, torch.zeros_like(lat)).backward()
        _, _, _, composed = profiled(lib, opt.step)
        assert composed == 0, "FusedAdamW.step() ran the composition kernel"
        _, _, _, composed = profiled(lib, lambda: infer(unet))      # ... the next inference call does, once per block
        assert composed == n_blocks(unet), (composed, n_blocks(unet))
        y = check(unet, y, "FusedAdamW.step")
        # 3. EMAModel.copy_to
        ema = EMAModel(tiny(seed=11).parameters())
        ema.copy_to(unet.parameters())
        check(unet, y, "EMAModel.copy_to")


@pytest.mark.parametrize("elem", ELEMS)
def test_graph_replay_and_switch_in_the_graph_key(cuda, elem):
    """switch 1: eager == captured == replayed, bit for bit; 1 -> 0 -> 1 on the same buffers reproduces the first result and never replays the other
    setting's graph (the two settings differ at rounding level: equal outputs would mean a wrong replay)"""
    from diffute_amd import _cabi
    from diffute_amd.synthetic import synth_inputs
    lib = _cabi.lib(elem)
    unet = tiny().requires_grad_(False)
    if elem == "fp16":
        unet = unet.to(dtype=torch.float16)
    lat, mask, mlat, ctx = synth_inputs(2, 16, 16, 77, 128, device=cuda)
    unet.set_context(ctx)
    t = torch.tensor([501], device=cuda)
    out = torch.empty(2, 4, 16, 16, device=cuda)
    st = torch.cuda.Stream()
    torch.cuda.synchronize()
    with fold(lib, 1), torch.cuda.stream(st):
        eager = unet.forward_parts([lat, mask, mlat], t).clone()
        runs = {}
        for on in (1, 0, 1):
            lib.dmx_set_ff_fold(on)
            reps = [unet.forward_parts([lat, mask, mlat], t, out=out, graph=True).clone() for _ in range(4)]      # eager, capture, two replays
            assert all(torch.equal(r, reps[0]) for r in reps), f"{elem} ff_fold {on}: the replayed graph differs from the eager walk"
            runs.setdefault(on, []).append(reps[0])
        torch.cuda.synchronize()
    assert torch.isfinite(eager).all()
    assert torch.equal(runs[1][0], eager) and torch.equal(runs[1][1], eager), f"{elem}: switch 1 -> 0 -> 1 does not reproduce the first result"
    assert not torch.equal(runs[0][0], eager), f"{elem}: switch 0 returned the folded walk's bits (a graph of the other setting was replayed?)"
    e = rel_l2(runs[0][0], eager)
    print(f"{elem}: folded vs two-launch forward rel-L2 {e:.2e}")
    assert e <= two_walks_bound()
