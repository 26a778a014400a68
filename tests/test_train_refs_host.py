"""Pins the references and bounds of test_train_layout_gpu.py on the CPU (no GPU, no kernel output involved).

For every case of train_refs.py the rounding-point restatement (fp64 arithmetic, rounded where the kernel is documented to
round: P and dS to the 16-bit element, 16-bit outputs stored rounded) and, for fp32 outputs, torch's float32 computation are
compared with the fp64 reference by the same whole-tensor and per-slice metrics the GPU tests use.  An honest implementation
must sit inside every bound with the margin the bound was derived with (3 x for 16-bit outputs, 8 x for fp32 ones), and the
figures recorded in train_floors.py - the ones the bounds are computed from - must be the measured ones.  The helpers
(slice_err, poisoned, assert_guard_intact) are exercised on deliberately corrupted tensors, and faults of the kind the GPU
cases exist for are injected into the restatement to show the per-slice bound catches what the whole-tensor bound lets through."""
import pytest
import torch

import train_refs as R
from util import assert_close, assert_close_slices, assert_guard_intact, poisoned, rel_l2, seeded, slice_err

CASES = R.all_cases()


@pytest.mark.parametrize("key,thunk", CASES, ids=[c[0] for c in CASES])
def test_restatement_inside_bounds(key, thunk):
    _, qty = thunk()
    bounds = R.bounds(key, qty)
    for name, q in qty.items():
        w, s = R.measure(q)
        rw, rs = R.FLOORS[f"{key}:{name}"]
        wt, st = bounds[name]
        print(f"{key}:{name} restatement whole {w:.3e} (bound {wt:.2e}) slice {s:.3e} (bound {st:.2e})")
        assert torch.isfinite(q.model).all() and torch.isfinite(q.ref).all()
        if q.kind == "x":
            assert torch.equal(q.model, q.ref) and (wt, st) == (0.0, 0.0)        # compared bit for bit on the GPU: no tolerance
        elif q.kind == "16":
            # the recorded floor is the measured one (the restatement is fp64 arithmetic + roundings: reproducible)
            assert abs(w - rw) <= 0.02 * rw + 1e-12 and abs(s - rs) <= 0.02 * rs + 1e-12, f"{key}:{name}: recorded ({rw:.3e}, {rs:.3e}), measured ({w:.3e}, {s:.3e})"
            assert w <= wt and s <= st / 3 * 1.02 or s <= q.base / 3, f"{key}:{name}: restatement outside its bound"
            assert w <= wt, f"{key}:{name}: restatement misses the whole-tensor bound: {w:.3e} > {wt:.1e}"
        else:
            # float32 summation order differs between hosts: the float32 computation only has to stay inside the bound
            assert w <= wt and s <= st, f"{key}:{name}: torch float32 ({w:.3e}, {s:.3e}) outside ({wt:.2e}, {st:.2e})"


def test_slice_err_definition():
    r = torch.zeros(4, 6, dtype=torch.float64); r[0] = 1.0; r[1] = 2.0; r[2] = 1e-9; r[3] = 3.0
    h = r.clone(); h[2] += 1e-9                    # a near-zero slice off by 100 %: the floor rho keeps it from dominating
    e, i = slice_err(h, r, 0)
    rho = float(r.pow(2).sum(1).sqrt().pow(2).mean().sqrt())
    assert i == 2 and abs(e - (6 ** 0.5) * 1e-9 / rho) < 1e-15
    h = r.clone(); h[1] *= 1.1                      # 10 % on one slice
    e, i = slice_err(h, r, 0)
    assert i == 1 and abs(e - 0.1) < 1e-12
    e, i = slice_err(h, r, 1)                       # along the other axis every slice sees it, diluted
    assert 0.05 < e < 0.1
    e, i = slice_err(h.view(2, 2, 6), r.view(2, 2, 6), (0, 1))
    assert i == (0, 1) and abs(e - 0.1) < 1e-12
    with pytest.raises(AssertionError, match=r"index 1"):
        assert_close_slices(h, r, 1e-2, [0], "demo")


def test_single_row_fault_passes_whole_tensor_but_not_slices():
    """the self-check of this file: perturb ONE row of a restatement by 10 % - the whole-tensor bound does not notice, the
    per-slice bound must"""
    case = R.ATTN_CASES[8]                          # cross_256x577
    key = f"attn/{case[0]}/bf16"
    _, qty = R.attn_eval(case, "bf16")
    q = qty["dq"]
    wt, st = R.bounds(key, qty)["dq"]
    bad = q.model.clone(); bad[0, 0] *= 1.1         # one query row of 512 off by 10 %
    assert_close(bad, q.whole_ref, wt, "whole tensor")             # 0.1 / sqrt(512) is far inside 1.5e-2
    with pytest.raises(AssertionError, match=r"index \(0, 0\)"):
        assert_close_slices(bad, q.ref, st, q.dims, "one query row off by 10 %")
    o = qty["o"]; wo, so = R.bounds(key, qty)["o"]
    bad_o = o.model.clone(); bad_o[1, 255] *= 1.05  # the last query row of the last sample off by 5 %
    assert_close(bad_o, o.whole_ref, wo, "whole tensor")
    with pytest.raises(AssertionError, match=r"index \(1, 255\)"):
        assert_close_slices(bad_o, o.ref, so, o.dims, "the last query row off by 5 %")
    assert_close_slices(q.model, q.ref, st, q.dims, "unperturbed")


def test_injected_kernel_faults_are_caught():
    # dS of the ragged last 32-query tile dropped (1 of 33 queries): that query's dq row vanishes
    case = R.ATTN_GS_CASE
    key = f"attn/{case[0]}/bf16"
    _, good = R.attn_eval(case, "bf16")
    _, bad = R.attn_eval(case, "bf16", fault="last_query_tile")
    b = R.bounds(key, good)
    with pytest.raises(AssertionError):
        assert_close_slices(bad["dq"].model, good["dq"].ref, b["dq"][1], good["dq"].dims, "dq of the dropped query rows")
    with pytest.raises(AssertionError):                 # ... and every key row's dk loses that query's contribution
        assert_close_slices(bad["dk"].model, good["dk"].ref, b["dk"][1], good["dk"].dims, "dk without the last query tile")
    # an error confined to the GroupNorm group that straddles the concat split (group 21), modelled as its dx off by 10 %
    case = R.GN_CASES[0]
    key = f"gn/{case[0]}/bf16"
    _, good = R.gn_eval(case, "bf16")
    _, bad = R.gn_eval(case, "bf16", fault="straddle_group_scaled")
    wt, st = R.bounds(key, good)["dx"]
    with pytest.raises(AssertionError, match=r"index \(\d+, 21\)"):
        assert_close_slices(bad["dx"].model, good["dx"].ref, st, good["dx"].dims, "straddling group")
    # a dq store 8 columns wide of its slice of the fused [rows][3C] gradient buffer: lands in dk's columns 0..7
    buf, g = poisoned((6, 3 * 64), torch.bfloat16, "cpu")
    g.copy_(seeded((6, 192), 1))
    ref = g.clone().double()
    g[:, 64:72] = g[:, 56:64]
    with pytest.raises(AssertionError):
        assert_close_slices(g[:, 64:128], ref[:, 64:128], 1e-2, [0], "dk after a wide dq store")
    assert_guard_intact(buf, g)
    # ... and off the right edge of the last operand: into the guard band
    buf.view(torch.int16)[3, 8 + 192] = 0
    with pytest.raises(AssertionError, match="outside the output"):
        assert_guard_intact(buf, g)


def test_injected_small_kernel_faults_are_caught():
    """one fault per family of the small training kernels (test_train_small_gpu.py), of the kind its cases exist for.  Each is
    confined to one column / one sample / one tile: the per-slice bound, the guard check or the bit comparison names it.  The
    whole-tensor figure is printed next to the training-step bounds that were these kernels' only check before (whole-gradient
    rel-L2 5e-2, worst parameter 1.5e-1): the figure of the one affected tensor is of that order, and a training step sees it
    only after it has been mixed into every gradient upstream."""
    for elem in ("bf16", "fp16"):
        # the softmax loops stop after one pass of 256 threads: column 256 of an n = 257 row never enters the sum and is not stored
        for fn, case, name in ((R.softmax_eval, ("gauss", 5, 257), "p"), (R.softmax_bwd_eval, (5, 257), "ds")):
            key = ("softmax/gauss_5x257/" if name == "p" else "softmax_bwd/5x257/") + elem
            _, good = fn(case, elem)
            _, bad = fn(case, elem, fault="first_256")
            wt, st = R.bounds(key, good)[name]
            print(f"{key}: first-256 fault whole {rel_l2(bad[name].model, good[name].whole_ref):.3e}")
            assert_close_slices(good[name].model, good[name].ref, st, good[name].dims, "unperturbed")
            with pytest.raises(AssertionError, match=r"dim 1 is index 256"):
                assert_close_slices(bad[name].model, good[name].ref, st, [1], "column 256 dropped")
    # the dx kernel of linear_small_bwd tiles the batch in eights: the second tile (sample 9 of B = 9) missing
    case = next(c for c in R.LSB_CASES if c[0] == 9 and c[5] == "both" and c[1] > 1)
    key = f"lsb/{R.lsb_name(case)}/bf16"
    _, good = R.lsb_eval(case, "bf16")
    _, bad = R.lsb_eval(case, "bf16", fault="ninth_sample")
    wt, st = R.bounds(key, good)["dx"]
    print(f"{key}: ninth-sample fault whole {R.rel_l2_f64(bad['dx'].model, good['dx'].ref):.3e}")
    assert_close_slices(good["dx"].model, good["dx"].ref, st, good["dx"].dims, "unperturbed")
    with pytest.raises(AssertionError, match=r"dim 0 is index 8"):
        assert_close_slices(bad["dx"].model, good["dx"].ref, st, [0], "ninth sample missing")
    # batched transpose: the last ragged 64-tile of a job left unwritten.  Into a poisoned buffer the guard check says so; over
    # the previous step's W^T (the product's situation: the weights moved by a few 1e-3 relative since) the whole
    # tensor stays inside every tolerance this suite uses and only the bit comparison sees the stale tile
    i = 2; Rr, C = R.TRB_JOBS[i][:2]                     # 65 x 63 -> out 63 x 65: the tile of output columns 64 .. 64
    inputs, qty = R.transpose_batch_eval("bf16")
    want = qty[f"out{i}"].ref.to(torch.bfloat16)
    buf, out = poisoned((C, Rr), torch.bfloat16, "cpu")
    out[:, :64] = want[:, :64]
    with pytest.raises(AssertionError, match="never written"):
        assert_guard_intact(buf, out)
    stale = (want.double() * (1.0 + 3e-3 * seeded((C, Rr), 5).double())).to(torch.bfloat16)
    out2 = want.clone(); out2[:, 64:] = stale[:, 64:]
    assert not torch.equal(out2.view(torch.int16), want.view(torch.int16))
    assert_close(out2, want.float(), 1e-3, "whole tensor over a stale tile")     # TOL_D does not notice
    assert torch.equal(want.view(torch.int16), inputs["xs"][i].t().to(torch.bfloat16).contiguous().view(torch.int16))


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16, torch.float32])
def test_poisoned_and_guard(dtype):
    buf, view = poisoned((5, 16), dtype, "cpu", pad_rows=2, pad_cols=8)
    assert buf.shape == (9, 32) and view.shape == (5, 16) and view.stride(0) == 32
    assert torch.isfinite(buf.float()).all() and float(buf.float().abs().min()) > 5e4        # finite, and far above any output
    with pytest.raises(AssertionError, match="never written"):
        assert_guard_intact(buf, view)                      # nothing written yet
    view.copy_(seeded((5, 16), 1))
    assert_guard_intact(buf, view)
    sub = view[:, :8]                                        # a narrower logical view: the rest of `view` now counts as outside
    with pytest.raises(AssertionError, match="outside the output"):
        assert_guard_intact(buf, sub)
    view[4, 15] = buf[0, 0]                                  # one element left at the sentinel
    with pytest.raises(AssertionError, match="never written"):
        assert_guard_intact(buf, view)
    view[4, 15] = 1.0
    buf[1, 9] = 0.0                                          # one element of the row guard band
    with pytest.raises(AssertionError, match="row 1 column 9"):
        assert_guard_intact(buf, view)
    b1, v1 = poisoned((24,), dtype, "cpu")
    assert v1.shape == (24,) and b1.shape == (5, 40)
    b4, v4 = poisoned((6, 8), dtype, "cpu")
    v4.view(2, 3, 8).fill_(2.0)                              # a reshaped view of the logical output is the same memory
    assert_guard_intact(b4, v4.view(2, 3, 8))
