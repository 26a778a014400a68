"""Pins the references and bounds of the forward layout tests (fwd_refs.py) on the CPU (no GPU, no kernel output involved): every clean restatement
of fwd_refs.py is inside its bounds, every figure recorded in fwd_floors.py is the measured one, and the per-slice bound rejects every
injected fault (the whole-tensor figure of each is printed next to its bound: most of them it lets through)."""
import pytest
import torch

import fwd_refs as R
from util import assert_close_slices, rel_l2

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
            assert torch.equal(q.model, q.ref) and (wt, st) == (0.0, 0.0)
        elif q.kind == "16":
            assert abs(w - rw) <= 0.02 * rw + 1e-12 and abs(s - rs) <= 0.02 * rs + 1e-12, f"{key}:{name}: recorded ({rw:.3e}, {rs:.3e}), measured ({w:.3e}, {s:.3e})"
            assert w <= wt, f"{key}:{name}: restatement misses the whole-tensor bound: {w:.3e} > {wt:.1e}"
            assert s <= st / 3 * 1.02 or s <= q.base / 3, f"{key}:{name}: restatement outside its per-slice bound"
        else:       # float32 summation order differs between hosts: the float32 computation only has to stay inside the bound
            assert w <= wt and s <= st, f"{key}:{name}: torch float32 ({w:.3e}, {s:.3e}) outside ({wt:.2e}, {st:.2e})"


def _faults():
    out = []
    for e in ("bf16", "fp16"):
        for c in (R.ATTN64_CASES[1], R.ATTN64_CASES[4], R.BAL_CASES[1]):
            out.append((f"attn64/{c[0]}/{e}", "o", "pad_key_unmasked", lambda f, c=c, e=e: R.attn64_eval(c, e, fault=f)[1]))
        for c in ((128, 33), (512, 200)):
            out.append((f"wide/d{c[0]}_S{c[1]}/{e}", "o", "last_key_tile_dropped", lambda f, c=c, e=e: R.wide_eval(c, e, fault=f)[1]))
        for c in (R.GNF_CASES[1], R.GNF_CASES[3], R.GNF_CASES[5], R.GNF_CASES[6]):
            out.append((f"gnf/{c[0]}/{e}", "y", "first_source_stats", lambda f, c=c, e=e: R.gnf_eval(c, e, fault=f)[1]))
        for rows in (1, 301):
            out.append((f"lnf/{rows}x520/{e}", "y", "ragged_octet_mean", lambda f, rows=rows, e=e: R.lnf_eval((rows, 520), e, fault=f)[1]))
        for fam, bk in (("base", 32), ("base", 64), ("streamk_tails", 64), ("shortcut", 64)):
            out.append((f"gemm/{fam}/k{bk}/{e}", "y", "bias_dropped_on_tail", lambda f, fam=fam, bk=bk, e=e: R.gemm_eval(fam, e, bk, f)[1]))
        out.append((f"ups2x/{e}", "y", "phase_swapped_on_right_border", lambda f, e=e: R.ups2x_eval(e, fault=f)[1]))
        for sh in ((8, 32), (32, 32)):
            out.append((f"halo/{sh[0]}x{sh[1]}_n160_gn_silu/{e}", "y", "bottom_pad_normalised", lambda f, sh=sh, e=e: R.halo_eval(sh, 160, "gn_silu", e, f)[1]))
        for m in R.XF_MODES:
            out.append((f"xf/mode{m}_M320/{e}", "y", "stats_from_row_plus_32", lambda f, m=m, e=e: R.xf_eval(m, 320, e, f)[1]))
        out.append((f"skinny/{R.SKINNY_SMALL[0][0]}/{e}", "y", "last_pixel_tap", lambda f, e=e: R.skinny_eval(R.SKINNY_SMALL[0], e, fault=f)[1]))
        out.append((f"ls/b3_n1280/{e}", "y", "third_sample", lambda f, e=e: R.ls_eval((3, 1280), e, fault=f)[1]))
    return out


FAULTS = _faults()


@pytest.mark.parametrize("key,name,fault,fn", FAULTS, ids=[f"{f[0]}:{f[2]}" for f in FAULTS])
def test_injected_fault_is_rejected_per_slice(key, name, fault, fn):
    good, bad = fn(None)[name], fn(fault)[name]
    wt, st = R.bounds(key, {name: good})[name]
    assert_close_slices(good.model, good.ref, st, good.dims, "unperturbed")
    w = rel_l2(bad.model, good.whole_ref) if good.kind == "16" else float((bad.model - good.ref).norm() / good.ref.norm())
    print(f"{key}:{name} fault {fault}: whole {w:.3e}/{wt:.2e} -> the whole-tensor bound {'REJECTS' if w > wt else 'passes'} it")
    with pytest.raises(AssertionError, match="worst slice"):
        assert_close_slices(bad.model, good.ref, st, good.dims, fault)


def test_gemm_table_names_a_reason_for_every_gap():
    """the table alone: every live instance is expected to run the base family and at least one other, every gap carries a reason.  That the
    library agrees - a refused pair raises, an accepted pair runs - is test_fwd_layout_gpu.py's test_conv_gemm_every_instance_every_epilogue"""
    for tn in R.GEMM_TN:
        can = [f for f in R.GEMM_FAMILIES if R.gemm_cannot_run(tn, f) is None]
        assert "base" in can and len(can) >= 2, f"tile instance {tn} runs only {can}"
        for f in R.GEMM_FAMILIES:
            r = R.gemm_cannot_run(tn, f)
            assert r is None or len(r) > 10
