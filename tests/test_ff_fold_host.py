"""Pins the references and bounds of the ff.net.2 + proj_out fold (fold_refs.py) on the CPU - no GPU, no kernel output involved: the clean
restatement of the composition and of the folded block tail is inside its bounds, every figure recorded in fold_floors.py is the measured
one, and every injected fault - K segments swapped, bf2 not carried through Wpo, Wf2 read transposed, W' of the weights before a change -
exceeds the bound that the GPU test applies.  Also: the C ABI of the fold is declared where the host mirror looks for it."""
import os
import re

import pytest
import torch

import fold_refs as R
from util import assert_close_slices, rel_l2

CASES = R.all_cases()
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


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
        if q.kind == "16":
            assert abs(w - rw) <= 0.02 * rw + 1e-12 and abs(s - rs) <= 0.02 * rs + 1e-12, f"{key}:{name}: recorded ({rw:.3e}, {rs:.3e}), measured ({w:.3e}, {s:.3e})"
            assert w <= wt, f"{key}:{name}: restatement misses the whole-tensor bound: {w:.3e} > {wt:.1e}"
            assert s <= st / 3 * 1.02 or s <= q.base / 3, f"{key}:{name}: restatement outside its per-slice bound"
        else:       # float32 summation order differs between hosts: the float32 computation only has to stay inside the bound
            assert w <= wt and s <= st, f"{key}:{name}: torch float32 ({w:.3e}, {s:.3e}) outside ({wt:.2e}, {st:.2e})"


@pytest.mark.parametrize("elem", ["bf16", "fp16"])
@pytest.mark.parametrize("C", R.COMPOSE_C)
def test_composed_weight_restatement_inside_the_element_bound(C, elem):
    """the per-element bound of the composed weight holds for the restatement (one rounding of the exact product), with room: the first term
    alone is twice (bf16) / sixteen times (fp16) the rounding; and the values stay far inside the 16-bit range (|W'| finite in the fp16 build)"""
    inputs, _, (ref_w, w) = R.compose_eval(C, elem)
    bound = R.compose_bound(inputs["wpo"], inputs["wf2"])
    assert torch.isfinite(w).all() and float(w.abs().max()) < 4.0
    assert bool(((w[:, :4 * C] - ref_w[:, :4 * C]).abs() <= bound).all())
    assert torch.equal(w[:, 4 * C:], inputs["wpo"])                   # the second K segment is Wpo itself


@pytest.mark.parametrize("elem", ["bf16", "fp16"])
@pytest.mark.parametrize("fault", ["segments_swapped", "wf2_transposed"])
def test_composition_fault_exceeds_the_element_bound(fault, elem):
    C = 88
    inputs, _, (ref_w, _) = R.compose_eval(C, elem)
    _, _, (_, bad) = R.compose_eval(C, elem, fault)
    bound = R.compose_bound(inputs["wpo"], inputs["wf2"])
    n = int(((bad[:, :4 * C] - ref_w[:, :4 * C]).abs() > bound).sum())
    print(f"compose/{C}/{elem} fault {fault}: {n} of {C * 4 * C} elements outside the bound")
    assert n > C * 4 * C // 2


@pytest.mark.parametrize("elem", ["bf16", "fp16"])
def test_bias_fault_exceeds_the_fp32_bound(elem):
    key = f"compose/64/{elem}"
    good = R.compose_eval(64, elem)[1]["b"]
    bad = R.compose_eval(64, elem, "bf2_not_through_wpo")[1]["b"]
    wt, st = R.bounds(key, {"b": good})["b"]
    e = float((bad.model - good.ref).norm() / good.ref.norm())
    print(f"{key}:b fault bf2_not_through_wpo: whole {e:.3e} against {wt:.2e}")
    assert e > 1e3 * wt


TAIL_FAULTS = [(c, e, f) for e in ("bf16", "fp16") for c in (R.TAIL_CASES[0], R.TAIL_CASES[3]) for f in R.FAULTS]


@pytest.mark.parametrize("case,elem,fault", TAIL_FAULTS, ids=[f"{c[0]}x{c[1]}/{e}:{f}" for c, e, f in TAIL_FAULTS])
def test_injected_fault_is_rejected(case, elem, fault):
    key = f"tail/{case[0]}x{case[1]}/{elem}"
    good, bad = R.tail_eval(case, elem)[1]["y"], R.tail_eval(case, elem, fault)[1]["y"]
    wt, st = R.bounds(key, {"y": good})["y"]
    assert_close_slices(good.model, good.ref, st, good.dims, "unperturbed")
    w = rel_l2(bad.model, good.whole_ref)
    print(f"{key}:y fault {fault}: whole {w:.3e}/{wt:.2e}")
    assert w > wt, f"{key}: the whole-tensor bound lets {fault} through"
    with pytest.raises(AssertionError, match="worst slice"):
        assert_close_slices(bad.model, good.ref, st, good.dims, fault)


def test_fold_abi_is_declared():
    """dmx_set_ff_fold and the test entry: in the public header and in the ctypes table, with matching argument counts"""
    from diffute_amd import _cabi
    hdr = open(os.path.join(ROOT, "include", "diffute_hip.h")).read()
    for sym in ("dmx_set_ff_fold", "dmx_test_compose_linear"):
        m = re.search(r"\bint " + sym + r"\(([^;]*)\);", hdr)
        assert m, f"{sym} is not declared in include/diffute_hip.h"
        assert sym in _cabi._PROTOS and len(_cabi._PROTOS[sym][1]) == len(m.group(1).split(",")), sym
