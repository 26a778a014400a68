"""Pins the references and bounds of test_train_walk_gpu.py on the CPU (no GPU, no kernel output involved).

For every case of train_walk_refs.py the rounding-point restatement of one training step is compared per parameter with the
fp32 oracle's gradient: the figures recorded in train_walk_floors.py - the ones the GPU bounds are computed from - must be the
measured ones, the parameters judged absolutely must be exactly the set the stated condition selects, and wiring faults of the
kind the GPU test exists for, injected into the oracle's graph with the element's rounding on top, must leave the fp16 bounds.
One of them (the d emb contribution of down level 3 halved) passes the whole-gradient 4e-2 / worst-parameter 1e-1 bars that
were the training walk's only check before: that is the recorded reason for these files."""
import statistics

import pytest
import torch

import train_walk_refs as R

KEYS = [(m, c, e) for m, c in R.ALL_KEYS for e in R.ELEMS]
_cache = {}


def _ref(model, case):
    if (model, case) not in _cache:
        P = R.host_params(model)
        loss, g = R.reference(model, case, P)
        _cache[(model, case)] = (P, loss, g, R.absolute_set(g))
    return _cache[(model, case)]


@pytest.mark.parametrize("model,case,elem", KEYS, ids=[f"{m}/{c}/{e}" for m, c, e in KEYS])
def test_floors_are_the_measured_ones(model, case, elem):
    key = f"{model}/{case}/{elem}"
    P, ref_loss, ref, ab = _ref(model, case)
    loss, g = R.restatement(model, case, P, elem)
    whole, per = R.errors(g, ref, ab)
    med = statistics.median(per.values())
    rw, rm, own = R.FLOORS[key]
    worst = max(per, key=per.get)
    print(f"{key} restatement whole {whole:.3e} median {med:.3e} worst {worst} {per[worst]:.3e} (recorded {rw:.3e} / {rm:.3e}); loss {loss:.6f} vs {ref_loss:.6f}")
    # the restatement is float64 arithmetic + roundings: reproducible (the tolerance of test_train_refs_host.py)
    assert abs(whole - rw) <= 0.02 * rw + 1e-12 and abs(med - rm) <= 0.02 * rm + 1e-12, f"{key}: recorded ({rw:.3e}, {rm:.3e}), measured ({whole:.3e}, {med:.3e})"
    assert set(own) <= set(per), f"{key}: recorded parameters that are not judged relatively: {sorted(set(own) - set(per))[:3]}"
    for k, e in per.items():
        if k in own:
            assert abs(e - own[k]) <= 0.02 * own[k] + 1e-12, f"{key}: {k}: recorded {own[k]:.3e}, measured {e:.3e}"
        else:
            assert e <= rm * 1.02, f"{key}: {k}: floor {e:.3e} above the median {rm:.3e} but not recorded"
    assert abs(loss - ref_loss) <= R.LOSS_TOL * abs(ref_loss)
    # an honest implementation sits inside every bound with the margin the bound was derived with
    wb, pb = R.bounds(key)
    assert whole <= wb / R.FACTOR_WHOLE * 1.02 and all(e <= pb(k) / R.FACTOR_PARAM * 1.02 for k, e in per.items())
    R.check(key, g, ref, loss, ref_loss, ab)


@pytest.mark.parametrize("model,case", R.ALL_KEYS, ids=[f"{m}/{c}" for m, c in R.ALL_KEYS])
def test_absolute_sets_are_exact(model, case):
    """which parameters leave the relative check is a stated condition (train_walk_refs.absolute_set), and it selects exactly:
    the VAE's two to_k.bias (softmax is shift invariant per row), and in min8_b1 the two attn1 weights of the 1x1 level (softmax
    over one key).  Nothing else, in any case."""
    _, _, ref, ab = _ref(model, case)
    if model == "vae":
        want = {"encoder.mid_block.attentions.0.to_k.bias", "decoder.mid_block.attentions.0.to_k.bias"}
    elif case == "min8_b1":
        t = "mid_block.attentions.0.transformer_blocks.0.attn1."
        want = {t + "to_q.weight", t + "to_k.weight"}
        assert all(float(ref[k].abs().max()) == 0.0 for k in want)             # exactly zero: one key, softmax == 1
    else:
        want = set()
    assert ab == want, f"{model}/{case}: judged absolutely {sorted(ab)}, expected {sorted(want)}"
    for k in ab:
        tov = R.to_v_of(k)
        assert tov in ref and R._norm(ref[tov]) > 0
        print(f"{model}/{case}: {k}: ||ref|| {R._norm(ref[k]):.2e}, ||ref to_v|| {R._norm(ref[tov]):.2e}")
    # every other parameter has a reference gradient that is not noise: far above float32 resolution of its own sum
    for k, r in ref.items():
        if k not in ab:
            assert R._norm(r) > 0, f"{model}/{case}: {k}: zero reference gradient"


@pytest.mark.parametrize("fault", R.FAULTS)
def test_injected_wiring_faults_are_caught(fault):
    """each fault, with fp16 rounding on top, leaves the fp16 per-parameter bounds; printed: whether the bars the walk was held to
    before (whole gradient 4e-2, worst parameter 1e-1) would have tripped"""
    case = "wide_b3"
    P, _, ref, ab = _ref("unet", case)
    old = {}
    for elem in ("fp16", "bf16"):
        key = f"unet/{case}/{elem}"
        _, g = R.restatement("unet", case, P, elem, fault=fault)
        whole, per = R.errors(g, ref, ab)
        worst = max(per.values())
        old[elem] = whole > R.OLD_BARS[0] or worst > R.OLD_BARS[1]
        out = R.caught(key, g, ref, ab)
        print(f"{fault} [{elem}]: whole {whole:.3e} worst parameter {worst:.3e}; old bars (4e-2 / 1e-1) {'trip' if old[elem] else 'PASS'}; "
              f"{len(out)} parameters outside the per-parameter bounds" + (f", worst {out[0][2]} {out[0][1]:.3e} = {out[0][0]:.1f} x bound" if out else ""))
        if elem == "fp16":
            assert out, f"{fault}: not caught by the fp16 per-parameter bounds"
            with pytest.raises(AssertionError, match="outside their bound"):
                R.check(key, g, ref, 1.0, 1.0, ab)
    # the d emb contribution of down level 3 halved: time_embedding.* off by ~3e-2 - three times the fp16 bound, a third of the old
    # worst-parameter bar.  (The same fault one level up lands at 1.2e-1 with these inputs, just over the old bar: printed above.)
    if fault == "down3_emb_halved":
        assert not old["fp16"], "the halved d emb contribution of down level 3 was expected to pass the old bars on the fp16 build"


def test_resolution_of_the_fp16_bounds():
    """printed, not asserted: the smallest relative scale error of ONE transformer block's residual gradient (the dy that joins in
    the block's GroupNorm backward) that the fp16 per-parameter bounds catch, by bisection"""
    case = "wide_b3"; key = f"unet/{case}/fp16"
    P, _, ref, ab = _ref("unet", case)
    hit = lambda eps: bool(R.caught(key, R.restatement("unet", case, P, "fp16", fault=("xf_residual_scaled", 1.0 + eps))[1], ref, ab))
    lo, hi = 0.0, 0.5
    if not hit(hi):
        print(f"resolution: a {hi:.0%} scale error of {R.RESIDUAL_BLOCK}residual is not caught")
        return
    for _ in range(7):
        mid = 0.5 * (lo + hi)
        lo, hi = (lo, mid) if hit(mid) else (mid, hi)
    print(f"resolution: the fp16 bounds catch a scale error of the residual gradient of {R.RESIDUAL_BLOCK[:-1]} from {hi:.1%} (not at {lo:.1%})")
    assert not hit(0.0)
