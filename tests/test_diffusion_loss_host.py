"""The weighted training objective (diffute_amd.training.diffusion_loss, dmx_diffusion_loss) without a GPU: the Min-SNR-gamma table against
an independent float64 formula, the float64 restatement against a torch-composed loss, the error bound the GPU test holds the kernel's sums
to, the faults that bound and the bit comparison must catch, and the argument errors."""
import math

import numpy as np
import pytest
import torch

import loss_restatement as R

import diffute_amd as D
from diffute_amd import _cabi
from diffute_amd.training import diffusion_loss


def tables(sched):
    sa, sb = sched._coef_tables("cpu")
    return dict(abar=sched.alphas_cumprod.numpy(), sa=sa.numpy(), sb=sb.numpy())


def test_header_constants_match_the_restatement():
    assert (_cabi.LOSS_SQ_ALL, _cabi.LOSS_SQ_MASK, _cabi.LOSS_SQ_WEIGHTED, _cabi.LOSS_MASK_SUM, _cabi.LOSS_WEIGHT) == (0, 1, 2, 3, 4)
    assert _cabi.LOSS_ROW_FLOATS == len(R.FIELDS) and _cabi.LOSS_CHUNK == R.CHUNK
    assert R.depth(4 * 64 * 64) == 24 and R.depth(140) == 17
    assert {"dmx_diffusion_loss", "dmx_diffusion_loss_workspace_bytes"} <= set(_cabi.exported_symbols())


@pytest.mark.parametrize("pt", ["epsilon", "v_prediction"])
def test_loss_weights_against_the_independent_formula(pt):
    sched = D.DDPMScheduler(prediction_type=pt)
    abar = sched.alphas_cumprod.numpy()
    ones = sched.loss_weights(None)
    assert ones.dtype == torch.float64 and ones.shape == (1000,) and bool((ones == 1).all())
    w = sched.loss_weights(5.0)
    assert w.dtype == torch.float64 and w.shape == (1000,)
    np.testing.assert_allclose(w.numpy(), R.snr_weights(abar, 5.0, pt), rtol=1e-15, atol=0)
    snr = abar.astype(np.float64) / (1 - abar.astype(np.float64))
    assert snr[0] > 500 and snr[999] < 0.1 and (snr > 5).any() and (snr < 5).any()             # both branches of the min occur on the SD2 schedule
    if pt == "epsilon":
        assert w[999] == 1.0 and abs(float(w[0]) - 5 / snr[0]) < 1e-12
    else:
        assert abs(float(w[999]) - abar[999].astype(np.float64)) < 1e-12 and abs(float(w[0]) - 5 / (snr[0] + 1)) < 1e-12
    # the device copy is fp32 and cached per (device, gamma, prediction type)
    t5 = sched._loss_weight_table("cpu", 5.0)
    assert t5.dtype == torch.float32 and t5 is sched._loss_weight_table("cpu", 5.0) and t5 is not sched._loss_weight_table("cpu", 4.0)
    assert torch.equal(t5, w.to(torch.float32)) and sched._coef_tables("cpu")[0].shape == (1000,)


@pytest.mark.parametrize("bad", [0, -1.0, float("inf"), float("nan")])
def test_loss_weights_refuses_a_bad_gamma(bad):
    with pytest.raises(ValueError, match="snr_gamma"):
        D.DDIMScheduler().loss_weights(bad)


@pytest.mark.parametrize("pt", ["epsilon", "v_prediction"])
def test_float64_restatement_equals_a_torch_composed_loss(pt):
    sched = D.DDPMScheduler(prediction_type=pt)
    case = R.make_case(tables(sched), (3, 4, 8, 24), [0, 500, 999], "rect", pt, 5.0, 4.0, seed=1)
    pred, x0, noise, M = (torch.from_numpy(case[k]).double() for k in ("pred", "x0", "noise", "mask"))
    t = torch.from_numpy(case["t"])
    if pt == "epsilon":
        target = noise
    else:       # the fp32 get_velocity tensor (see the restatement's docstring), composed with torch
        sa, sb = (x[t].reshape(-1, 1, 1, 1) for x in sched._coef_tables("cpu"))
        target = (sa * noise.float() - sb * x0.float()).double()
    q = (pred - target) ** 2
    w = torch.from_numpy(case["wt"]).double()[t]
    m = 1 + 4.0 * M
    want = torch.stack([q.sum((1, 2, 3)), (M * q).sum((1, 2, 3)), (m * q).sum((1, 2, 3)), M.sum((1, 2, 3))], 1).numpy()
    got = R.sums64(case)
    np.testing.assert_allclose(got, want, rtol=1e-13)
    loss64 = float((w * (m * q).sum((1, 2, 3))).sum() / q.numel())
    loss = R.model_kernel(case)[2]
    # each record one rounding of a float64 sum of terms with 6 roundings; times the weight; 3 additions; times the rounded 1 / N: 7 more
    assert abs(float(loss) - loss64) <= R.bound(7, 6) * loss64


def test_the_sum_bound_holds_for_a_worse_order():
    """a purely serial float32 sum of the largest test shape's terms - an honest evaluation in a worse order, k = the number of terms - stays
    inside its own bound of the same form"""
    sched = D.DDPMScheduler(prediction_type="v_prediction")
    case = R.make_case(tables(sched), (1, 4, 64, 64), [500], "rect", "v_prediction", 5.0, 4.0, seed=2)
    r = R.restate(case)
    want = R.sums64(case)[0]
    M0 = np.ascontiguousarray(r["M"][:, :1])
    for name, terms, w64 in (("sq_all", r["q"], want[0]), ("sq_mask", r["Mq"], want[1]), ("sq_weighted", r["mq"], want[2]), ("mask_sum", M0, want[3])):
        serial = float(np.add.accumulate(terms.reshape(-1), dtype=np.float32)[-1])
        assert abs(serial - w64) <= R.bound(terms.size, R.ROUNDINGS[name]) * w64, name
    # the shape of the bound: first-order (k + r) u, and the kernel's k at this span is the documented 24
    assert R.bound(24, 4) == pytest.approx(28 * 2.0 ** -24, rel=1e-5)


def _fault_case(fault):
    v = fault == "v_target_swapped_signs"
    pt = "v_prediction" if v else "epsilon"
    sched = D.DDPMScheduler(prediction_type=pt)
    return R.make_case(tables(sched), (3, 4, 5, 7), [0, 500, 999], "rect", pt, 5.0, 4.0, seed=3)


def test_the_host_model_passes_the_checks():
    for fault in ("no_min", "v_target_swapped_signs"):           # (both prediction types)
        case = _fault_case(fault)
        R.verify(case, *R.model_kernel(case))
        R.verify(case, None, *R.model_kernel(case)[1:])


@pytest.mark.parametrize("fault", R.FAULTS)
def test_injected_faults_are_caught(fault):
    """each fault breaks the bit comparison of dpred or the bound of a sum on the 3 x 4 x 5 x 7 rectangle-mask case at t = 0, 500, 999,
    gamma = 5, lambda = 4 (v-prediction for the target fault, epsilon otherwise)"""
    case = _fault_case(fault)
    dp, rec, loss = R.model_kernel(case, fault)
    with pytest.raises(AssertionError, match="dpred differs|exceeds|weight field"):
        R.verify(case, dp, rec, loss)
    if fault in ("mask_not_broadcast", "v_target_swapped_signs"):            # these are visible in the sums alone
        with pytest.raises(AssertionError, match="exceeds"):
            R.verify(case, None, rec, loss)


def test_argument_errors_name_the_argument():
    sched = D.DDPMScheduler()
    p = torch.zeros(2, 4, 8, 8)
    t = torch.tensor([1, 2])
    for lam in (-1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="mask_weight"):
            diffusion_loss(p, p, p, t, sched, mask_weight=lam)
    with pytest.raises(ValueError, match="snr_gamma"):
        diffusion_loss(p, p, p, t, sched, snr_gamma=0.0)
    with pytest.raises(ValueError, match="mask"):
        diffusion_loss(p, p, p, t, sched, mask=torch.zeros(2, 4, 8, 8))
    with pytest.raises(ValueError, match="mask"):
        diffusion_loss(p, p, p, t, sched, mask=torch.zeros(2, 1, 8, 4))
    with pytest.raises(ValueError, match="timesteps"):
        diffusion_loss(p, p, p, torch.tensor([1, 2, 3]), sched)
    with pytest.raises(ValueError, match="latents"):
        diffusion_loss(p, torch.zeros(2, 4, 8, 4), p, t, sched)
    with pytest.raises(ValueError, match="noise"):
        diffusion_loss(p, p, torch.zeros(1, 4, 8, 8), t, sched)
    with pytest.raises(ValueError, match="pred"):
        diffusion_loss(torch.zeros(2, 4, 64), p, p, t, sched)
    with pytest.raises(RuntimeError, match="GPU"):                           # the scalar and shape checks come first; there is no CPU path
        diffusion_loss(p, p, p, t, sched, snr_gamma=5.0, mask_weight=4.0, mask=torch.zeros(2, 1, 8, 8))
    assert math.isfinite(float(sched.loss_weights(5.0).sum()))
