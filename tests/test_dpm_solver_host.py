"""DPMSolverMultistepScheduler on the host (no GPU): grids, order plan, step coefficients, refusals, config round trips, and the
published update itself (tests/dpm_restatement.py) on a problem with a closed-form solution."""
import json

import numpy as np
import pytest
import torch

import dpm_restatement as R

LINSPACE_20 = [999, 949, 899, 849, 799, 749, 699, 649, 599, 549, 500, 450, 400, 350, 300, 250, 200, 150, 100, 50]
LEADING_20 = [941, 894, 847, 800, 753, 706, 659, 612, 565, 518, 471, 424, 377, 330, 283, 236, 189, 142, 95, 48]


def _grid(n, spacing, N=1000, offset=1):
    if spacing == "linspace":
        ts = np.linspace(0, N - 1, n + 1).round()[::-1][:-1].copy().astype(np.int64)
    else:
        ts = (np.arange(0, n + 1) * (N // (n + 1))).round()[::-1][:-1].copy().astype(np.int64) + offset
    _, idx = np.unique(ts, return_index=True)
    return ts[np.sort(idx)]


def test_grids():
    import diffute_amd as D
    s = D.DPMSolverMultistepScheduler()
    assert s.config.timestep_spacing == "linspace" and D.DDPMScheduler().config.timestep_spacing == "leading"
    s.set_timesteps(20)
    assert s.timesteps.tolist() == LINSPACE_20 and s.num_inference_steps == 20 and s.timesteps.dtype == torch.int64
    lead = D.DPMSolverMultistepScheduler(timestep_spacing="leading")
    lead.set_timesteps(20)
    assert lead.timesteps.tolist() == LEADING_20
    for spacing, sch in (("linspace", s), ("leading", lead)):
        for n in (1, 10, 50, 1000):
            sch.set_timesteps(n)
            ref = _grid(n, spacing)
            assert sch.timesteps.tolist() == ref.tolist(), (spacing, n)
            assert sch.num_inference_steps == len(ref)
            assert len(set(ref.tolist())) == len(ref) and np.all(np.diff(ref) < 0)
    s.set_timesteps(1000)                                    # linspace(0, 999, 1001) rounds to repeated timesteps
    assert s.num_inference_steps < 1000 and s.timesteps.tolist() == sorted(set(s.timesteps.tolist()), reverse=True)
    s.set_timesteps(1)
    assert s.timesteps.tolist() == [999]


def test_order_plan():
    import diffute_amd as D
    s = D.DPMSolverMultistepScheduler()
    s.set_timesteps(20)
    assert [o for o, _ in s.step_plan()] == [1] + [2] * 19
    s.set_timesteps(10)
    assert [o for o, _ in s.step_plan()] == [1] + [2] * 8 + [1]
    s3 = D.DPMSolverMultistepScheduler(solver_order=3)
    s3.set_timesteps(10)
    assert [o for o, _ in s3.step_plan()] == [1, 2] + [3] * 6 + [2, 1]
    s3.set_timesteps(20)
    assert [o for o, _ in s3.step_plan()] == [1, 2] + [3] * 18
    s1 = D.DPMSolverMultistepScheduler(solver_order=1)
    s1.set_timesteps(20)
    assert [o for o, _ in s1.step_plan()] == [1] * 20
    nolow = D.DPMSolverMultistepScheduler(lower_order_final=False)
    nolow.set_timesteps(10)
    assert [o for o, _ in nolow.step_plan()] == [1] + [2] * 9
    for n in (10, 20):
        s3.set_timesteps(n)
        assert [o for o, _ in s3.step_plan()] == R.orders(n, 3)


def _restated_coefs(tab, ts, i, order, solver_type):
    """The parenthesised scalars of dpm_restatement.step, each as its own 0-d expression."""
    al, sg, lam = tab
    s0 = int(ts[i]); t = int(ts[i + 1]) if i + 1 < len(ts) else 0
    alpha_t, sigma_t, lambda_t = al[t], sg[t], lam[t]
    alpha_s0, sigma_s0, lambda_s0 = al[s0], sg[s0], lam[s0]
    h = lambda_t - lambda_s0
    c = dict(alpha_s0=alpha_s0, sigma_s0=sigma_s0, c_x=sigma_t / sigma_s0, c_m0=alpha_t * (torch.exp(-h) - 1.0))
    if order >= 2:
        r0 = (lambda_s0 - lam[int(ts[i - 1])]) / h
        c["inv_r0"] = 1.0 / r0
        c["c_d1"] = (-(0.5 * (alpha_t * (torch.exp(-h) - 1.0))) if order == 2 and solver_type == "midpoint"
                     else alpha_t * ((torch.exp(-h) - 1.0) / h + 1.0))
    if order == 3:
        r1 = (lam[int(ts[i - 1])] - lam[int(ts[i - 2])]) / h
        c.update(inv_r1=1.0 / r1, r0_over_r01=r0 / (r0 + r1), inv_r01=1.0 / (r0 + r1),
                 c_d2=alpha_t * ((torch.exp(-h) - 1.0 + h) / h ** 2 - 0.5))
    return {k: float(v) for k, v in c.items()}


@pytest.mark.parametrize("order,solver_type", [(1, "midpoint"), (2, "midpoint"), (2, "heun"), (3, "midpoint"), (3, "heun")])
def test_step_plan_coefficients(order, solver_type):
    import diffute_amd as D
    s = D.DPMSolverMultistepScheduler(solver_order=order, solver_type=solver_type)
    tab = R.tables(s.alphas_cumprod)
    for a, b in zip(tab, (s.alpha_t, s.sigma_t, s.lambda_t)):
        assert torch.equal(a, b)
    for n in (10, 20, 25):
        s.set_timesteps(n)
        ts = s.timesteps.tolist()
        plan = s.step_plan()
        assert len(plan) == len(ts)
        for i, (o, c) in enumerate(plan):
            want = _restated_coefs(tab, ts, i, o, solver_type)
            for k, v in want.items():
                assert c[k] == v, (n, i, k, c[k], v)
            assert all(c[k] == 0.0 for k in c if k not in want)          # fields this order does not read


def test_refusals():
    import diffute_amd as D
    for bad in (dict(thresholding=True), dict(algorithm_type="dpmsolver"), dict(algorithm_type="sde-dpmsolver++"),
                dict(use_karras_sigmas=True), dict(timestep_spacing="trailing"), dict(clip_sample=True), dict(euler_at_final=True),
                dict(final_sigmas_type="zero"), dict(solver_type="bh2"), dict(prediction_type="sample")):
        with pytest.raises(NotImplementedError):
            D.DPMSolverMultistepScheduler(**bad)
    for order in (0, 4):
        with pytest.raises(ValueError):
            D.DPMSolverMultistepScheduler(solver_order=order)
    D.DPMSolverMultistepScheduler(euler_at_final=False, final_sigmas_type="sigma_min")       # the defaults are accepted
    with pytest.raises(ValueError):
        D.DPMSolverMultistepScheduler().step_plan()                                          # before set_timesteps


def test_from_config_both_directions(tmp_path):
    import diffute_amd as D
    cfg = dict(D.SD2_SCHEDULER_CONFIG, prediction_type="v_prediction", _class_name="DDPMScheduler", _diffusers_version="0.15.0")
    (tmp_path / "scheduler").mkdir()
    (tmp_path / "scheduler" / "scheduler_config.json").write_text(json.dumps(cfg))
    ddpm = D.DDPMScheduler.from_pretrained(str(tmp_path), subfolder="scheduler")
    dpm = D.DPMSolverMultistepScheduler.from_config(ddpm.config)
    assert isinstance(dpm, D.DPMSolverMultistepScheduler)
    assert dpm.config.prediction_type == "v_prediction" and dpm.config.timestep_spacing == "leading"     # the config's, not the default
    assert dpm.config.solver_order == 2 and dpm.config.algorithm_type == "dpmsolver++"
    assert not hasattr(dpm.config, "variance_type") and not hasattr(dpm.config, "set_alpha_to_one")
    assert torch.equal(dpm.alphas_cumprod, ddpm.alphas_cumprod)
    dpm.set_timesteps(20)
    assert dpm.timesteps.tolist() == LEADING_20
    back = D.DDPMScheduler.from_config(dpm.config)
    assert isinstance(back, D.DDPMScheduler)
    assert {k: v for k, v in vars(back.config).items() if k != "thresholding"} == vars(ddpm.config) and back.config.thresholding is False
    ddim = D.DDIMScheduler.from_config(vars(dpm.config))                                      # a dict works too
    assert ddim.config.prediction_type == "v_prediction"
    o = D.DPMSolverMultistepScheduler.from_config(ddpm.config, solver_order=3, timestep_spacing="linspace", not_a_key=1)
    assert o.config.solver_order == 3 and o.config.timestep_spacing == "linspace" and not hasattr(o.config, "not_a_key")
    with pytest.raises(NotImplementedError):       # a default DPM grid is "linspace", which the DDIM / DDPM classes refuse
        D.DDIMScheduler.from_config(D.DPMSolverMultistepScheduler().config)


def test_save_from_pretrained_round_trip(tmp_path):
    import diffute_amd as D
    s = D.DPMSolverMultistepScheduler(solver_order=3, solver_type="heun", prediction_type="v_prediction", lower_order_final=False)
    s.save_pretrained(str(tmp_path))
    saved = json.loads((tmp_path / "scheduler_config.json").read_text())
    assert saved["_class_name"] == "DPMSolverMultistepScheduler" and saved["solver_order"] == 3
    r = D.DPMSolverMultistepScheduler.from_pretrained(str(tmp_path))
    assert vars(r.config) == vars(s.config)
    s.set_timesteps(12); r.set_timesteps(12)
    assert torch.equal(s.timesteps, r.timesteps) and s.step_plan() == r.step_plan()


@pytest.mark.parametrize("order,solver_type,min_ratio", [(1, "midpoint", 1.8), (2, "midpoint", 2.7), (2, "heun", 2.7), (3, "midpoint", 3.5)])
def test_restatement_converges_on_gaussian_data(order, solver_type, min_ratio):
    """x0 ~ N(mu, I): the restated solver with the exact eps converges to the closed-form ODE solution at its order (80 -> 160 steps
    on the linspace grid; below ~40 steps the large final lambda-step dominates and the ratios mean nothing)."""
    import diffute_amd as D
    errs = {}
    for n in (80, 160):
        s = D.DPMSolverMultistepScheduler(solver_order=order, solver_type=solver_type)
        s.set_timesteps(n)
        ts = s.timesteps.tolist()
        tab = R.tables(s.alphas_cumprod)
        g = R.Gaussian(tab, ts[0])
        x, hist = g.xT.clone(), []
        for i, o in enumerate(R.orders(len(ts), order)):
            x, m0 = R.step(tab, ts, i, x, g.eps(x, ts[i]), hist, o, solver_type)
            hist.append(m0)
        errs[n] = g.rel_err(x)
    assert errs[80] / errs[160] >= min_ratio, errs
    if order == 2 and solver_type == "midpoint":
        s1 = D.DPMSolverMultistepScheduler(solver_order=1)
        s1.set_timesteps(160)
        ts = s1.timesteps.tolist()
        tab = R.tables(s1.alphas_cumprod)
        g = R.Gaussian(tab, ts[0])
        x = g.xT.clone()
        for i in range(len(ts)):
            x, _ = R.step(tab, ts, i, x, g.eps(x, ts[i]), [], 1)
        assert errs[160] <= 0.35 * g.rel_err(x), (errs[160], g.rel_err(x))
