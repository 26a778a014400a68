"""DDPMScheduler / DDIMScheduler with the surface the reference uses:

  from_pretrained(path, subfolder="scheduler")   train_diffute_v1.py:628, app.ipynb:545
  .num_train_timesteps / .config.prediction_type  train_diffute_v1.py:892,904
  .add_noise / .get_velocity                      train_diffute_v1.py:897,907
  .init_noise_sigma / .set_timesteps / .timesteps app.ipynb:800,803-804
  .scale_model_input / .step(...).prev_sample     app.ipynb:810,816

Host logic (tables, integer timestep grids, the scalar coefficients of a step) is Python/torch,
written with the same tensor expressions as diffusers >=0.15 so it rounds identically on the same
machine; the elementwise update over the latents is a gfx950 kernel behind the C-ABI.

One step is one `_cabi.SchedRowRec` (`scheduler.plan(eta)`: the scalars, whether noise is added, the DPM-Solver++ history-ring
slots, the timestep).  The three `step()` methods, `pipeline.denoise()` and the in-flight engine (`inflight.py`) all read that
record; `launch_step` hands one to the scalar entry of its scheduler kind.
"""
import json
import math
import os
from types import SimpleNamespace

import numpy as np
import torch

from . import _cabi

SD2_SCHEDULER_CONFIG = dict(
    num_train_timesteps=1000, beta_start=0.00085, beta_end=0.012, beta_schedule="scaled_linear",
    prediction_type="epsilon", clip_sample=False, steps_offset=1, set_alpha_to_one=False,
    variance_type="fixed_small", timestep_spacing="leading")


class SchedulerOutput(SimpleNamespace):
    """`.prev_sample` (app.ipynb:816)."""


def launch_step(kind, rec, x, eps, noise, m1, m2, x0_out, out, vpred, stream):
    """One scalar scheduler step over fp32 CUDA tensors from its record: `kind` is the scheduler's (_cabi.SCHED_*), `out` may be `x`.
    DDIM / DDPM read rec.c and add the noise term when `noise` is given; DPM-Solver++ reads rec.order / rec.dpm, the previous data
    predictions m1 / m2 (None where the order does not read them) and writes this step's into x0_out."""
    lib, P = _cabi.lib(), _cabi.ptr
    if kind == _cabi.SCHED_DPMPP:
        rc = lib.dmx_sched_step_dpmpp(P(x), P(eps), P(m1), P(m2), P(x0_out), P(out), x.numel(), rec.order, rec.dpm, vpred, stream)
    else:
        fn = lib.dmx_sched_step_ddim if kind == _cabi.SCHED_DDIM else lib.dmx_sched_step_ddpm
        rc = fn(P(x), P(eps), P(noise), P(out), x.numel(), *rec.c, vpred, stream)
    _cabi.check(rc, ("sched_step_ddim", "sched_step_ddpm", "sched_step_dpmpp")[kind])


def launch_step_guided(kind, rec, x, eps, noise, hist, vpred, scale, rescale, stream, ratio_out=None):
    """One guided scheduler step in one launch (include/diffute_hip.h dmx_sched_step_guided): x / eps fp32 CUDA [2B, ...], rows [0,B) the
    conditional half and [B,2B) the unconditional one.  The classifier-free combination eu + scale * (ec - eu), with rescale != 0 the
    guidance rescale (per-sample std(ec) / std(g), Lin et al. 2023), then the update of `kind` from the record; prev_sample is written in
    place to row b AND row B + b of x.  noise [B, ...] or None; hist [n_hist, B, ...], the DPM-Solver++ ring (None otherwise);
    ratio_out fp32 [B] or None receives the per-sample ratios."""
    B2 = x.shape[0]
    if B2 < 2 or B2 % 2 or eps.shape != x.shape:
        raise ValueError(f"launch_step_guided: x {tuple(x.shape)} / eps {tuple(eps.shape)} must be [2B, ...] and agree")
    B = B2 // 2
    rc = _cabi.lib().dmx_sched_step_guided(_cabi.ptr(x), _cabi.ptr(eps), _cabi.ptr(noise), _cabi.ptr(hist), 0 if hist is None else hist.shape[0],
                                           rec, kind, vpred, float(scale), float(rescale), float(1 - rescale), _cabi.ptr(ratio_out), B,
                                           x.numel() // B2, stream)
    _cabi.check(rc, "sched_step_guided")


def launch_step_rows_guided(kind, x, eps, noise, hist, plan, row_index, guide, vpred, stream, ratio_out=None, lib=None):
    """The per-row guided scheduler step in one launch (include/diffute_hip.h dmx_sched_step_rows_guided): the in-flight engine's per-row
    step with a role per row.  x / eps fp32 CUDA [B, ...]; `plan` the device records and `row_index` int32 [B] as for the per-row entry;
    `guide` the device table of B _cabi.GuideRow (dmx_rows_guide writes it).  A PLAIN row is the per-row entry's update, a COND row the
    guided update of its pair - prev_sample into its own row and its UNCOND partner's -, idle and UNCOND rows are left alone.  noise
    [B, ...] or None; hist [n_hist, B, ...], the DPM-Solver++ ring (None otherwise); ratio_out fp32 [B] or None."""
    l = _cabi.lib() if lib is None else lib
    B = x.shape[0]
    rc = l.dmx_sched_step_rows_guided(_cabi.ptr(x), _cabi.ptr(eps), _cabi.ptr(noise), _cabi.ptr(hist), 0 if hist is None else hist.shape[0],
                                      _cabi.ptr(plan), _cabi.ptr(row_index), _cabi.ptr(guide), _cabi.ptr(ratio_out), B, x.numel() // B, kind,
                                      vpred, stream)
    _cabi.check(rc, "sched_step_rows_guided", l)


class Guidance:
    """Classifier-free guidance for denoise() and the edit functions: the model runs on the glyph context and on an unconditional one and
    the scheduler steps on eu + scale * (ec - eu).  rescale in [0, 1] is the guidance rescale of Lin et al. 2023 (diffusers'
    rescale_noise_cfg): the guided output scaled back towards the per-sample standard deviation of the conditional one.  uncond: the
    unconditional context - None is the all-zero context (what training_batch(context_dropout=) trains), a tensor [1,S,D] is shared by all
    rows, [N,S,D] is one per row.  scale == 1 with rescale == 0 is the plain loop (`active` is False): no unconditional rows are run.
    Everything is checked here or, against the conditional context, in check_context - on the host, before anything touches the device."""

    def __init__(self, scale, rescale=0.0, uncond=None):
        scale, rescale = float(scale), float(rescale)
        if not np.isfinite(scale):
            raise ValueError(f"Guidance: scale = {scale} is not finite")
        if not 0.0 <= rescale <= 1.0:                      # (NaN fails both comparisons)
            raise ValueError(f"Guidance: rescale = {rescale} outside [0, 1]")
        if uncond is not None:
            if not torch.is_tensor(uncond) or uncond.dim() != 3 or uncond.shape[0] < 1:
                raise ValueError("Guidance: uncond must be a tensor [1,S,D] or [N,S,D]")
            if not uncond.is_floating_point():
                raise ValueError(f"Guidance: uncond has dtype {uncond.dtype}, expected a floating-point context")
        self.scale, self.rescale, self.uncond = scale, rescale, uncond

    @property
    def active(self):
        return not (self.scale == 1.0 and self.rescale == 0.0)

    def check_context(self, ctx, N=None):
        """uncond against the conditional context [N,S,D] (N: the number of rows where ctx is not given whole)"""
        u = self.uncond
        if u is None:
            return
        N = ctx.shape[0] if N is None else N
        if tuple(u.shape[1:]) != tuple(ctx.shape[1:]) or u.shape[0] not in (1, N):
            raise ValueError(f"Guidance: uncond {tuple(u.shape)} does not fit {N} contexts of {tuple(ctx.shape[1:])}: expected "
                             f"[1,{ctx.shape[1]},{ctx.shape[2]}] or [{N},{ctx.shape[1]},{ctx.shape[2]}]")
        if u.dtype != ctx.dtype or u.device != ctx.device:
            raise ValueError(f"Guidance: uncond is {u.dtype} on {u.device}, the context {ctx.dtype} on {ctx.device}")

    def rows(self, index):
        """the guidance of the rows `index` (a slice or a list of row numbers) of a batch: a per-row uncond follows its rows"""
        if self.uncond is None or self.uncond.shape[0] == 1:
            return self
        return Guidance(self.scale, self.rescale, self.uncond[index])

    def uncond_for(self, ctx):
        """the unconditional context of the rows of `ctx` [B,S,D]"""
        if self.uncond is None:
            return torch.zeros_like(ctx)
        return self.uncond.expand(ctx.shape[0], -1, -1) if self.uncond.shape[0] == 1 else self.uncond


class _Config(SimpleNamespace):
    def __getitem__(self, k):
        return getattr(self, k)


class _SchedulerBase:
    order = 1
    kind = None                                  # _cabi.SCHED_*: which step kernel runs this class's records
    _config_defaults = SD2_SCHEDULER_CONFIG      # the class's own defaults; their keys (+ "thresholding") are what from_pretrained / from_config keep

    def __init__(self, **config):
        cfg = dict(self._config_defaults); cfg.update(config)
        self._check_config(cfg)
        self.config = _Config(**cfg)
        N = cfg["num_train_timesteps"]
        self.num_train_timesteps = N                      # read directly at train_diffute_v1.py:892
        if cfg["beta_schedule"] == "scaled_linear":
            self.betas = torch.linspace(cfg["beta_start"] ** 0.5, cfg["beta_end"] ** 0.5, N, dtype=torch.float32) ** 2
        elif cfg["beta_schedule"] == "linear":
            self.betas = torch.linspace(cfg["beta_start"], cfg["beta_end"], N, dtype=torch.float32)
        else:
            raise NotImplementedError(f"{cfg['beta_schedule']} is not implemented for {self.__class__}")
        self.alphas = 1.0 - self.betas
        self.alphas_cumprod = torch.cumprod(self.alphas, dim=0)
        self.one = torch.tensor(1.0)
        self.init_noise_sigma = 1.0                       # app.ipynb:800
        self.num_inference_steps = None
        self.timesteps = torch.from_numpy(np.arange(0, N)[::-1].copy().astype(np.int64))
        self._dev_tables = {}

    @staticmethod
    def _check_config(cfg):
        # options of the diffusers schedulers whose arithmetic is NOT implemented by the step kernels: refuse them instead of
        # silently computing something else (DDPMScheduler's own default is clip_sample=True; SD2's scheduler config sets False)
        if cfg.get("clip_sample"):
            raise NotImplementedError("clip_sample=True is not implemented (the SD2-inpainting scheduler config uses clip_sample=false)")
        if cfg.get("thresholding"):
            raise NotImplementedError("thresholding=True is not implemented")
        if cfg.get("variance_type", "fixed_small") != "fixed_small":
            raise NotImplementedError(f"variance_type={cfg['variance_type']!r} is not implemented (only 'fixed_small')")
        if cfg.get("timestep_spacing", "leading") != "leading":
            raise NotImplementedError(f"timestep_spacing={cfg['timestep_spacing']!r} is not implemented (only 'leading')")
        if cfg["prediction_type"] not in ("epsilon", "v_prediction"):
            raise NotImplementedError(f"prediction_type={cfg['prediction_type']!r} is not implemented")

    @classmethod
    def _known_keys(cls):
        return set(cls._config_defaults) | {"thresholding"}

    @classmethod
    def from_pretrained(cls, pretrained_model_name_or_path, subfolder=None, **kw):
        d = pretrained_model_name_or_path if subfolder is None else os.path.join(pretrained_model_name_or_path, subfolder)
        with open(os.path.join(d, "scheduler_config.json")) as f:
            cfg = json.load(f)
        known = cls._known_keys()
        return cls(**{k: v for k, v in cfg.items() if k in known})

    @classmethod
    def from_config(cls, config, **overrides):
        """`SchedulerB.from_config(scheduler_a.config)`, the diffusers idiom for swapping schedulers: `config` is a `.config`
        object or a dict; the keys this class knows are kept (overrides win), the rest are dropped."""
        cfg = dict(config) if isinstance(config, dict) else dict(vars(config))
        cfg.update(overrides)
        known = cls._known_keys()
        return cls(**{k: v for k, v in cfg.items() if k in known})

    def save_pretrained(self, save_directory):
        os.makedirs(save_directory, exist_ok=True)
        with open(os.path.join(save_directory, "scheduler_config.json"), "w") as f:
            json.dump(dict(vars(self.config), _class_name=type(self).__name__), f, indent=2)

    def __len__(self):
        return self.config.num_train_timesteps

    def scale_model_input(self, sample, timestep=None):
        """Identity for DDPM/DDIM (app.ipynb:810)."""
        return sample

    def _grid(self, num_inference_steps):
        N = self.config.num_train_timesteps
        if num_inference_steps > N:
            raise ValueError(f"`num_inference_steps`: {num_inference_steps} cannot be larger than {N}")
        step_ratio = N // num_inference_steps                              # integer index math (bit-exact)
        return (np.arange(0, num_inference_steps) * step_ratio).round()[::-1].copy().astype(np.int64)

    def previous_timestep(self, timestep):
        return int(timestep) - self.config.num_train_timesteps // self.num_inference_steps

    # ---- training-side helpers: per-sample coefficient gather on the host tables, update on the GPU
    def _coef_tables(self, device):
        key = str(device)
        if key not in self._dev_tables:
            sa = (self.alphas_cumprod ** 0.5).to(device)
            sb = ((1 - self.alphas_cumprod) ** 0.5).to(device)
            self._dev_tables[key] = (sa, sb)
        return self._dev_tables[key]

    def loss_weights(self, snr_gamma=None):
        """The per-timestep sample weight of the training loss, float64 [num_train_timesteps], computed in float64 from alphas_cumprod.
        None: 1 everywhere.  Otherwise Min-SNR-gamma (Hang et al., ICCV 2023; diffusers' --snr_gamma) with snr = abar / (1 - abar):
        min(snr, gamma) / snr for an epsilon model, min(snr, gamma) / (snr + 1) for a v model."""
        abar = self.alphas_cumprod.to(torch.float64)
        g = self._check_snr_gamma(snr_gamma)
        if g is None:
            return torch.ones_like(abar)
        snr = abar / (1 - abar)
        clipped = torch.minimum(snr, torch.full_like(snr, g))
        if self.config.prediction_type == "epsilon":
            return clipped / snr
        if self.config.prediction_type == "v_prediction":
            return clipped / (snr + 1)
        raise ValueError(f"Unknown prediction type {self.config.prediction_type}")

    @staticmethod
    def _check_snr_gamma(snr_gamma):
        if snr_gamma is None:
            return None
        g = float(snr_gamma)
        if not (math.isfinite(g) and g > 0):
            raise ValueError(f"snr_gamma must be finite and greater than 0, got {snr_gamma!r}")
        return g

    def _loss_weight_table(self, device, snr_gamma=None):
        """loss_weights(snr_gamma) as fp32 on `device`, cached per (device, snr_gamma, prediction_type) like _coef_tables"""
        key = (str(device), self._check_snr_gamma(snr_gamma), self.config.prediction_type)
        if key not in self._dev_tables:
            self._dev_tables[key] = self.loss_weights(snr_gamma).to(torch.float32).to(device)
        return self._dev_tables[key]

    def _mix(self, a, b, timesteps, velocity):
        _cabi.require_cuda(a, b)
        sa_t, sb_t = self._coef_tables(a.device)
        t = timesteps.to(a.device).reshape(-1).long()
        if t.numel() != a.shape[0]:
            raise ValueError("timesteps must have one entry per sample")
        sa = sa_t[t].contiguous(); sb = sb_t[t].contiguous()
        x = a.to(torch.float32).contiguous(); n = b.to(torch.float32).contiguous()
        out = torch.empty_like(x)
        fn = _cabi.lib().dmx_sched_get_velocity if velocity else _cabi.lib().dmx_sched_add_noise
        _cabi.check(fn(_cabi.ptr(x), _cabi.ptr(n), _cabi.ptr(sa), _cabi.ptr(sb), _cabi.ptr(out), x.shape[0],
                       x.numel() // x.shape[0], _cabi.current_stream()), "add_noise/get_velocity")
        return out.to(a.dtype)

    def add_noise(self, original_samples, noise, timesteps):
        """sqrt(abar_t) x0 + sqrt(1-abar_t) noise (train_diffute_v1.py:897)."""
        return self._mix(original_samples, noise, timesteps, False)

    def get_velocity(self, sample, noise, timesteps):
        """sqrt(abar_t) noise - sqrt(1-abar_t) sample (train_diffute_v1.py:907)."""
        return self._mix(sample, noise, timesteps, True)

    @staticmethod
    def _t_int(timestep):
        return int(timestep.item()) if torch.is_tensor(timestep) else int(timestep)

    def plan(self, eta=0.0):
        """One _cabi.SchedRowRec per step of the current grid (set_timesteps first): what the step kernels read for that step."""
        if self.num_inference_steps is None:
            raise ValueError("Number of inference steps is 'None', you need to run 'set_timesteps' after creating the scheduler")
        return list(self.iter_plan(eta))

    def iter_plan(self, eta=0.0):
        """plan(eta) one record at a time, each built when it is asked for: a loop that enqueues step i before it asks for step i + 1 computes
        the scalars (0-d torch expressions, about 0.1 ms of host time per step) behind the GPU work it has queued, not in front of it"""
        for i, t in enumerate(self.timesteps.tolist()):
            yield self._record(t, eta, i)

    def _step(self, rec, model_output, sample, generator, variance_noise, return_dict):
        """step() of DDIM / DDPM from the step's record"""
        x = sample.to(torch.float32).contiguous(); eps = model_output.to(torch.float32).contiguous()
        noise = None
        if rec.use_noise:
            if variance_noise is None:      # the reference passes no generator: device RNG (app.ipynb:816)
                variance_noise = torch.randn(x.shape, generator=generator, device=x.device, dtype=torch.float32)
            noise = variance_noise.to(torch.float32).contiguous()
        out = torch.empty_like(x)
        launch_step(self.kind, rec, x, eps, noise, None, None, None, out, self._vpred(), _cabi.current_stream())
        out = out.to(sample.dtype)
        return SchedulerOutput(prev_sample=out) if return_dict else (out,)

    def _vpred(self):
        return int(self.config.prediction_type == "v_prediction")


class DDPMScheduler(_SchedulerBase):
    """The scheduler the reference instantiates (app.ipynb:545, train_diffute_v1.py:628).

    `steps_offset`: implemented is the behaviour of the diffusers release the reference was written against (0.15-era,
    SURVEY Appendix A.3): DDPMScheduler.set_timesteps does NOT add `steps_offset` to the leading-spaced grid (the inference
    grid ends at timestep 0), while DDIMScheduler does.  Later diffusers releases apply the offset to DDPM as well.  The SD2
    `scheduler_config.json` carries `steps_offset: 1`; the key is kept in `.config` (round trip through save_pretrained) and a
    warning says once per process that the DDPM grid ignores it."""
    kind = _cabi.SCHED_DDPM
    _warned_offset = False

    def __init__(self, **config):
        super().__init__(**config)
        if int(self.config.steps_offset) != 0 and not DDPMScheduler._warned_offset:
            DDPMScheduler._warned_offset = True
            import warnings
            warnings.warn(f"DDPMScheduler: steps_offset={self.config.steps_offset} is kept in the config but NOT applied to the "
                          "inference grid (the behaviour of the diffusers release the reference uses; later releases add it)", stacklevel=2)

    def set_timesteps(self, num_inference_steps, device=None):
        self.num_inference_steps = int(num_inference_steps)
        self.timesteps = torch.from_numpy(self._grid(self.num_inference_steps))
        if device is not None:
            self.timesteps = self.timesteps.to(device)

    def step_coefficients(self, timestep):
        """(sqrt_beta_prod_t, sqrt_alpha_prod_t, coef_x0, coef_xt, sigma) as python floats holding fp32 values."""
        t = self._t_int(timestep)
        if self.num_inference_steps is None:
            raise ValueError("Number of inference steps is 'None', you need to run 'set_timesteps' after creating the scheduler")
        prev_t = self.previous_timestep(t)
        alpha_prod_t = self.alphas_cumprod[t]
        alpha_prod_t_prev = self.alphas_cumprod[prev_t] if prev_t >= 0 else self.one
        beta_prod_t = 1 - alpha_prod_t
        beta_prod_t_prev = 1 - alpha_prod_t_prev
        current_alpha_t = alpha_prod_t / alpha_prod_t_prev
        current_beta_t = 1 - current_alpha_t
        c0 = (alpha_prod_t_prev ** (0.5) * current_beta_t) / beta_prod_t
        c1 = current_alpha_t ** (0.5) * beta_prod_t_prev / beta_prod_t
        sigma = torch.tensor(0.0)
        if t > 0:
            variance = (1 - alpha_prod_t_prev) / (1 - alpha_prod_t) * current_beta_t
            variance = torch.clamp(variance, min=1e-20)                 # fixed_small
            sigma = variance ** 0.5
        return (float(beta_prod_t ** 0.5), float(alpha_prod_t ** 0.5), float(c0), float(c1), float(sigma))

    def _record(self, t, eta=0.0, i=None):
        r = _cabi.SchedRowRec(timestep=t, use_noise=int(t > 0))
        r.c[:] = self.step_coefficients(t)
        return r

    def step(self, model_output, timestep, sample, generator=None, variance_noise=None, return_dict=True):
        _cabi.require_cuda(model_output, sample)
        rec = self._record(self._t_int(timestep))
        return self._step(rec, model_output, sample, generator, variance_noise, return_dict)


class DDIMScheduler(_SchedulerBase):
    """Named by BASELINE.json's north_star (deterministic eta=0 sampler); same surface as DDPM."""
    kind = _cabi.SCHED_DDIM

    def __init__(self, **config):
        super().__init__(**config)
        self.final_alpha_cumprod = torch.tensor(1.0) if self.config.set_alpha_to_one else self.alphas_cumprod[0]

    def set_timesteps(self, num_inference_steps, device=None):
        self.num_inference_steps = int(num_inference_steps)
        ts = self._grid(self.num_inference_steps) + np.int64(self.config.steps_offset)
        self.timesteps = torch.from_numpy(ts)
        if device is not None:
            self.timesteps = self.timesteps.to(device)

    def step_coefficients(self, timestep, eta=0.0):
        """(sqrt_beta_prod_t, sqrt_alpha_prod_t, sqrt_alpha_prod_prev, dir_coef, std_dev)."""
        t = self._t_int(timestep)
        if self.num_inference_steps is None:
            raise ValueError("Number of inference steps is 'None', you need to run 'set_timesteps' after creating the scheduler")
        prev_t = self.previous_timestep(t)
        alpha_prod_t = self.alphas_cumprod[t]
        alpha_prod_t_prev = self.alphas_cumprod[prev_t] if prev_t >= 0 else self.final_alpha_cumprod
        beta_prod_t = 1 - alpha_prod_t
        beta_prod_t_prev = 1 - alpha_prod_t_prev
        variance = (beta_prod_t_prev / beta_prod_t) * (1 - alpha_prod_t / alpha_prod_t_prev)
        std_dev_t = eta * variance ** (0.5)
        dir_coef = (1 - alpha_prod_t_prev - std_dev_t ** 2) ** (0.5)
        return (float(beta_prod_t ** 0.5), float(alpha_prod_t ** 0.5), float(alpha_prod_t_prev ** 0.5),
                float(dir_coef), float(std_dev_t))

    def _record(self, t, eta=0.0, i=None):
        r = _cabi.SchedRowRec(timestep=t, use_noise=int(eta > 0))
        r.c[:] = self.step_coefficients(t, eta)
        return r

    def step(self, model_output, timestep, sample, eta=0.0, generator=None, variance_noise=None, return_dict=True):
        _cabi.require_cuda(model_output, sample)
        rec = self._record(self._t_int(timestep), eta)
        return self._step(rec, model_output, sample, generator, variance_noise, return_dict)


DPM_SOLVER_CONFIG = dict(
    num_train_timesteps=1000, beta_start=0.00085, beta_end=0.012, beta_schedule="scaled_linear", prediction_type="epsilon",
    solver_order=2, algorithm_type="dpmsolver++", solver_type="midpoint", lower_order_final=True,
    timestep_spacing="linspace", steps_offset=1, clip_sample=False, thresholding=False, use_karras_sigmas=False)


class DPMSolverMultistepScheduler(_SchedulerBase):
    """DPM-Solver++ multistep (Lu et al. 2022, arXiv 2211.01095, Alg. 2), orders 1-3, in the tensor form of diffusers >=0.15's
    DPMSolverMultistepScheduler: the deterministic ~20-step replacement of DDIM-50 / DDPM-150 for eps / v models.  Betas and
    prediction_type as SD2_SCHEDULER_CONFIG; the grid defaults to "linspace" (diffusers' default for this class).

    The scalars of every step (order plus the parenthesised 0-d fp32 expressions of diffusers' update) are computed on the host
    once per set_timesteps (plan() / step_plan()); the elementwise update - data prediction m0, the multistep combination with
    the previous m0's - is one kernel (launch_step).  step() keeps the m0 history itself, as diffusers does, so the
    reference-shaped loop works unchanged; denoise() keeps its own fixed buffers instead.

    Refused (NotImplementedError): thresholding, algorithm_type other than "dpmsolver++", Karras / Lu sigmas, "trailing" spacing,
    clip_sample, euler_at_final=True and any final_sigmas_type but "sigma_min" (the last step lands on timestep 0 - diffusers'
    "zero" would land on sigma = 0).  The solver is deterministic: no noise, no eta."""
    kind = _cabi.SCHED_DPMPP
    _config_defaults = DPM_SOLVER_CONFIG

    def __init__(self, **config):
        super().__init__(**config)
        ac = self.alphas_cumprod
        self.alpha_t = torch.sqrt(ac)
        self.sigma_t = torch.sqrt(1 - ac)
        self.lambda_t = torch.log(self.alpha_t) - torch.log(self.sigma_t)
        self._ts = np.zeros(0, dtype=np.int64)
        self._plan = []
        self._history = []
        self._step_index = None

    @staticmethod
    def _check_config(cfg):
        if cfg.get("clip_sample"):
            raise NotImplementedError("clip_sample=True is not implemented")
        if cfg.get("thresholding"):
            raise NotImplementedError("thresholding=True is not implemented")
        if cfg["algorithm_type"] != "dpmsolver++":
            raise NotImplementedError(f"algorithm_type={cfg['algorithm_type']!r} is not implemented (only 'dpmsolver++')")
        if cfg.get("use_karras_sigmas") or cfg.get("use_lu_lambdas"):
            raise NotImplementedError("use_karras_sigmas / use_lu_lambdas are not implemented")
        if cfg["timestep_spacing"] not in ("linspace", "leading"):
            raise NotImplementedError(f"timestep_spacing={cfg['timestep_spacing']!r} is not implemented (only 'linspace', 'leading')")
        if cfg.get("euler_at_final"):
            raise NotImplementedError("euler_at_final=True is not implemented")
        if cfg.get("final_sigmas_type", "sigma_min") != "sigma_min":
            raise NotImplementedError(f"final_sigmas_type={cfg['final_sigmas_type']!r} is not implemented (the last step lands on timestep 0)")
        if cfg["solver_type"] not in ("midpoint", "heun"):
            raise NotImplementedError(f"solver_type={cfg['solver_type']!r} is not implemented (only 'midpoint', 'heun')")
        if cfg["prediction_type"] not in ("epsilon", "v_prediction"):
            raise NotImplementedError(f"prediction_type={cfg['prediction_type']!r} is not implemented")
        if cfg["solver_order"] not in (1, 2, 3):
            raise ValueError(f"solver_order={cfg['solver_order']!r}: 1, 2 or 3")

    @classmethod
    def _known_keys(cls):
        return set(cls._config_defaults) | {"euler_at_final", "final_sigmas_type", "use_lu_lambdas"}

    def _grid(self, num_inference_steps):
        N = self.config.num_train_timesteps
        if num_inference_steps > N:
            raise ValueError(f"`num_inference_steps`: {num_inference_steps} cannot be larger than {N}")
        n = num_inference_steps
        if self.config.timestep_spacing == "linspace":
            ts = np.linspace(0, N - 1, n + 1).round()[::-1][:-1].copy().astype(np.int64)
        else:                                                              # "leading"
            ts = (np.arange(0, n + 1) * (N // (n + 1))).round()[::-1][:-1].copy().astype(np.int64) + np.int64(self.config.steps_offset)
        _, first = np.unique(ts, return_index=True)                        # dense grids round to repeated timesteps: keep the first of each
        return ts[np.sort(first)]

    def set_timesteps(self, num_inference_steps, device=None):
        """The grid (deduplicated, so num_inference_steps may come out smaller than asked), the step plan, an empty history."""
        ts = self._grid(int(num_inference_steps))
        self.num_inference_steps = len(ts)
        self.timesteps = torch.from_numpy(ts)
        if device is not None:
            self.timesteps = self.timesteps.to(device)
        self._ts = ts
        self._plan = [(o, _cabi.DpmCoefs(**c)) for o, c in self._make_plan(ts)]
        self._history = []
        self._step_index = None

    def _orders(self, n):
        k = self.config.solver_order
        low = self.config.lower_order_final and n < 15
        out = []
        for i in range(n):
            if k == 1 or i == 0 or (low and i == n - 1):
                out.append(1)
            elif k == 2 or i == 1 or (low and i == n - 2):
                out.append(2)
            else:
                out.append(3)
        return out

    def _make_plan(self, ts):
        """Per step: (order, {dmx_dpm_coefs field: python float holding the fp32 value}), with diffusers' 0-d fp32 expressions."""
        lam, al, sg = self.lambda_t, self.alpha_t, self.sigma_t
        heun = self.config.solver_type == "heun"
        plan = []
        for i, o in enumerate(self._orders(len(ts))):
            s0 = int(ts[i]); t = int(ts[i + 1]) if i + 1 < len(ts) else 0
            alpha_t, sigma_t, lambda_t = al[t], sg[t], lam[t]
            alpha_s0, sigma_s0, lambda_s0 = al[s0], sg[s0], lam[s0]
            h = lambda_t - lambda_s0
            c = dict(alpha_s0=alpha_s0, sigma_s0=sigma_s0, c_x=sigma_t / sigma_s0, c_m0=alpha_t * (torch.exp(-h) - 1.0),
                     c_d1=0.0, c_d2=0.0, inv_r0=0.0, inv_r1=0.0, r0_over_r01=0.0, inv_r01=0.0)
            if o >= 2:
                h_0 = lambda_s0 - lam[int(ts[i - 1])]
                r0 = h_0 / h
                c["inv_r0"] = 1.0 / r0
                if o == 2 and not heun:      # midpoint: "- 0.5 * (alpha_t * (exp(-h) - 1.0)) * D1", the sign carried by the coefficient
                    c["c_d1"] = -(0.5 * (alpha_t * (torch.exp(-h) - 1.0)))
                else:
                    c["c_d1"] = alpha_t * ((torch.exp(-h) - 1.0) / h + 1.0)
            if o == 3:
                h_1 = lam[int(ts[i - 1])] - lam[int(ts[i - 2])]
                r1 = h_1 / h
                c["inv_r1"] = 1.0 / r1
                c["r0_over_r01"] = r0 / (r0 + r1)
                c["inv_r01"] = 1.0 / (r0 + r1)
                c["c_d2"] = alpha_t * ((torch.exp(-h) - 1.0 + h) / h ** 2 - 0.5)
            plan.append((o, {k: float(v) for k, v in c.items()}))
        return plan

    def _record(self, t, eta, i):
        """step i of the grid: its order and coefficients, the history slots it writes (i % k) and reads ((i-1) % k, (i-2) % k); the solver is
        deterministic, eta plays no part"""
        k = int(self.config.solver_order)
        order, c = self._plan[i]
        return _cabi.SchedRowRec(dpm=c, order=order, ring_w=i % k, ring_m1=(i - 1) % k, ring_m2=(i - 2) % k, timestep=t)

    def step_plan(self):
        """[(order, {coefficient: float})] of every step of the current grid - what step() and denoise() hand to the kernel."""
        if self.num_inference_steps is None:
            raise ValueError("Number of inference steps is 'None', you need to run 'set_timesteps' after creating the scheduler")
        return [(o, {k: getattr(c, k) for k, _ in c._fields_}) for o, c in self._plan]

    def step(self, model_output, timestep, sample, return_dict=True):
        """One solver step; the steps of the grid are taken in order (set_timesteps starts over)."""
        _cabi.require_cuda(model_output, sample)
        if self.num_inference_steps is None:
            raise ValueError("Number of inference steps is 'None', you need to run 'set_timesteps' after creating the scheduler")
        t = self._t_int(timestep)
        i = self._step_index
        if i is None:
            hits = np.flatnonzero(self._ts == t)
            i = int(hits[0]) if len(hits) else len(self._ts)
        if i >= len(self._ts) or int(self._ts[i]) != t:
            raise ValueError(f"step(): timestep {t} is not the next step of the grid (a multistep solver takes its steps in order; "
                             "call set_timesteps to start over)")
        rec = self._record(t, 0.0, i)
        x = sample.to(torch.float32).contiguous(); e = model_output.to(torch.float32).contiguous()
        m1 = self._history[-1] if rec.order >= 2 else None
        m2 = self._history[-2] if rec.order >= 3 else None
        x0 = torch.empty_like(x); out = torch.empty_like(x)
        launch_step(self.kind, rec, x, e, None, m1, m2, x0, out, self._vpred(), _cabi.current_stream())
        k = self.config.solver_order
        self._history = (self._history + [x0])[1 - k:] if k > 1 else []
        self._step_index = i + 1
        out = out.to(sample.dtype)
        return SchedulerOutput(prev_sample=out) if return_dict else (out,)
