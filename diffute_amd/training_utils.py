"""`EMAModel` - diffusers.training_utils.EMAModel (0.15-era call shape) for the reference's `--use_ema` path.

Reference (train_diffute_v1.py): `EMAModel(ema_unet.parameters(), model_cls=UNet2DConditionModel, model_config=ema_unet.config)`
(:642-646), `ema_unet.save_pretrained(out/"unet_ema")` in the save hook (:664-666), `EMAModel.from_pretrained(in/"unet_ema",
UNet2DConditionModel)` + `load_state_dict` + `.to(device)` in the load hook (:674-678), `ema_unet.to(accelerator.device)`
(:784-785) and `ema_unet.step(unet.parameters())` after every synced step (:934-935).

The per-element arithmetic is diffusers' `s.sub_((1 - decay) * (s - p))` (or `s.copy_(p)` for a parameter with
requires_grad=False), bit for bit:
  - GPU tensors: one launch of dmx_ema_step_multi over a cached device chunk table (all tensors, any of fp32 / bf16 / fp16);
    copy_to / store / restore are one dmx_copy_multi launch.
  - CPU tensors (the reference builds the EMA on the CPU before `.to(device)`): the same expression in torch.
  - A diffute_amd.UNet2DConditionModel trained by FusedAdamW: the weights live in the optimizer's fp32 master arena (the
    torch Parameters are stale until `sync_to_model()`).  The shadow then lives in the same packed layout and each step
    is one dmx_ema_step_multi launch over the arena (master -> shadow), with no per-step sync; the torch-layout shadows are
    exported only when someone reads `shadow_params`, `state_dict()` or `save_pretrained()`.
`FusedAdamW(ema_decay=...)` keeps its own in-kernel EMA (it forms `1.0f - (float)decay` where diffusers rounds the double
`1 - decay`): the two agree to ~1e-5 relative, not bit for bit.
"""
import copy
import ctypes
import json
import os

import numpy as np
import torch

from . import _cabi

_DT = {torch.float32: _cabi.DT_F32, torch.bfloat16: _cabi.DT_BF16, torch.float16: _cabi.DT_F16}
_EMA, _COPY = _cabi.MULTI_EMA, _cabi.MULTI_COPY
_CHUNK = 65536                                                          # elements per table entry (a multiple of 4: aligned tensors give aligned chunks)
_ENTRY = np.dtype(_cabi.MultiChunk)                                     # include/diffute_hip.h dmx_multi_chunk


def _runs_to_table(runs):
    """[(dst_addr, src_addr, n, dst_dtype, src_dtype, mode, elem_dst, elem_src)] -> numpy array of dmx_multi_chunk entries"""
    rows = []
    for dst, src, n, dd, sd, mode, ed, es in runs:
        for o in range(0, n, _CHUNK):
            rows.append((dst + o * ed, src + o * es, min(_CHUNK, n - o), dd, sd, mode, 0))
    return np.array(rows, dtype=_ENTRY)


class _DeviceTable:
    """a chunk table uploaded stream-ordered (pinned staging buffer kept alive with it: no host sync)"""

    def __init__(self, arr, device):
        self.nchunks = int(arr.shape[0])
        self.elements = int(arr["count"].sum()) if self.nchunks else 0
        host = torch.from_numpy(arr.view(np.uint8).copy())
        self._pinned = host.pin_memory()
        self.dev = torch.empty(host.numel(), dtype=torch.uint8, device=device)
        with torch.cuda.device(device):
            self.dev.copy_(self._pinned, non_blocking=True)


def _element_runs(dsts, srcs, modes):
    runs = []
    for d, s, m in zip(dsts, srcs, modes):
        n = d.numel()
        if n:
            runs.append((d.data_ptr(), s.data_ptr(), n, _DT[d.dtype], _DT[s.dtype], m, d.element_size(), s.element_size()))
    return runs


def _check_kernel_operands(dsts, srcs, what):
    dev = dsts[0].device if dsts else None
    for d, s in zip(dsts, srcs):
        if d.device != dev or s.device != dev:
            raise RuntimeError(f"EMAModel.{what}: every shadow and parameter must be on the same device ({dev}); got {d.device} / {s.device}")
        if d.shape != s.shape:
            raise RuntimeError(f"EMAModel.{what}: shape mismatch {tuple(d.shape)} vs {tuple(s.shape)}")
        if d.dtype not in _DT or s.dtype not in _DT:
            raise NotImplementedError(f"EMAModel.{what}: dtype {d.dtype} / {s.dtype} (fp32, bf16 and fp16 are implemented)")
        if not (d.is_contiguous() and s.is_contiguous()):
            raise NotImplementedError(f"EMAModel.{what}: non-contiguous tensors are not implemented")
    return dev


def _owner_of(params, full=True):
    """the live diffute_amd model whose parameters `params` are (all of them when `full`, else a subset; any order)
    -> (model, names) or (None, None)"""
    from .models import _LIVE_MODELS
    if not params:
        return None, None
    for m in list(_LIVE_MODELS):
        named = m.__dict__.get("_ema_param_ids")
        if named is None or len(named) != len(m._keys):
            named = m.__dict__["_ema_param_ids"] = dict((id(p), k) for k, p in m.named_parameters())
        if id(params[0]) not in named or (full and len(named) != len(params)):
            continue
        if all(id(p) in named for p in params):
            return m, [named[id(p)] for p in params]
    return None, None


class EMAModel:
    """Exponential moving average of model parameters - diffusers.training_utils.EMAModel as train_diffute_v1.py uses it."""

    def __init__(self, parameters, decay=0.9999, min_decay=0.0, update_after_step=0, use_ema_warmup=False, inv_gamma=1.0,
                 power=2 / 3, model_cls=None, model_config=None, **kwargs):
        unknown = sorted(set(kwargs) - {"max_value", "min_value", "foreach", "device"})
        if unknown:
            raise NotImplementedError(f"EMAModel: argument(s) {unknown} are not implemented")
        if isinstance(parameters, torch.nn.Module):
            parameters = parameters.parameters()
            use_ema_warmup = True                 # (diffusers' backwards-compatible behaviour for a module argument)
        if kwargs.get("max_value") is not None:
            decay = kwargs["max_value"]           # deprecated names of decay / min_decay
        if kwargs.get("min_value") is not None:
            min_decay = kwargs["min_value"]
        self.foreach = bool(kwargs.get("foreach", False))      # accepted: the multi-tensor kernel is the same arithmetic
        parameters = list(parameters)
        self._shadow = [p.clone().detach() for p in parameters]
        owner, names = _owner_of(parameters)
        self._names = names                       # state-dict keys of the shadows (save_pretrained), when the parameters came from a model
        self._arena = None                        # FusedAdamW path: shadow in the masters' packed layout (dict, see _fused_step)
        self._stale = False                       # True: the arena is newer than self._shadow
        self._tables = {}
        if kwargs.get("device") is not None:
            self.to(device=kwargs["device"])
        self.collected_params = None
        self.decay = decay
        self.min_decay = min_decay
        self.update_after_step = update_after_step
        self.use_ema_warmup = use_ema_warmup
        self.inv_gamma = inv_gamma
        self.power = power
        self.optimization_step = 0
        self.cur_decay_value = None
        self.model_cls = model_cls
        self.model_config = model_config

    # ---- the shadows in torch layouts (exported from the packed arena on demand)
    @property
    def shadow_params(self):
        self._export()
        return self._shadow

    @shadow_params.setter
    def shadow_params(self, value):
        self._arena = None
        self._stale = False
        self._shadow = value

    def _export(self):
        if not self._stale:
            return
        a = self._arena
        with torch.cuda.device(a["buf"].device):
            a["unet"]._export_arena(a["buf"], self._shadow, a["keys"])
        self._stale = False

    def _drop_arena(self):
        self._export()
        self._arena = None

    # ---- decay schedule
    def get_decay(self, optimization_step):
        """the decay the `optimization_step`-th call of step() uses"""
        step = max(0, optimization_step - self.update_after_step - 1)
        if step <= 0:
            return 0.0
        if self.use_ema_warmup:
            cur_decay_value = 1 - (1 + step / self.inv_gamma) ** -self.power
        else:
            cur_decay_value = (1 + step) / (10 + step)
        cur_decay_value = min(cur_decay_value, self.decay)
        cur_decay_value = max(cur_decay_value, self.min_decay)
        return cur_decay_value

    # ---- the update
    @torch.no_grad()
    def step(self, parameters):
        if isinstance(parameters, torch.nn.Module):
            parameters = parameters.parameters()
        parameters = list(parameters)
        self.optimization_step += 1
        decay = self.get_decay(self.optimization_step)
        self.cur_decay_value = decay
        one_minus_decay = 1 - decay
        if self._fused_step(parameters, one_minus_decay):
            return
        self._drop_arena()
        shadows = self._shadow[:len(parameters)]
        parameters = parameters[:len(shadows)]
        if not shadows:
            return
        if all(s.device.type == "cpu" for s in shadows):
            for s_param, param in zip(shadows, parameters):
                if param.requires_grad:
                    s_param.sub_(one_minus_decay * (s_param - param))
                else:
                    s_param.copy_(param)
            return
        dev = _check_kernel_operands(shadows, parameters, "step")
        owner, _ = _owner_of(parameters, full=False)
        f = owner._fused if owner is not None else None
        if f is not None:
            f.sync_to_model()                     # (FusedAdamW with shadows the arena path does not take - not fp32, a partial list)
        key = ("step",) + tuple((s.data_ptr(), s.dtype, p.data_ptr(), p.numel(), p.dtype, p.requires_grad) for s, p in zip(shadows, parameters))
        t = self._tables.get(key)
        if t is None:
            runs = _element_runs(shadows, parameters, [_EMA if p.requires_grad else _COPY for p in parameters])
            self._tables = {k: v for k, v in self._tables.items() if k[0] != "step"}
            t = self._tables[key] = _DeviceTable(_runs_to_table(runs), dev)
        with torch.cuda.device(dev):
            _cabi.check(_cabi.lib().dmx_ema_step_multi(_cabi.ptr(t.dev), t.nchunks, ctypes.c_float(one_minus_decay), _cabi.current_stream()),
                        "ema_step_multi")

    def _fused_step(self, parameters, one_minus_decay):
        """the parameters of a diffute_amd UNet trained by FusedAdamW: EMA over the fp32 master arena -> False when not applicable"""
        a = self._arena
        if a is not None:
            u = a["unet"]
            f = u._fused
            if f is None or len(parameters) != len(a["ids"]) or any(id(p) != i for p, i in zip(parameters, a["ids"])):
                self._drop_arena()
                a = None
        if a is None:
            u, names = _owner_of(parameters)
            f = u._fused if u is not None else None
            if f is None:
                return False
            if len(self._shadow) != len(parameters) or not all(s.dtype == torch.float32 and s.is_cuda and s.device == f.masters.device
                                                                and s.shape == p.shape for s, p in zip(self._shadow, parameters)):
                return False
            self._import_arena(u, names, parameters)
            a = self._arena
        rg = tuple(p.requires_grad for p in parameters)
        key = (u._h, f.masters.data_ptr(), a["buf"].data_ptr(), rg)
        if a.get("key") != key:
            a["table"] = _DeviceTable(self._arena_table(u, a, f.masters, rg), a["buf"].device)
            a["key"] = key
        t = a["table"]
        with torch.cuda.device(a["buf"].device):
            _cabi.check(u._lib.dmx_ema_step_multi(_cabi.ptr(t.dev), t.nchunks, ctypes.c_float(one_minus_decay), _cabi.current_stream()),
                        "ema_step_multi")
        self._stale = True
        return True

    def _import_arena(self, u, names, parameters):
        with torch.cuda.device(self._shadow[0].device):
            buf = u._import_arena(self._shadow, keys=names)
        self._arena = dict(unet=u, keys=names, ids=[id(p) for p in parameters], buf=buf)
        self._stale = False

    @staticmethod
    def _arena_table(u, a, masters, rg):
        """runs of the packed layout: the merged parameter ranges when all of them train, else per-parameter runs (per row where
        a packed matrix shares its rows with another parameter) with the copy mode for requires_grad=False"""
        lib = u._lib
        b, e = ctypes.c_size_t(), ctypes.c_size_t()
        spans = []
        for k in a["keys"]:
            _cabi.check(lib.dmx_unet_grad_range(u._h, k.encode(), ctypes.byref(b), ctypes.byref(e)), "grad_range")
            spans.append((b.value, e.value))
        base_d, base_s = a["buf"].data_ptr(), masters.data_ptr()
        if all(rg):                               # the union of the parameters' ranges (derived slots of the layout left out)
            merged = []
            for lo, hi in sorted(spans):
                if merged and lo <= merged[-1][1]:
                    merged[-1][1] = max(merged[-1][1], hi)
                else:
                    merged.append([lo, hi])
            return _runs_to_table([(base_d + lo, base_s + lo, (hi - lo) // 4, 0, 0, _EMA, 4, 4) for lo, hi in merged])
        sd = dict(u.named_parameters())
        runs = []
        for k, (lo, hi), train in zip(a["keys"], spans, rg):
            mode = _EMA if train else _COPY
            n, span = sd[k].numel(), (hi - lo) // 4
            if span == n:
                runs.append((base_d + lo, base_s + lo, n, 0, 0, mode, 4, 4))
                continue
            rows = sd[k].shape[0]
            rlen = n // rows
            ld = (span - rlen) // (rows - 1)
            for r in range(rows):
                o = lo + 4 * r * ld
                runs.append((base_d + o, base_s + o, rlen, 0, 0, mode, 4, 4))
        return _runs_to_table(runs)

    # ---- evaluating with the EMA weights
    def _write_params(self, srcs, parameters, what):
        """param.data <- src for every pair; a diffute_amd model then re-packs its weights (and FusedAdamW re-imports its masters)"""
        owner, _ = _owner_of(parameters, full=False)
        f = owner._fused if owner is not None else None
        if f is not None and len(parameters) < len(owner._keys):
            f.sync_to_model()                     # the Parameters not written here must be current before the re-pack below
        cuda = [(s, p) for s, p in zip(srcs, parameters) if p.is_cuda and s.device == p.device]
        other = [(s, p) for s, p in zip(srcs, parameters) if not (p.is_cuda and s.device == p.device)]
        for s, p in other:
            p.data.copy_(s.to(p.device).data)
        if cuda:
            ss, ps = [c[0] for c in cuda], [c[1].data for c in cuda]
            dev = _check_kernel_operands(ps, ss, what)
            key = ("copy",) + tuple((s.data_ptr(), s.dtype, p.data_ptr(), p.numel(), p.dtype) for s, p in zip(ss, ps))
            t = self._tables.get(key)
            if t is None:
                if len(self._tables) > 8:
                    self._tables = {}
                t = self._tables[key] = _DeviceTable(_runs_to_table(_element_runs(ps, ss, [_COPY] * len(ps))), dev)
            with torch.cuda.device(dev):
                _cabi.check(_cabi.lib().dmx_copy_multi(_cabi.ptr(t.dev), t.nchunks, _cabi.current_stream()), "copy_multi")
        if owner is not None:
            if f is not None:
                f.dirty = False                   # the Parameters are the current weights now; the masters follow below
            owner.mark_parameters_changed()
            owner._weights_changed()
            if owner.device.type == "cuda":
                owner._ensure_packed()

    def copy_to(self, parameters):
        """the model's parameters <- the EMA weights"""
        parameters = list(parameters)
        n = min(len(parameters), len(self._shadow))
        self._write_params(self.shadow_params[:n], parameters[:n], "copy_to")

    def store(self, parameters):
        """save the current parameters (restore() brings them back after evaluating with copy_to())"""
        parameters = list(parameters)
        owner, _ = _owner_of(parameters, full=False)
        f = owner._fused if owner is not None else None
        if f is not None:
            f.sync_to_model()                     # a FusedAdamW-trained model's current weights are its masters
        self.collected_params = [param.detach().clone() for param in parameters]

    def restore(self, parameters):
        if self.collected_params is None:
            raise RuntimeError("This ExponentialMovingAverage has no `store()`ed weights to `restore()`")
        parameters = list(parameters)
        n = min(len(parameters), len(self.collected_params))
        self._write_params(self.collected_params[:n], parameters[:n], "restore")
        self.collected_params = None

    def to(self, device=None, dtype=None):
        """move the shadows to `device`; cast the floating-point ones to `dtype`"""
        self._drop_arena()
        self._shadow = [p.to(device=device, dtype=dtype) if p.is_floating_point() else p.to(device=device) for p in self._shadow]
        self._tables = {}

    # ---- checkpointing (accelerator save / load hooks, train_diffute_v1.py:664-678)
    def state_dict(self):
        return {
            "decay": self.decay,
            "min_decay": self.min_decay,
            "optimization_step": self.optimization_step,
            "update_after_step": self.update_after_step,
            "use_ema_warmup": self.use_ema_warmup,
            "inv_gamma": self.inv_gamma,
            "power": self.power,
            "shadow_params": self.shadow_params,
        }

    def load_state_dict(self, state_dict):
        state_dict = copy.deepcopy(state_dict)
        self.decay = state_dict.get("decay", self.decay)
        if self.decay < 0.0 or self.decay > 1.0:
            raise ValueError("Decay must be between 0 and 1")
        self.min_decay = state_dict.get("min_decay", self.min_decay)
        if not isinstance(self.min_decay, float):
            raise ValueError("Invalid min_decay")
        self.optimization_step = state_dict.get("optimization_step", self.optimization_step)
        if not isinstance(self.optimization_step, int):
            raise ValueError("Invalid optimization_step")
        self.update_after_step = state_dict.get("update_after_step", self.update_after_step)
        if not isinstance(self.update_after_step, int):
            raise ValueError("Invalid update_after_step")
        self.use_ema_warmup = state_dict.get("use_ema_warmup", self.use_ema_warmup)
        if not isinstance(self.use_ema_warmup, bool):
            raise ValueError("Invalid use_ema_warmup")
        self.inv_gamma = state_dict.get("inv_gamma", self.inv_gamma)
        if not isinstance(self.inv_gamma, (float, int)):
            raise ValueError("Invalid inv_gamma")
        self.power = state_dict.get("power", self.power)
        if not isinstance(self.power, (float, int)):
            raise ValueError("Invalid power")
        shadow_params = state_dict.get("shadow_params", None)
        if shadow_params is not None:
            if not isinstance(shadow_params, list):
                raise ValueError("shadow_params must be a list")
            if not all(isinstance(p, torch.Tensor) for p in shadow_params):
                raise ValueError("shadow_params must all be Tensors")
            self.shadow_params = shadow_params
            self._tables = {}

    def save_pretrained(self, path):
        """`ema_unet.save_pretrained(out/"unet_ema")`: config.json (the model config + the EMA hyper-parameters) and
        diffusion_pytorch_model.safetensors with the shadows under the model's state-dict keys - the directory both
        `UNet2DConditionModel.from_pretrained` and `EMAModel.from_pretrained` read"""
        if self.model_cls is None:
            raise ValueError("`save_pretrained` can only be used if `model_cls` was defined at __init__.")
        if self.model_config is None:
            raise ValueError("`save_pretrained` can only be used if `model_config` was defined at __init__.")
        from safetensors.torch import save_file
        names = self._names
        if names is None:                         # parameters that did not come from a live model: the model class names them
            names = [k for k, _ in self.model_cls.from_config(self.model_config).named_parameters()]
        shadows = self.shadow_params
        if len(names) != len(shadows):
            raise ValueError(f"EMAModel.save_pretrained: {len(shadows)} shadow parameters, the model has {len(names)}")
        cfg = self.model_config.to_dict() if hasattr(self.model_config, "to_dict") else dict(self.model_config)
        cfg = {k: (list(v) if isinstance(v, tuple) else v) for k, v in cfg.items()}
        ema = self.state_dict()
        ema.pop("shadow_params")
        cfg.update(ema)
        cfg["_class_name"] = self.model_cls.__name__
        os.makedirs(path, exist_ok=True)
        with open(os.path.join(path, "config.json"), "w") as f:
            json.dump(cfg, f, indent=2)
        save_file({k: s.detach().cpu().contiguous() for k, s in zip(names, shadows)}, os.path.join(path, "diffusion_pytorch_model.safetensors"))

    @classmethod
    def from_pretrained(cls, path, model_cls):
        _, ema_kwargs = model_cls.load_config(path, return_unused_kwargs=True)
        model = model_cls.from_pretrained(path)
        ema_model = cls(model.parameters(), model_cls=model_cls, model_config=model.config)
        ema_model.load_state_dict(ema_kwargs)
        return ema_model
