"""Low-rank adapters (LoRA) on the UNet's attention-block linears, in diffusers' / peft's call shapes: `unet.add_adapter(LoraConfig(...))`,
`set_adapters`, `disable_adapters`, `delete_adapter`, `lora_parameters`, `save_lora_weights` / `load_lora_weights`, `fuse_lora`.

The adapters are MERGED: the packed weights arena holds W' = W0 + sum_j s_j B_j A_j (s_j = weight_j * alpha_j / r_j) for every target, written
by dmx_unet_lora_apply (csrc/lora.hip) through the pack path of the ordinary weights, so no forward or backward kernel knows about LoRA.
The base Parameters are never written (only `fuse_lora` does).  Training: the unchanged HIP backward leaves every dW in the gradient arena;
dmx_lora_grads forms dA_j = s_j B_j^T dW and dB_j = s_j dW A_j^T from the targets' dW, exported to torch layout by the existing export
kernel, and autograd fills `.grad` of the LoRA Parameters.  The forward runs W' rounded to the compute type: a delta below one 16-bit ulp of
W0 is invisible to the forward until it grows (as a full fine-tune with fp32 masters behaves here).  One set of adapters per model handle.
"""
import ctypes
import math
import os
from collections import OrderedDict

import torch
from torch import nn

from . import _cabi

LORA_TARGETS = ("to_q", "to_k", "to_v", "to_out.0", "proj_in", "proj_out", "ff.net.0.proj", "ff.net.2")
DEFAULT_TARGETS = ("to_q", "to_k", "to_v", "to_out.0")
LORA_WEIGHT_NAME = "pytorch_lora_weights.safetensors"
_PREFIXES = ("unet.", "base_model.model.", "")


class LoraConfig:
    """The fields of peft.LoraConfig this library reads (a peft.LoraConfig is accepted in its place)."""

    def __init__(self, r=16, lora_alpha=16, target_modules=DEFAULT_TARGETS, init_lora_weights=True):
        self.r, self.lora_alpha, self.target_modules, self.init_lora_weights = r, lora_alpha, target_modules, init_lora_weights


def merge_scale(weight, alpha, r):
    """s = weight * alpha / r, rounded once to fp32 (what the kernels multiply by)"""
    return float(torch.tensor(float(weight) * float(alpha) / int(r), dtype=torch.float32))


def target_keys(keys_shapes, target_modules):
    """the parameter names `<module>.weight` the suffixes `target_modules` select among `keys_shapes` ({name: shape}), in the model's order.
    Targets are the 2-D linear weights inside `attentions.*`; any other suffix raises ValueError."""
    if isinstance(target_modules, str):
        target_modules = (target_modules,)
    tm = tuple(target_modules)
    if not tm:
        raise ValueError("LoRA: empty target_modules")
    for t in tm:
        if t not in LORA_TARGETS:
            raise ValueError(f"LoRA: target module {t!r} is not supported (only the linears {LORA_TARGETS} inside the attention blocks; "
                             "convolutions, norms and embeddings cannot carry an adapter here)")
    out = []
    for k, shp in keys_shapes.items():
        if not k.endswith(".weight") or ".attentions." not in k or len(shp) != 2:
            continue
        mod = k[:-len(".weight")]
        if any(mod.endswith("." + t) for t in tm):
            out.append(k)
    if not out:
        raise ValueError(f"LoRA: target_modules {tm} match no linear of this model")
    return out


def lora_file_keys(module):
    """the three keys one module is written under"""
    return f"unet.{module}.lora_A.weight", f"unet.{module}.lora_B.weight", f"unet.{module}.alpha"


def parse_lora_state_dict(sd, module_shapes, metadata=None):
    """a LoRA state dict in any accepted spelling -> OrderedDict module -> (A [r,K], B [N,r], alpha), checked against
    `module_shapes` ({module path: (N, K)} of the linears that may carry an adapter).  Accepted: the prefixes `unet.`, `base_model.model.`
    and none; `<module>.lora_A.weight` / `.lora_B.weight` (also peft's `.lora_A.<adapter>.weight`) and diffusers' older
    `<module>_lora.down.weight` / `.up.weight` (with or without `.processor`, `to_out_lora` for `to_out.0`); alpha from `<module>.alpha`,
    else from `lora_alpha` in `metadata`, else r.  Unknown modules, shape and rank mismatches raise ValueError naming the key."""
    found = OrderedDict()
    for key, v in sd.items():
        rest = key
        for pre in _PREFIXES:
            if pre and rest.startswith(pre):
                rest = rest[len(pre):]
                break
        if rest.endswith(".alpha"):
            mod, what = rest[:-len(".alpha")], "alpha"
        elif rest.endswith(".weight") and ".lora_A." in rest + ".":
            mod, what = rest.split(".lora_A")[0], "A"
        elif rest.endswith(".weight") and ".lora_B." in rest + ".":
            mod, what = rest.split(".lora_B")[0], "B"
        elif rest.endswith("_lora.down.weight") or rest.endswith("_lora.up.weight"):
            mod = rest.rsplit("_lora.", 1)[0].replace(".processor.", ".")
            if mod.endswith(".to_out"):
                mod += ".0"
            what = "A" if rest.endswith(".down.weight") else "B"
        else:
            raise ValueError(f"LoRA: key {key!r} is not a LoRA tensor name")
        if mod.endswith("_lora"):                    # (`<module>_lora.alpha` of the older spelling)
            mod = mod[:-len("_lora")].replace(".processor.", ".")
            if mod.endswith(".to_out"):
                mod += ".0"
        if mod not in module_shapes:
            raise ValueError(f"LoRA: key {key!r} names module {mod!r}, which is not a linear of this model that can carry an adapter")
        found.setdefault(mod, {})[what] = (key, v)
    meta_alpha = None
    if metadata and metadata.get("lora_alpha") is not None:
        meta_alpha = float(metadata["lora_alpha"])
    out = OrderedDict()
    for mod, parts in found.items():
        if "A" not in parts or "B" not in parts:
            have = parts.get("A") or parts.get("B") or parts.get("alpha")
            raise ValueError(f"LoRA: module {mod!r} has {have[0]!r} but not both lora_A and lora_B")
        (ka, A), (kb, B) = parts["A"], parts["B"]
        N, K = module_shapes[mod]
        if A.ndim != 2 or A.shape[1] != K:
            raise ValueError(f"LoRA: key {ka!r} has shape {tuple(A.shape)}, expected [r, {K}]")
        if B.ndim != 2 or B.shape[0] != N:
            raise ValueError(f"LoRA: key {kb!r} has shape {tuple(B.shape)}, expected [{N}, r]")
        if A.shape[0] != B.shape[1] or A.shape[0] < 1:
            raise ValueError(f"LoRA: key {kb!r} has rank {B.shape[1]} but {ka!r} has rank {A.shape[0]}")
        alpha = float(parts["alpha"][1]) if "alpha" in parts else (meta_alpha if meta_alpha is not None else float(A.shape[0]))
        out[mod] = (A, B, alpha)
    return out


class _Adapter(nn.Module):
    """one named adapter: per target key the Parameters A [r,K], B [N,r] (registered as t<i>_A / t<i>_B) and its alpha"""

    def __init__(self):
        super().__init__()
        self.layers = OrderedDict()     # parameter key of the target -> (A, B, alpha)

    def add_layer(self, key, A, B, alpha):
        i = len(self.layers)
        pa, pb = nn.Parameter(A, requires_grad=True), nn.Parameter(B, requires_grad=True)
        self.register_parameter(f"t{i}_A", pa)
        self.register_parameter(f"t{i}_B", pb)
        self.layers[key] = (pa, pb, float(alpha))

    def items(self):
        """(key, A, B, alpha) with the Parameters as they are registered now (`.to()` may have replaced their storage, not the objects)"""
        return [(k, a, b, al) for k, (a, b, al) in self.layers.items()]


class LoraMixin:
    """LoRA state and interface of UNet2DConditionModel (models.py calls _lora_init, _lora_sync_arena, _lora_train_params, _lora_train_backward)."""

    def _lora_init(self):
        self._lora = OrderedDict()      # adapter name -> _Adapter
        self._lora_active = []          # [(name, weight)] in the order their contributions are summed
        self._lora_disabled = False
        self._lora_ever = False         # an adapter was added at some time: _ensure_packed looks at the LoRA signature
        self._lora_sig = None           # LoRA signature the arena was last brought to
        self._lora_applied = []         # target keys whose arena contents are merged values
        self._lora_staging = {}         # target key -> the fp32 merged weight the arena was packed from
        self._lora_dw = {}              # target key -> dW in torch layout (training)
        self._lora_ids = frozenset()    # ids of the LoRA Parameters: not part of the base signature
        self._lora_keep = None          # what the last launches read (tables, temporaries)
        self._lora_keep_grads = None

    # ---- adapters
    def _lora_module_shapes(self):
        shapes = {k: tuple(p.shape) for k, p in zip(self._keys, self._param_list())}
        return OrderedDict((k[:-len(".weight")], shapes[k]) for k in target_keys(shapes, LORA_TARGETS))

    def _lora_register(self, name, adapter):
        if "lora_adapters" not in self._modules:
            self.add_module("lora_adapters", nn.Module())
        self._modules["lora_adapters"].add_module(name, adapter)
        self._lora[name] = adapter
        self._lora_ever = True
        self._lora_refresh_ids()
        for p in self._param_list():                   # the base is frozen, as peft does it
            p.requires_grad_(False)

    def _lora_refresh_ids(self):
        self._lora_ids = frozenset(id(p) for ad in self._lora.values() for _, a, b, _ in ad.items() for p in (a, b))
        self.__dict__.pop("_ema_param_ids", None)

    def add_adapter(self, adapter_config, adapter_name="default"):
        """`unet.add_adapter(LoraConfig(r=16, lora_alpha=16, target_modules=(...)), adapter_name="default")`: A is initialised as peft does it
        (kaiming-uniform, a = sqrt(5)), B is zero; the adapter becomes the active one and the base Parameters are frozen."""
        if adapter_name in self._lora:
            raise ValueError(f"add_adapter: an adapter named {adapter_name!r} exists")
        if not str(adapter_name).isidentifier():
            raise ValueError(f"add_adapter: adapter name {adapter_name!r} must be an identifier")
        r, alpha = int(adapter_config.r), float(adapter_config.lora_alpha)
        if r < 1:
            raise ValueError(f"add_adapter: r = {r}")
        tm = adapter_config.target_modules
        base = dict(zip(self._keys, self._param_list()))
        keys = target_keys({k: tuple(p.shape) for k, p in base.items()}, DEFAULT_TARGETS if tm is None else tm)
        ad = _Adapter()
        dev = self.device
        for k in keys:
            N, K = base[k].shape
            A = torch.empty(r, K, dtype=torch.float32)
            nn.init.kaiming_uniform_(A, a=math.sqrt(5))
            B = torch.zeros(N, r, dtype=torch.float32)
            if not getattr(adapter_config, "init_lora_weights", True):
                nn.init.kaiming_uniform_(B, a=math.sqrt(5))
            ad.add_layer(k, A.to(dev), B.to(dev), alpha)
        self._lora_register(adapter_name, ad)
        self.set_adapters(adapter_name)

    def set_adapters(self, adapter_names, weights=None):
        """make these adapters (a name or a list) the active ones, summed in the order given with `weights` (default 1.0 each)"""
        names = [adapter_names] if isinstance(adapter_names, str) else list(adapter_names)
        if weights is None:
            weights = [1.0] * len(names)
        elif not isinstance(weights, (list, tuple)):
            weights = [weights] * len(names)
        if len(weights) != len(names) or len(set(names)) != len(names):
            raise ValueError(f"set_adapters: {len(names)} names (each once) need as many weights, got {len(weights)}")
        for n in names:
            if n not in self._lora:
                raise ValueError(f"set_adapters: no adapter named {n!r} (have {list(self._lora)})")
        self._lora_active = [(n, 1.0 if w is None else float(w)) for n, w in zip(names, weights)]
        self._lora_disabled = False

    def disable_adapters(self):
        """run the base model; `enable_adapters()` / `set_adapters(...)` bring the adapters back"""
        self._lora_disabled = True

    def enable_adapters(self):
        self._lora_disabled = False

    def delete_adapter(self, adapter_name):
        if adapter_name not in self._lora:
            raise ValueError(f"delete_adapter: no adapter named {adapter_name!r}")
        del self._lora[adapter_name]
        del self._modules["lora_adapters"]._modules[adapter_name]
        self._lora_active = [(n, w) for n, w in self._lora_active if n != adapter_name]
        self._lora_refresh_ids()

    @property
    def active_adapters(self):
        return [] if self._lora_disabled else [n for n, _ in self._lora_active]

    def _lora_effective(self):
        return [] if self._lora_disabled else [(self._lora[n], w) for n, w in self._lora_active]

    def lora_parameters(self, adapter_name=None):
        """the nn.Parameters (A, B per target) of one adapter, or of all of them"""
        names = list(self._lora) if adapter_name is None else [adapter_name]
        for n in names:
            if n not in self._lora:
                raise ValueError(f"lora_parameters: no adapter named {n!r}")
        return [p for n in names for _, a, b, _ in self._lora[n].items() for p in (a, b)]

    # ---- files
    def lora_state_dict(self, adapter_name="default"):
        if adapter_name not in self._lora:
            raise ValueError(f"lora_state_dict: no adapter named {adapter_name!r}")
        sd = OrderedDict()
        for k, a, b, alpha in self._lora[adapter_name].items():
            ka, kb, kal = lora_file_keys(k[:-len(".weight")])
            sd[ka], sd[kb], sd[kal] = a.detach(), b.detach(), torch.tensor(alpha, dtype=torch.float32)
        return sd

    def save_lora_weights(self, path, adapter_name="default"):
        """one safetensors file: `path` itself when it ends in .safetensors, else `path/pytorch_lora_weights.safetensors`"""
        from safetensors.torch import save_file
        sd = self.lora_state_dict(adapter_name)
        if not str(path).endswith(".safetensors"):
            os.makedirs(path, exist_ok=True)
            path = os.path.join(path, LORA_WEIGHT_NAME)
        alphas = sorted({al for _, _, _, al in self._lora[adapter_name].items()})
        meta = {"format": "pt"}
        if len(alphas) == 1:
            meta["lora_alpha"] = repr(alphas[0])
        save_file({k: v.cpu().contiguous() for k, v in sd.items()}, path, metadata=meta)
        return path

    def load_lora_weights(self, path_or_state_dict, adapter_name="default"):
        """a file / directory written by save_lora_weights (or peft / diffusers with the accepted key spellings), or such a state dict, as
        adapter `adapter_name` (new, or an existing one with the same targets and ranks); the adapter becomes the active one"""
        meta = None
        if isinstance(path_or_state_dict, dict):
            sd = path_or_state_dict
        else:
            from safetensors import safe_open
            path = path_or_state_dict
            if os.path.isdir(path):
                path = os.path.join(path, LORA_WEIGHT_NAME)
            sd = OrderedDict()
            with safe_open(path, framework="pt", device="cpu") as f:
                meta = f.metadata()
                for k in f.keys():
                    sd[k] = f.get_tensor(k)
        layers = parse_lora_state_dict(sd, self._lora_module_shapes(), meta)
        if not layers:
            raise ValueError("load_lora_weights: no LoRA tensors")
        dev = self.device
        order = {k: i for i, k in enumerate(self._keys)}
        mods = sorted(layers, key=lambda m: order[m + ".weight"])
        if adapter_name in self._lora:
            ad = self._lora[adapter_name]
            if set(ad.layers) != {m + ".weight" for m in mods}:
                raise ValueError(f"load_lora_weights: adapter {adapter_name!r} exists with other target modules")
            with torch.no_grad():
                for m in mods:
                    A, B, alpha = layers[m]
                    a, b, _ = ad.layers[m + ".weight"]
                    if a.shape != A.shape or b.shape != B.shape:
                        raise ValueError(f"load_lora_weights: module {m!r}: rank {A.shape[0]} but adapter {adapter_name!r} has rank {a.shape[0]}")
                    a.copy_(A); b.copy_(B)
                    ad.layers[m + ".weight"] = (a, b, float(alpha))
        else:
            if not str(adapter_name).isidentifier():
                raise ValueError(f"load_lora_weights: adapter name {adapter_name!r} must be an identifier")
            ad = _Adapter()
            for m in mods:
                A, B, alpha = layers[m]
                ad.add_layer(m + ".weight", A.detach().to(device=dev, dtype=torch.float32).contiguous().clone(),
                             B.detach().to(device=dev, dtype=torch.float32).contiguous().clone(), alpha)
            self._lora_register(adapter_name, ad)
        self.set_adapters(adapter_name)

    def merged_lora_weights(self):
        """{parameter name: the fp32 merged weight W0 + sum_j s_j B_j A_j the arena was packed from} for the targets of the active adapters.
        The tensors are the staging buffers themselves: valid until the adapters or the base weights change."""
        self._ensure_packed()
        return OrderedDict((k, self._lora_staging[k]) for k in self._lora_applied)

    def fuse_lora(self):
        """write the merged values into the base Parameters and drop every adapter"""
        merged = self.merged_lora_weights()
        base = dict(zip(self._keys, self._param_list()))
        with torch.no_grad():
            for k, w in merged.items():
                base[k].copy_(w)
        for n in list(self._lora):
            self.delete_adapter(n)

    # ---- the arena follows the adapters
    def _lora_signature(self):
        sig = [self._lora_disabled]
        for n, w in self._lora_active:
            sig.append((n, w))
            for k, a, b, alpha in self._lora[n].items():
                sig.append((a.data_ptr(), a._version, b.data_ptr(), b._version, alpha))
        return tuple(sig)

    def _lora_records(self, keys, per_key, src, dst, dst2=None):
        """the dmx_lora_rec array of `keys`: per_key[k] = [(A, B, s)]; src[k] = W of the record, dst[k] (merge) or dst[(k, j)] / dst2[(k, j)] (grads)"""
        n = sum(len(per_key.get(k, ())) for k in keys)
        recs = (_cabi.LoraRec * max(n, 1))()
        i = 0
        for k in keys:
            lst = per_key.get(k, ())
            for j, (A, B, s) in enumerate(lst):
                for t in (A, B):
                    if t.dtype != torch.float32 or not t.is_contiguous() or not t.is_cuda:
                        raise RuntimeError("LoRA: the adapter Parameters must be fp32, contiguous and on the GPU")
                q = recs[i]
                q.A, q.B, q.W = A.data_ptr(), B.data_ptr(), src[k].data_ptr()
                q.N, q.K, q.r, q.s = B.shape[0], A.shape[1], A.shape[0], s
                if dst2 is None:
                    q.dst, q.count = dst[k].data_ptr(), (len(lst) if j == 0 else 0)
                else:
                    q.dst, q.dst2, q.count = dst[(k, j)].data_ptr(), dst2[(k, j)].data_ptr(), 0
                i += 1
        return recs, n

    def _lora_per_key(self, pairs):
        per_key = OrderedDict()
        for ad, w in pairs:
            for k, a, b, alpha in ad.items():
                per_key.setdefault(k, []).append((a, b, merge_scale(w, alpha, a.shape[0])))
        return per_key

    def _lora_base_f32(self, keys, keep):
        base = dict(zip(self._keys, self._param_list()))
        out = {}
        for k in keys:
            w = base[k].detach()
            if w.dtype != torch.float32 or not w.is_contiguous():
                w = w.to(torch.float32).contiguous()
                keep.append(w)
            out[k] = w
        return out

    def _lora_sync_arena(self, repacked):
        """bring the arena to the current adapters: `repacked` says the arena was just packed from the base Parameters.  -> True when the arena changed"""
        sig = self._lora_signature()
        if repacked:
            self._lora_applied = []
        elif sig == self._lora_sig:
            return False
        per_key = self._lora_per_key(self._lora_effective())
        prev = set(self._lora_applied)
        keys = [k for k in self._keys if k in per_key or k in prev]
        self._lora_sig = sig
        if not keys:
            return False
        keep = []
        dev = self.device
        w0 = self._lora_base_f32(keys, keep)
        for k in keys:
            if k in per_key and (k not in self._lora_staging or self._lora_staging[k].device != dev):
                self._lora_staging[k] = torch.empty(w0[k].shape, dtype=torch.float32, device=dev)
        recs, n = self._lora_records(keys, per_key, w0, self._lora_staging)
        targets = (_cabi.LoraTarget * len(keys))()
        i = 0
        for t, k in zip(targets, keys):
            t.name, t.w0, t.rec0, t.nrec = k.encode(), w0[k].data_ptr(), i, len(per_key.get(k, ()))
            i += t.nrec
        table = torch.empty(max(n, 1) * ctypes.sizeof(_cabi.LoraRec), dtype=torch.uint8, device=dev)
        _cabi.check(self._lib.dmx_unet_lora_apply(self._h, targets, len(keys), recs, n, _cabi.ptr(table), table.numel(), _cabi.current_stream()),
                    "unet_lora_apply")
        self._lora_keep = (table, keep)
        self._lora_applied = [k for k in keys if k in per_key]
        for k in list(self._lora_staging):
            if k not in per_key:
                del self._lora_staging[k]
        return True

    # ---- training
    def _lora_train_params(self):
        """the Parameters the training function takes as inputs: A, B per target of every active adapter"""
        return [p for ad, _ in self._lora_effective() for _, a, b, _ in ad.items() for p in (a, b)]

    def _lora_grads(self, grads_arena):
        """dA / dB of every active adapter from the gradient arena -> (flat fp32 tensor, its views in _lora_train_params order)"""
        pairs = self._lora_effective()
        per_key = self._lora_per_key(pairs)
        keys = [k for k in self._keys if k in per_key]
        dev = self.device
        for k in keys:
            if k not in self._lora_dw or self._lora_dw[k].device != dev:
                self._lora_dw[k] = torch.empty(per_key[k][0][1].shape[0], per_key[k][0][0].shape[1], dtype=torch.float32, device=dev)
        self._export_arena(grads_arena, [self._lora_dw[k] for k in keys], keys)
        total = sum(a.numel() + b.numel() for lst in per_key.values() for a, b, _ in lst)
        flat = torch.empty(total, dtype=torch.float32, device=dev)
        dA, dB, off = {}, {}, 0
        by_param = {}
        for k in keys:
            for j, (a, b, _) in enumerate(per_key[k]):
                dA[(k, j)] = flat[off:off + a.numel()].view(a.shape); off += a.numel()
                dB[(k, j)] = flat[off:off + b.numel()].view(b.shape); off += b.numel()
                by_param[id(a)], by_param[id(b)] = dA[(k, j)], dB[(k, j)]
        recs, n = self._lora_records(keys, per_key, self._lora_dw, dA, dB)
        table = torch.empty(max(n, 1) * ctypes.sizeof(_cabi.LoraRec), dtype=torch.uint8, device=dev)
        _cabi.check(self._lib.dmx_lora_grads(recs, n, _cabi.ptr(table), table.numel(), _cabi.current_stream()), "lora_grads")
        self._lora_keep_grads = table
        return flat, [by_param[id(p)] for p in self._lora_train_params()]

    def _lora_train_backward(self, dpred):
        """the unchanged HIP backward into the gradient arena, then dmx_lora_grads: -> the gradients of _lora_train_params.  With
        set_gradient_sync the flat dA / dB tensor is exchanged with ONE all-reduce (exact: dA and dB are linear in dW, A and B are equal on
        every rank); inside a no_sync / accumulate_steps window dA / dB are summed locally and `.grad` is left alone until the boundary."""
        lib, tb, sync = self._lib, self._tb, self._sync
        if self._fused is not None:
            raise RuntimeError("FusedAdamW owns every weight of the model; train adapters with a torch optimizer over unet.lora_parameters()")
        if sync is not None:
            dpred = dpred / sync["world"]
        dpred = dpred.to(torch.float32).contiguous()
        with torch.cuda.stream(tb["fwd_stream"]):
            _cabi.check(lib.dmx_unet_train_backward(self._h, _cabi.ptr(tb["grads"]), _cabi.ptr(dpred), None, 0, _cabi.current_stream()),
                        "unet_train_backward")
            flat, views = self._lora_grads(tb["grads"])
        torch.cuda.current_stream(dpred.device).wait_stream(tb["fwd_stream"])
        if sync is not None:
            acc = sync["acc"]
            if not acc.boundary():
                acc.stash(flat)
                return [None] * len(views)
            if acc.acc_n:
                flat.add_(acc.acc)
            sync["dist"].all_reduce(flat, group=sync["group"])
            acc.exchanged()
        return views
