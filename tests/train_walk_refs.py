"""Per-parameter references, rounding-point restatements, cases and bounds for the training WALKS (unet_train.hip,
vae_train.hip, train_common.h): the code that wires the backward kernels into a gradient - which consumer's gradient joins
through which `res` input, how the skip gradients find their tensors, how the concat halves split, where the 22 `dtproj`
slices land, what happens to padded context rows, how H and W travel.  The kernels themselves are held per slice by
train_refs.py; here one whole training step is held per PARAMETER.

Shared by test_train_walk_gpu.py (HIP step vs the reference) and test_train_walk_host.py (restatement vs the reference, on
the CPU).  For a case and an element ("bf16" / "fp16"):
  reference    torch autograd over the fp32 oracle (oracle.pipeline.*_train_grads, emulate_bf16=False);
  restatement  the same graph with every 16-bit materialisation point of the HIP path as a cast (emulate_bf16=elem,
               train_points=True), in float64 arithmetic between the roundings so that the figures do not depend on the
               host's float32 summation order (in float32 they move by 5 - 20 % with the thread count: a 1e-7 difference
               flips a 16-bit rounding).  Autograd differentiates the cast, so the gradient is rounded at the same points on the way
               back.  The loss is multiplied by the loss scale before backward() and the gradients divided by it afterwards
               (LOSS_SCALE: 1024 for fp16 as under GradScaler(init_scale=1024), 1 for bf16).  The restatement has the rounding
               points; it does not have the MFMA accumulation order or the 16-bit P / dS inside the attention backward, and it
               rounds the weight gradients once more than the HIP path does (the weight cast's own backward: 2^-9 / 2^-12
               relative, far below the floors).
  figures      err_k = ||g_k - r_k|| / ||r_k|| per parameter, and the whole-gradient figure sqrt(sum ||g_k - r_k||^2 /
               sum ||r_k||^2); FLOORS (train_walk_floors.py) records the restatement's: "<model>/<case>/<elem>" ->
               (whole, median parameter, {parameter: floor} where the floor exceeds the median).
  bounds       per parameter FACTOR_PARAM (3, as train_refs.py for slices) x max(floor_k, median floor); whole gradient
               FACTOR_WHOLE (1.5) x the whole-gradient floor (an average over ~1e6 elements; the one HIP point known sits at
               1.03 - 1.06 x); loss within LOSS_TOL (2 %) of the fp32 oracle's.
  judged absolutely (absolute_set): an attention's to_q / to_k parameter whose reference gradient is below ABS_COND x the
               norm of the same attention's to_v gradient (weight for a weight, bias for a bias) is zero in exact arithmetic -
               the softmax is invariant under a per-row shift (VAE to_k.bias), or runs over one key (the 1x1 level of
               min8_b1: attn1.to_q / to_k) - and its reference is rounding noise.  For these: ||g_k|| <= ABS_TOL x
               ||g_to_v||.  That is a check that the gradient is essentially zero, not a noise bound.  No other parameter
               leaves the relative check.
Faults (unet_eval(fault=...)) rewire one edge of the oracle's graph through its `tap` hook - the kind of wiring mistake the
GPU test exists for.  Regenerate the table with `python tests/train_walk_refs.py > tests/train_walk_floors.py`."""
import os
import statistics
import sys

import torch

if __name__ == "__main__":                               # run as a script: the repository root is not on the path yet
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from oracle import pipeline as OP, unet as OU, vae as OV

ELEMS = {"bf16": torch.bfloat16, "fp16": torch.float16}
LOSS_SCALE = {"bf16": 1.0, "fp16": 1024.0}
FACTOR_PARAM, FACTOR_WHOLE, LOSS_TOL = 3.0, 1.5, 2e-2
ABS_COND, ABS_TOL = 1e-4, 1e-2
OLD_BARS = (4e-2, 1e-1)                     # test_models_gpu.py's UNet training bars: whole gradient, worst parameter

# the smallest inputs at which each route of the walk exists
UNET_CASES = {
    "sq16_b2": dict(B=2, H=16, W=16, ctx=77, shared_t=False, ctx16=False),          # the case of test_models_gpu.py, now per parameter
    "wide_b3": dict(B=3, H=8, W=24, ctx=130, shared_t=False, ctx16=False),          # non-square, odd batch, two tiles of context padding
    "tall_b2_shared_t": dict(B=2, H=24, W=8, ctx=77, shared_t=True, ctx16=False),   # the other orientation, t_count == 1
    "min8_b1": dict(B=1, H=8, W=8, ctx=64, shared_t=True, ctx16=True),              # 1x1 deepest level, no padding rows, 16-bit context
}
# (never below a 4-pixel latent edge: at a 2x2 latent the bf16 restatement itself is 2e-1 off - ill-conditioned, a bound from it checks
# nothing.)  AutoencoderKL training takes image sides that are multiples of 64 only (AutoencoderKL.forward and
# dmx_vae_train_forward both refuse anything else; the mid attention keeps P as an [S][S] GEMM operand, S = HW/64): wide_b3 is the smallest non-square odd-batch input of the reference graph and is
# held on the host only - on the GPU the product must refuse it - and wide128_b3 is the smallest one the training graph admits.
VAE_CASES = {
    "sq64_b2": dict(B=2, H=64, W=64, admitted=True),
    "wide_b3": dict(B=3, H=32, W=48, admitted=False),
    "wide128_b3": dict(B=3, H=64, W=128, admitted=True),
}
TIMESTEPS = (981, 17, 500)
ALL_KEYS = [("unet", c) for c in UNET_CASES] + [("vae", c) for c in VAE_CASES]
GPU_KEYS = [(m, c) for m, c in ALL_KEYS if m == "unet" or VAE_CASES[c]["admitted"]]


# ---------------------------------------------------------------------------------------------- inputs and parameters
def host_params(model):
    """the seeded parameters the product classes start from (their default seeds: UNet 1234, AutoencoderKL 4321), so that the
    floors are measured on the gradient the GPU test sees"""
    if model == "unet":
        return OU.make_params(OU.unet_param_spec(OU.TINY_UNET), seed=1234)
    return OU.make_params(OV.vae_param_spec(OV.TINY_VAE), seed=4321)


def unet_inputs(case):
    """(x [B,9,H,W], t [B] or [1], ctx [B,S,128] fp32, target [B,4,H,W]) on the CPU.  A 16-bit context (ctx16) is this
    fp32 tensor cast to the build's element by the caller: the oracle rounds it to the same values."""
    from diffute_amd.synthetic import synth_inputs
    c = UNET_CASES[case]
    lat, mask, mlat, ctx = synth_inputs(c["B"], c["H"], c["W"], c["ctx"], OU.TINY_UNET["cross_attention_dim"])
    t = torch.tensor(TIMESTEPS[:1] if c["shared_t"] else TIMESTEPS[:c["B"]])
    target = torch.randn(c["B"], 4, c["H"], c["W"], generator=torch.Generator().manual_seed(11))
    return torch.cat([lat, mask, mlat], 1), t, ctx, target


def vae_inputs(case):
    c = VAE_CASES[case]
    g = torch.Generator().manual_seed(21)
    x = torch.rand(c["B"], 3, c["H"], c["W"], generator=g) * 2 - 1
    tgt = torch.rand(c["B"], 3, c["H"], c["W"], generator=g) * 2 - 1
    return x, tgt


# ---------------------------------------------------------------------------------------------- faults (oracle graph)
class _ScaleGrad(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, s):
        ctx.s = s
        return x.view_as(x)

    @staticmethod
    def backward(ctx, g):
        return g * ctx.s, None


UP_SKIP_RESNET = "up_blocks.2.resnets.0."                # concatenated input (256 from below | 128 skip), has a shortcut conv
UP_SKIP_SPLIT = 256
RESIDUAL_BLOCK = "down_blocks.1.attentions.0."           # the block of the resolution probe


def fault_tap(fault):
    """the `tap` of a named wiring fault; ("xf_residual_scaled", s): one transformer block's residual gradient times s"""
    if fault is None:
        return None
    if fault == "up_emb_detached":                       # (a) one up-block resnet's contribution to d emb lost (1 of 22)
        return lambda n, x: x.detach() if n == "up_blocks.1.resnets.1.emb_act" else x
    if fault in ("down2_emb_halved", "down3_emb_halved"):  # (b) ... mis-scaled (x 0.5) in the two resnets of one down level
        pre = f"down_blocks.{fault[4]}.resnets."
        return lambda n, x: _ScaleGrad.apply(x, 0.5) if n.startswith(pre) and n.endswith("emb_act") else x
    if fault == "up_skip_shortcut_detached":             # (c) the shortcut conv's gradient never reaches the skip half (r1 of res_bwd)
        def tap(n, x):
            if n != UP_SKIP_RESNET + "shortcut_in":
                return x
            assert x.shape[1] > UP_SKIP_SPLIT
            return torch.cat([x[:, :UP_SKIP_SPLIT], x[:, UP_SKIP_SPLIT:].detach()], 1)
        return tap
    if isinstance(fault, tuple) and fault[0] == "xf_residual_scaled":
        return lambda n, x: _ScaleGrad.apply(x, float(fault[1])) if n == RESIDUAL_BLOCK + "residual" else x
    raise ValueError(f"unknown fault {fault!r}")


FAULTS = ("up_emb_detached", "down2_emb_halved", "down3_emb_halved", "up_skip_shortcut_detached")


# ---------------------------------------------------------------------------------------------- reference, restatement
def reference(model, case, P):
    """(loss, {name: fp32 gradient}) of the fp32 oracle"""
    if model == "unet":
        x, t, ctx, target = unet_inputs(case)
        loss, _, g = OP.unet_train_grads(P, OU.TINY_UNET, x, t, ctx, target, emulate_bf16=False)
    else:
        x, tgt = vae_inputs(case)
        loss, _, g = OP.vae_train_grads(P, OV.TINY_VAE, x, tgt, emulate_bf16=False)
    return loss, g


def restatement(model, case, P, elem, fault=None):
    """(loss, {name: gradient}) of the rounding-point restatement in `elem`, optionally with a wiring fault on top"""
    S = LOSS_SCALE[elem]
    if model == "unet":
        x, t, ctx, target = unet_inputs(case)
        loss, _, g = OP.unet_train_grads(P, OU.TINY_UNET, x, t, ctx, target, emulate_bf16=elem, grad_scale=S, train_points=True,
                                         tap=fault_tap(fault), dtype=torch.float64)
    else:
        assert fault is None
        x, tgt = vae_inputs(case)
        loss, _, g = OP.vae_train_grads(P, OV.TINY_VAE, x, tgt, emulate_bf16=elem, grad_scale=S, train_points=True, dtype=torch.float64)
    return loss, g


def unet_eval(case, elem, fault=None, P=None):
    """(reference gradients, restatement gradients) of one UNet case, as attn_eval / gn_eval of train_refs.py"""
    P = host_params("unet") if P is None else P
    return reference("unet", case, P)[1], restatement("unet", case, P, elem, fault)[1]


# ---------------------------------------------------------------------------------------------- figures and bounds
def _norm(x):
    return float(x.detach().double().cpu().norm())


def absolute_set(ref):
    """names judged absolutely, from the reference gradients alone: see the module docstring"""
    out = set()
    for k in ref:
        for leaf in ("to_q.weight", "to_k.weight", "to_q.bias", "to_k.bias"):
            if k.endswith("." + leaf):
                tov = k[:-len(leaf)] + "to_v." + leaf.split(".")[1]
                if _norm(ref[k]) <= ABS_COND * _norm(ref[tov]):
                    out.add(k)
    return out


def to_v_of(k):
    stem, leaf = k.rsplit(".", 1)
    return stem.rsplit(".", 1)[0] + ".to_v." + leaf


def errors(grads, ref, absolute=()):
    """(whole-gradient rel-L2 over every parameter, {name: ||g - r|| / ||r||} of the relatively judged ones) in float64"""
    num = den = 0.0
    per = {}
    for k, r in ref.items():
        g = grads[k].detach().double().cpu(); r = r.detach().double().cpu()
        assert g.shape == r.shape, f"{k}: shape {tuple(g.shape)} vs {tuple(r.shape)}"
        assert torch.isfinite(g).all(), f"{k}: non-finite gradient"
        n2 = float((g - r).pow(2).sum()); d2 = float(r.pow(2).sum())
        num += n2; den += d2
        if k not in absolute:
            per[k] = (n2 / d2) ** 0.5
    return (num / den) ** 0.5, per


def measure(model, case, elem, P=None):
    """the restatement's figures: (whole, median parameter, {name: floor}) and the absolute set"""
    P = host_params(model) if P is None else P
    _, ref = reference(model, case, P)
    _, g = restatement(model, case, P, elem)
    ab = absolute_set(ref)
    whole, per = errors(g, ref, ab)
    return (whole, statistics.median(per.values()), per), ab


def bounds(key):
    """recorded floors of "<model>/<case>/<elem>" -> (whole-gradient bound, per-parameter bound function)"""
    whole, med, own = FLOORS[key]
    return FACTOR_WHOLE * whole, lambda k: FACTOR_PARAM * max(own.get(k, 0.0), med)


def check(key, grads, ref, loss, ref_loss, absolute):
    """the assertions of one (case, element): returns the printable line `key whole e/b worst <name> e/b`.  On failure names
    the five worst parameters (error / bound)."""
    wb, pb = bounds(key)
    whole, per = errors(grads, ref, absolute)
    ranked = sorted(((e / pb(k), e, k) for k, e in per.items()), reverse=True)
    line = f"{key} whole {whole:.3e}/{wb:.3e} worst {ranked[0][2]} {ranked[0][1]:.3e}/{pb(ranked[0][2]):.3e}"
    for k in sorted(absolute):
        ratio = _norm(grads[k]) / _norm(grads[to_v_of(k)])
        line += f" | {k} / to_v {ratio:.2e}"
        assert ratio <= ABS_TOL, f"{key}: {k}: gradient norm {ratio:.3e} x that of to_v, expected essentially zero (<= {ABS_TOL:.0e})\n{line}"
    print(line)
    assert abs(loss - ref_loss) <= LOSS_TOL * abs(ref_loss), f"{key}: loss {loss} vs fp32 oracle {ref_loss}"
    five = ", ".join(f"{k} {e:.3e}/{pb(k):.3e}" for _, e, k in ranked[:5])
    assert ranked[0][0] <= 1.0, f"{key}: parameters outside their bound (error/bound), worst five: {five}"
    assert whole <= wb, f"{key}: whole-gradient rel-L2 {whole:.3e} > {wb:.3e}; worst five parameters: {five}"
    return line


def caught(key, grads, ref, absolute):
    """[(error / bound, error, name)] of the parameters a gradient puts outside their bounds, worst first"""
    _, pb = bounds(key)
    _, per = errors(grads, ref, absolute)
    return sorted(((e / pb(k), e, k) for k, e in per.items() if e > pb(k)), reverse=True)


try:
    from train_walk_floors import FLOORS
except ImportError:                                      # only while the table is being regenerated
    FLOORS = {}

if __name__ == "__main__":                               # regenerate train_walk_floors.py
    print('"""Recorded restatement figures of train_walk_refs.py: "<model>/<case>/<elem>" -> (whole gradient, median parameter,\n'
          '{parameter: floor} where the floor exceeds the median).  Regenerate with `python tests/train_walk_refs.py`;\n'
          'test_train_walk_host.py re-measures every entry."""')
    print("FLOORS = {")
    for model, case in ALL_KEYS:
        for elem in ELEMS:
            (whole, med, per), _ = measure(model, case, elem)
            print(f'    "{model}/{case}/{elem}": ({whole:.3e}, {med:.3e}, {{')
            for k, e in per.items():
                if e > med:
                    print(f'        "{k}": {e:.3e},')
            print("    }),")
    print("}")
