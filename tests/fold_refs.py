"""fp64 references, rounding-point restatements and the case / tolerance tables of the ff.net.2 + proj_out fold (dmx_set_ff_fold).

Shared by test_ff_fold_gpu.py (HIP vs fp64) and test_ff_fold_host.py (restatement vs fp64, on the CPU); the machinery is train_refs.py's /
fwd_refs.py's: `*_eval(case, elem, fault=None)` returns (inputs, qty) with qty = {name: Q(ref, model, kind, base, dims, whole_ref)}.

The block tail is   h4 = g Wf2^T + bf2 + h3 ;  y = h4 Wpo^T + bpo + x   (fp64 reference, on the 16-bit inputs), and folded
                    y = [g | h3] [W' | Wpo]^T + b' + x,   W' = round16(Wpo Wf2),  b' = bpo + Wpo bf2.
The restatement rounds where the fold rounds: W' once to the 16-bit element, y once; b' and every sum stay wide (the kernels sum in fp32 -
the accumulation order is not restated).  Bounds (train_refs.tol_of): whole tensor TOL_CHAIN_Y1 - the project's figure for the same block
output produced by the chain kernel, which rounds h and y once each; per slice that figure, or 3 x the restatement's worst slice where it
exceeds a third of it.  The composed bias is an fp32 quantity (kind "32").  The composed weight has a bound PER ELEMENT (compose_bound):
one 16-bit rounding of the exact value plus the fp32 summation bound of a C-term dot product.
`fault=` injects one defect the cases exist for into the restatement (test_ff_fold_host.py): each must exceed the bound."""
import math

import torch

from fwd_refs import TOL_CHAIN_Y1
from train_refs import ELEMS, Q, inp, measure, q16, q32, rnd, tol_of  # noqa: F401  (re-exported for the tests)
from util import seeded

D = torch.float64
# C of the composition kernel's cases: 64 and 128 (whole 64 x 64 tiles; K = 4C = 256 / 512), 88: no multiple of the 64-wide tile in n, of the
# 64-wide tile in k (352) or of the 16-deep j slab - every ragged edge of the kernel at once
COMPOSE_C = (64, 128, 88)
# (M, C) of the folded tail: M = 64 is less than one 128-row tile, 192 = one whole tile + a ragged one
TAIL_CASES = [(64, 64), (192, 64), (64, 128), (192, 128)]
FAULTS = ("segments_swapped", "bf2_not_through_wpo", "wf2_transposed", "stale_w")


def weights(C, elem, seed=0):
    """Wpo [C][C], Wf2 [C][4C] (16-bit values), bf2, bpo (fp32 values), all in fp64 containers"""
    wpo = inp((C, C), 11 + seed, elem, 1.0 / math.sqrt(C))
    wf2 = inp((C, 4 * C), 12 + seed, elem, 1.0 / math.sqrt(4 * C))
    bf2 = (0.1 * seeded((C,), 13 + seed)).float().double()
    bpo = (0.1 * seeded((C,), 14 + seed)).float().double()
    return wpo, wf2, bf2, bpo


def compose(wpo, wf2, bf2, bpo, elem, fault=None):
    """the restated composition: ([W' | Wpo] with W' rounded once, b')"""
    C = wpo.shape[0]
    w2 = wf2.reshape(4 * C, C).t() if fault == "wf2_transposed" else wf2           # (the bytes of Wf2 read as [4C][C])
    wp = rnd(wpo @ w2, elem)
    b = bpo + (bf2 if fault == "bf2_not_through_wpo" else wpo @ bf2)
    return torch.cat([wpo, wp] if fault == "segments_swapped" else [wp, wpo], 1), b


def compose_bound(wpo, wf2):
    """per element: |got - ref64| <= 2^-8 |ref64| + C 2^-23 sum_j |wpo[n][j] wf2[j][k]|"""
    C = wpo.shape[0]
    return 2.0 ** -8 * (wpo @ wf2).abs() + C * 2.0 ** -23 * (wpo.abs() @ wf2.abs())


def compose_eval(C, elem, fault=None):
    wpo, wf2, bf2, bpo = weights(C, elem)
    w, b = compose(wpo, wf2, bf2, bpo, elem, fault)
    ref_w = torch.cat([wpo @ wf2, wpo], 1)
    ref_b = bpo + wpo @ bf2
    b32 = bpo.float() + wpo.float() @ bf2.float()
    if fault == "bf2_not_through_wpo": b32 = b.float()
    qty = {"b": q32(ref_b, b32, [0])}
    return dict(wpo=wpo, wf2=wf2, bf2=bf2, bpo=bpo), qty, (ref_w, w)


def tail_eval(case, elem, fault=None):
    M, C = case
    wpo, wf2, bf2, bpo = weights(C, elem)
    g, h3, x = inp((M, 4 * C), 1, elem), inp((M, C), 2, elem), inp((M, C), 3, elem)
    ref = (g @ wf2.t() + bf2 + h3) @ wpo.t() + bpo + x
    if fault == "stale_w":                                    # W' / b' of the weights before a change, the walk on the new ones
        w, b = compose(*weights(C, elem, seed=100), elem)
    else:
        w, b = compose(wpo, wf2, bf2, bpo, elem, fault)
    mod = rnd(torch.cat([g, h3], 1) @ w.t() + b + x, elem)
    return dict(g=g, h3=h3, x=x, wpo=wpo, wf2=wf2, bf2=bf2, bpo=bpo), {"y": q16(ref, mod, TOL_CHAIN_Y1, [0, 1], True, elem)}


def all_cases():
    out = []
    for elem in ("bf16", "fp16"):
        for C in COMPOSE_C: out.append((f"compose/{C}/{elem}", lambda C=C, e=elem: compose_eval(C, e)[:2]))
        for c in TAIL_CASES: out.append((f"tail/{c[0]}x{c[1]}/{elem}", lambda c=c, e=elem: tail_eval(c, e)))
    return out


def measure_all():
    return {f"{key}:{name}": measure(q) for key, thunk in all_cases() for name, q in thunk()[1].items()}


def bounds(key, qty):
    """{name: (whole bound, slice bound)} of one evaluated case from the recorded floors"""
    return {name: tol_of(q, FLOORS[f"{key}:{name}"]) for name, q in qty.items()}


try:
    from fold_floors import FLOORS   # the recorded table: "family/case/element:quantity" -> (whole, worst slice) figure
except ImportError:                  # only while the table is being regenerated
    FLOORS = {}

if __name__ == "__main__":                                   # regenerate fold_floors.py's table
    for k, (w, s) in measure_all().items():
        print(f'    "{k}": ({w:.3e}, {s:.3e}),')
