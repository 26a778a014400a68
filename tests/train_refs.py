"""fp64 references, rounding-point restatements and the case / tolerance tables of the training-kernel layout tests.

Shared by test_train_layout_gpu.py (HIP kernel vs fp64) and test_train_refs_host.py (restatement vs fp64, on the CPU).
Every `*_eval` function builds one case's inputs (rounded to the 16-bit element of the build) and returns
  inputs : dict of float64 CPU tensors that hold exactly representable 16-bit / fp32 values
  qty    : {name: Q(ref, model, kind, base, dims, whole_ref)}
with  ref        the fp64 result,
      model      kind "16": the restatement - fp64 arithmetic rounded where the kernel is documented to round (P and dS
                 to the 16-bit element, every 16-bit output stored rounded); kind "32": the same quantity computed by torch
                 in float32,
      base       the per-kernel whole-tensor bound of test_train_ops_gpu.py,
      dims       the slice axes of the per-slice check,
      whole_ref  what the whole-tensor bound is taken against (the rounded fp64 value where test_train_ops_gpu.py rounds its
                 oracle, else `ref`).
Bounds (tol_of): kind "16": whole = base; slice = base, or 3 x the restatement's worst slice where that exceeds base / 3 (the
restatement has the rounding points, not the MFMA accumulation order or the 1-ulp exp).  kind "32": 8 x the float32 torch
deviation from fp64, never below 2^-20; kind "x" (the kernels that only move or cast: transposes, add, casts): the single torch
operation, compared bit for bit - no tolerance.  FLOORS records the measured restatement figures the bounds are computed from;
test_train_refs_host.py re-measures them."""
import math
from collections import namedtuple

import torch
import torch.nn.functional as F

from util import rel_l2, seeded, slice_err

TOL_W, TOL_D, TOL_N, TOL_A, TOL_F = 2e-3, 1e-3, 4e-3, 1.5e-2, 4e-3      # test_train_ops_gpu.py's bounds (TOL_F: the forwards)
TOL_F16_ATTN_FWD = 2e-3                                                  # test_ops_gpu.py: fp16 forward attention
ELEMS = {"bf16": torch.bfloat16, "fp16": torch.float16}
GS_BASE = 2.0 ** -7           # gradient-scaling cases: upstream gradient ~ N(0, 2^-7) times the GradScaler factor
GS_FACTORS = (1.0, 2.0 ** 10, 2.0 ** 16)
Q = namedtuple("Q", "ref model kind base dims whole_ref")


def rnd(x, elem):
    """round to the 16-bit element, back in a float64 container"""
    return x.to(torch.float32).to(ELEMS[elem]).to(torch.float64)


def inp(shape, seed, elem, scale=1.0):
    return rnd(seeded(shape, seed) * scale, elem)


def q16(ref, model, base, dims, rounded_whole, elem):
    return Q(ref, model, "16", base, dims, rnd(ref, elem) if rounded_whole else ref)


def q32(ref, f32, dims):
    return Q(ref, f32.double(), "32", None, dims, ref)


def qx(want):
    """a bit-exact quantity: `want` holds the expected values (exactly representable in the output type)"""
    return Q(want, want, "x", None, [0], want)


def rel_l2_f64(a, b):
    """util.rel_l2 casts both sides to float32, which would measure an fp32 output against the ROUNDED fp64 reference: fp32
    quantities take their whole-tensor figure in double"""
    a = a.detach().double().cpu(); b = b.detach().double().cpu()
    return float((a - b).norm() / b.norm().clamp_min(1e-300))


def measure(q):
    """(whole-tensor figure, worst-slice figure) of the restatement / float32 computation against fp64"""
    w = rel_l2(q.model, q.whole_ref) if q.kind == "16" else rel_l2_f64(q.model, q.ref)
    s = max(slice_err(q.model, q.ref, d)[0] for d in q.dims)
    return w, s


def tol_of(q, floor):
    """(whole-tensor bound, per-slice bound) from the recorded floor (whole, slice)"""
    fw, fs = floor
    if q.kind == "x":
        return 0.0, 0.0
    if q.kind == "32":
        return max(8 * fw, 2.0 ** -20), max(8 * fs, 2.0 ** -20)
    return q.base, (q.base if fs <= q.base / 3 else 3 * fs)


# ---------------------------------------------------------------------------------------------- attention
ATTN_CASES = [
    # name, layout, B, H, Sq, Skv : the dq kernel tiles 128 queries x 64 keys, the dkv kernel 128 keys x 32 queries
    ("self_128", "self", 2, 5, 128, 128),          # one tile exactly (dq queries, dkv keys)
    ("self_129_h1", "self", 2, 1, 129, 129),       # tile + 1
    ("self_127_h20", "self", 1, 20, 127, 127),     # tile - 1
    ("self_577_h2", "self", 1, 2, 577, 577),
    ("cross_32x64_h1", "cross", 2, 1, 32, 64),     # one tile exactly (dkv queries, dq keys)
    ("cross_33x65", "cross", 2, 5, 33, 65),
    ("cross_31x63", "cross", 2, 5, 31, 63),
    ("cross_200x150", "cross", 1, 3, 200, 150),
    ("cross_256x577", "cross", 2, 5, 256, 577),    # the product's context: sp = 640 rows per sample, 577 live
]
ATTN_GS_CASE = ("cross_33x65", "cross", 2, 5, 33, 65)
ATTN_SCALE = 0.125


def _heads(x, H):
    B, S, _ = x.shape
    return x.view(B, S, H, 64).transpose(1, 2)            # [B,H,S,64]


def _unheads(x):
    B, H, S, _ = x.shape
    return x.transpose(1, 2).reshape(B, S, H * 64)


def attn_eval(case, elem, gscale=1.0, fault=None):
    name, layout, B, H, Sq, Skv = case
    C = H * 64
    k = seeded((B, Skv, C), 2)
    k[:, 3] *= 6.0                                       # a spiked key in the first key tile ...
    k[:, Skv - 1] *= 5.0                                 # ... and in the last one
    q, k, v, do = inp((B, Sq, C), 1, elem), rnd(k, elem), inp((B, Skv, C), 3, elem), inp((B, Sq, C), 4, elem, gscale)
    qh, kh, vh, doh = _heads(q, H), _heads(k, H), _heads(v, H), _heads(do, H)
    s = qh @ kh.transpose(-1, -2) * ATTN_SCALE
    lse = torch.logsumexp(s, -1) / math.log(2.0)
    P = torch.softmax(s, -1)
    o = P @ vh
    dP = doh @ vh.transpose(-1, -2)
    dS = P * (dP - (doh * o).sum(-1, keepdim=True)) * ATTN_SCALE
    ref = dict(o=_unheads(o), lse=lse, dq=_unheads(dS @ kh), dk=_unheads(dS.transpose(-1, -2) @ qh), dv=_unheads(P.transpose(-1, -2) @ doh))
    # restatement: forward P = exp(s - max) rounded before P V, o stored rounded; backward P recomputed from the fp32 lse,
    # P (for dV) and dS (for dQ / dK) rounded to the 16-bit element, delta from the stored o, outputs stored rounded
    m = s.max(-1, keepdim=True).values
    e = torch.exp(s - m)
    o_m = rnd((rnd(e, elem) @ vh) / e.sum(-1, keepdim=True), elem)
    lse32 = lse.float().double()
    Pm = torch.exp2(s / math.log(2.0) - lse32.unsqueeze(-1))
    dSm = rnd(Pm * (dP - (doh * o_m).sum(-1, keepdim=True)) * ATTN_SCALE, elem)
    if fault == "last_query_tile":                       # dS of the ragged last 32-query tile dropped: those rows' dq vanish, dk loses them
        dSm = dSm.clone(); dSm[:, :, (Sq - 1) // 32 * 32:, :] = 0
    mod = dict(o=_unheads(o_m), dq=rnd(_unheads(dSm @ kh), elem), dk=rnd(_unheads(dSm.transpose(-1, -2) @ qh), elem),
               dv=rnd(_unheads(rnd(Pm, elem).transpose(-1, -2) @ doh), elem))
    lse_f32 = torch.logsumexp((qh.float() @ kh.float().transpose(-1, -2)) * ATTN_SCALE, -1) / math.log(2.0)
    v4 = lambda t: t.view(B, -1, H, 64)
    row_head = [(0, 1), 2]
    qty = {"o": q16(v4(ref["o"]), v4(mod["o"]), TOL_F16_ATTN_FWD if elem == "fp16" else TOL_F, row_head, True, elem),
           "lse": q32(lse, lse_f32, [(0, 2), 1]),
           "dq": q16(v4(ref["dq"]), v4(mod["dq"]), TOL_A, row_head, False, elem),
           "dk": q16(v4(ref["dk"]), v4(mod["dk"]), TOL_A, row_head, False, elem),
           "dv": q16(v4(ref["dv"]), v4(mod["dv"]), TOL_A, row_head, False, elem)}
    return dict(q=q, k=k, v=v, do=do), qty


# ---------------------------------------------------------------------------------------------- GroupNorm
GN_CASES = [
    # name, B, H, W, C, groups, silu, c0 : HW is no multiple of the apply kernel's rows per block (multiples of 8 / 16)
    ("960_straddle_silu", 3, 5, 7, 960, 32, True, 656),     # groups of 30 channels: group 21 = channels 630..659 straddles c0 = 656
    ("64_plain", 3, 9, 7, 64, 32, False, None),
    ("320_straddle", 3, 3, 3, 320, 32, False, 168),         # groups of 10: group 16 = 160..169 straddles c0 = 168
]
GN_GS_CASE = GN_CASES[0]


def _gn_autograd(x, gamma, beta, dy, G, silu, dt):
    x, g, b = (t.detach().to(dt).clone().requires_grad_(True) for t in (x, gamma, beta))
    u = F.group_norm(x, G, g, b, eps=1e-5)
    y = F.silu(u) if silu else u
    y.backward(dy.to(dt))
    B, C = x.shape[:2]
    xg = x.detach().reshape(B, G, -1)
    mean = xg.mean(-1); rstd = (xg.var(-1, unbiased=False) + 1e-5).rsqrt()
    return y.detach(), x.grad, g.grad, b.grad, torch.stack([mean, rstd], -1)


def gn_eval(case, elem, gscale=1.0, fault=None):
    name, B, H, W, C, G, silu, c0 = case
    x = inp((B, C, H, W), 1, elem, 1.5) + rnd(torch.tensor(0.3), elem)
    x = rnd(x, elem)
    gamma = (1.0 + 0.1 * seeded((C,), 2)).double(); beta = (0.1 * seeded((C,), 3)).double()
    dy, r = inp((B, C, H, W), 4, elem, gscale), inp((B, C, H, W), 5, elem, gscale)
    y, dx, dg, db, st = _gn_autograd(x, gamma, beta, dy, G, silu, torch.float64)
    y32, dx32, dg32, db32, st32 = _gn_autograd(x, gamma, beta, dy, G, silu, torch.float32)
    dxr = dx + r
    dxm = rnd(dxr, elem)
    if fault == "straddle_group_scaled":                     # a stand-in for any error confined to the straddling group: its dx off by 10 %
        cpg = C // G; g0 = c0 // cpg
        dxm = dxm.clone(); dxm[:, g0 * cpg:(g0 + 1) * cpg] *= 1.1
    nh = lambda t: t.permute(0, 2, 3, 1).reshape(B, H * W, G, C // G)          # [B][HW][group][channel in group]
    qty = {"y": q16(nh(y), nh(rnd(y, elem)), TOL_F, [(0, 2), (2, 3)], True, elem),
           "dx": q16(nh(dxr), nh(dxm), TOL_N, [(0, 2), (2, 3), (0, 1)], True, elem),
           "dgamma": q32(dg, dg32, [0]), "dbeta": q32(db, db32, [0]), "stats": q32(st, st32, [(0, 1, 2)])}
    return dict(x=x, gamma=gamma, beta=beta, dy=dy, r=r), qty


# ---------------------------------------------------------------------------------------------- LayerNorm / GEGLU
LN_CASES = [(1, 320), (33, 2048), (15, 8), (17, 640)]        # rows = 1, 33, 4 * LNB_ROWS -/+ 1 ; C = 8 and the maximum 2048
LN_GS_CASE = (17, 640)


def _ln_autograd(x, gamma, beta, dy, dt):
    x, g, b = (t.detach().to(dt).clone().requires_grad_(True) for t in (x, gamma, beta))
    F.layer_norm(x, (x.shape[-1],), g, b, eps=1e-5).backward(dy.to(dt))
    return x.grad, g.grad, b.grad


def ln_eval(case, elem, gscale=1.0):
    rows, C = case
    x = rnd(inp((rows, C), 1, elem, 2.0) + 0.5, elem)
    gamma = (1.0 + 0.1 * seeded((C,), 2)).double(); beta = (0.1 * seeded((C,), 3)).double()
    dy, r = inp((rows, C), 4, elem, gscale), inp((rows, C), 5, elem, gscale)
    dx, dg, db = _ln_autograd(x, gamma, beta, dy, torch.float64)
    dx32, dg32, db32 = _ln_autograd(x, gamma, beta, dy, torch.float32)
    qty = {"dx": q16(dx + r, rnd(dx + r, elem), TOL_N, [0, 1], True, elem), "dgamma": q32(dg, dg32, [0]), "dbeta": q32(db, db32, [0])}
    return dict(x=x, gamma=gamma, dy=dy, r=r), qty


GEGLU_CASES = [(1, 8), (33, 320), (300, 1280)]
GEGLU_GS_CASE = (33, 320)


def geglu_eval(case, elem, gscale=1.0):
    rows, C2 = case
    h = seeded((rows, 2 * C2), 1) * 1.5
    h[:, C2:] = (seeded((rows, C2), 6) * 3.0).clamp(-8.0, 8.0)       # gates out to the GELU tails
    h[0, C2:C2 + 4] = torch.tensor([8.0, -8.0, 6.0, -6.0])
    h = rnd(h, elem).requires_grad_(True)
    dy = inp((rows, C2), 2, elem, gscale)
    a, g = h.chunk(2, dim=-1)
    y = a * F.gelu(g)
    y.backward(dy)
    y = y.detach(); dh = h.grad; h = h.detach()
    qty = {"y": q16(y, rnd(y, elem), TOL_F, [0, 1], True, elem), "dh": q16(dh, rnd(dh, elem), TOL_F, [0, 1], True, elem)}
    return dict(h=h, dy=dy), qty


# ---------------------------------------------------------------------------------------------- wgrad / colsum / dgrad
CONV_CASES = [
    # name, B, H, W, Cin, Cout, stride, fwd pad, asym ((0,1,0,1) pad in front of a pad-0 conv: the VAE's downsample)
    ("s2_asym", 2, 16, 16, 64, 64, 2, 0, True),
    ("uneven_split", 5, 12, 12, 64, 96, 1, 1, False),       # M = 720: three split partials of 256 / 256 / 208 rows
    ("tailM_5x7", 3, 5, 7, 64, 64, 1, 1, False),
]
# the data gradient is a dmx_conv_gemm with N = Cin: the GEMM puts no lower bound on N; N % 8 != 0 (or ldo % 8 != 0) leaves the
# coalesced 8-channel epilogue for the scalar one (split-K wants N % 4).  Cin = 4 is the narrowest the product runs (the VAE
# decoder's conv_in data gradient, N = latent channels): scalar stores, row stride 20, residual added there.  Cin = 8 stays coalesced.
DGRAD_EXTRA = [("narrow_cin4", 2, 12, 12, 4, 64, 1, 1, False), ("narrow_cin8", 2, 12, 12, 8, 64, 1, 1, False)]
CONV_GS_CASE = CONV_CASES[0]


def conv_eval(case, elem, gscale=1.0):
    name, B, H, W, Cin, Cout, st, pad, asym = case
    def run(dt):
        x, w = (t.detach().to(dt).clone().requires_grad_(True) for t in (X, Wt))
        y = F.conv2d(F.pad(x, (0, 1, 0, 1)) if asym else x, w, None, stride=st, padding=pad)
        y.backward(DY.to(dt))
        return x.grad, w.grad
    X = inp((B, Cin, H, W), 1, elem); Wt = inp((Cout, Cin, 3, 3), 2, elem, 1.0 / math.sqrt(Cin * 9))
    OH = H // st; OW = W // st
    DY = inp((B, Cout, OH, OW), 3, elem, gscale); R = inp((B, Cin, H, W), 4, elem, gscale)
    dx, dw = run(torch.float64)
    _, dw32 = run(torch.float32)
    pk = lambda t: t.permute(0, 2, 3, 1).reshape(Cout, 9, Cin)               # packed [n][tap][c]
    nh = lambda t: t.permute(0, 2, 3, 1)
    qty = {"dw": q32(pk(dw), pk(dw32), [0, 1]),
           "dx": q16(nh(dx), nh(rnd(dx, elem)), TOL_D, [3, (0, 1, 2)], True, elem),
           "dx_res": q16(nh(dx + R), nh(rnd(dx + R, elem)), 2 * TOL_D, [3, (0, 1, 2)], True, elem)}
    return dict(x=X, w=Wt, dy=DY, r=R), qty


COLSUM_CASES = [("g3_rpg35", 3, 35, 200), ("g3_rpg300", 3, 300, 200), ("g1_rows900", 1, 900, 72)]    # row step 32, chunks of 256 rows
COLSUM_GS_CASE = COLSUM_CASES[1]


def colsum_eval(case, elem, gscale=1.0):
    name, G, rpg, N = case
    dy = inp((G, rpg, N), 5, elem, gscale)
    return dict(dy=dy), {"colsum": q32(dy.sum(1), dy.float().sum(1), [0, 1])}


MSE_SIZES = [1, 255, 256, 257, 1024 * 256 + 513]


def mse_eval(n):
    p = seeded((n,), 1).double(); t = seeded((n,), 2).double()
    loss = ((p - t) ** 2).mean().reshape(1)
    return dict(pred=p, target=t), {"loss": q32(loss, F.mse_loss(p.float(), t.float()).reshape(1), [0])}


# ---------------------------------------------------------------------------------------------- the small training kernels
# (test_train_small_gpu.py, through the dmx_test_* entries).  Bit-exact ones first: transposes, add, the casts of the posterior mode.
TRANSPOSE_CASES = [(1, 1), (31, 33), (32, 32), (33, 31), (64, 4), (577, 130), (1280, 320)]      # the single kernel tiles 32 x 32


def transpose_eval(case, elem):
    x = inp(case, 1, elem)
    return dict(x=x), {"out": qx(x.t().contiguous())}


# one batch of the batched kernel (64 x 64 tiles; 16-byte accesses on a side whose stride is a multiple of 8 and whose base is
# 16-byte aligned, element accesses otherwise):  R, C, ldin, ldout, input base offset, output base offset (elements past a
# 16-byte boundary).  A one-tile job first and last: both ends of the bisection over the jobs' first tiles.
TRB_JOBS = [
    (64, 64, 72, 72, 0, 0),          # one tile, vector loads and stores
    (63, 65, 72, 64, 0, 0),          # aligned strides, ragged both ways: vector body, element edges
    (65, 63, 67, 69, 0, 0),          # odd ldin and ldout
    (1, 200, 200, 8, 0, 0),          # one row: every vector store would be 7 elements too wide
    (4, 320, 321, 8, 0, 0),          # odd ldin, vector-eligible output of 4 columns
    (129, 7, 8, 133, 0, 1),          # 7 columns: vector-eligible input never has 8 to load; odd ldout, output base off by one
    (320, 1280, 1288, 328, 3, 0),    # a real weight shape; input base off by three
    (64, 64, 72, 72, 8, 8),
    (63, 65, 72, 72, 1, 3),          # aligned strides, both bases off
    (40, 24, 24, 40, 0, 0),          # one tile, last
]


def transpose_batch_eval(elem, jobs=None, seed=0):
    jobs = TRB_JOBS if jobs is None else jobs
    xs = [inp((j[0], j[1]), 10 + seed + i, elem) for i, j in enumerate(jobs)]
    return dict(xs=xs), {f"out{i}": qx(x.t().contiguous()) for i, x in enumerate(xs)}


ADD_CASES = [(1, 8), (3, 320), (4099, 1280), (16411, 1280)]      # the last: 2.6 M vectors > 8192 blocks x 256, the grid-stride loop turns


def add_eval(case, elem):
    a, b = inp(case, 1, elem), inp(case, 2, elem)
    return dict(a=a, b=b), {"out": qx((a.float() + b.float()).to(ELEMS[elem]).double())}


CAST_CASES = [(M, C) for M in (1, 257, 4096) for C in (4, 8)]


def cast_eval(kind, case, elem):
    M, C = case
    if kind == "slice_cast":                       # z (16-bit) = the mean half of the fp32 moments [M][2C]
        mom = seeded((M, 2 * C), 1).double()
        return dict(x=mom), {"out": qx(mom[:, :C].float().to(ELEMS[elem]).double())}
    dz = inp((M, C), 1, elem)
    if kind == "mode_bwd":                         # dmom (fp32 [M][2C]) = (dz | 0)
        return dict(x=dz), {"out": qx(torch.cat([dz.float(), torch.zeros(M, C)], 1).double())}
    return dict(x=dz), {"out": qx(dz.float().double())}          # bf16_to_f32_rows


CAST_KINDS = ("slice_cast", "mode_bwd", "bf16_to_f32_rows")

# ---- row softmax (the VAE's single-head d = 512 attention: fp32 scores -> 16-bit P) and its backward
SM_SCALE = float(torch.tensor(1.0 / math.sqrt(512.0), dtype=torch.float32))
SM_N = (1, 63, 64, 255, 256, 257, 1000, 4096)            # one block of 256 threads per row: n < / = / > one pass of the loops
SM_ROWS = (1, 5)
SM_PATTERNS = ("gauss", "equal", "spike")
SM_CASES = [(p, r, n) for p in SM_PATTERNS for r in SM_ROWS for n in SM_N]
SMB_CASES = [(r, n) for r in SM_ROWS for n in SM_N]
# the gradient-scaling case: scores 4 x as wide, so each row has a few P of 0.1 .. 0.9 and the dS that carry the row stay fp16
# normals at GS_BASE x 1 (with P ~ 1 / n every dS of that factor, ~1e-6, would be a subnormal and its rounding would set the bound
# of the larger factors too)
SMB_GS_CASE = (5, 257, 4.0)


def _scores(pattern, rows, n):
    s = seeded((rows, n), 1) * math.sqrt(512.0)           # scaled scores ~ N(0, 1)
    if pattern == "equal":
        s = torch.full((rows, n), 3.25)
    if pattern == "spike":                                # one score 1e4 above the rest (test_attention_reference_max_stress)
        for r in range(rows):
            s[r, (n - 1 - 97 * r) % n] = float(s[r].max()) + 1e4
    return s.float().double()


def softmax_eval(case, elem, fault=None):
    pattern, rows, n = case
    s = _scores(pattern, rows, n)
    P = torch.softmax(s * SM_SCALE, -1)
    model = rnd(P, elem)
    if fault == "first_256":                              # the loops stop after their first pass: columns >= 256 never enter
        model = torch.zeros_like(P); model[:, :256] = rnd(torch.softmax(s[:, :256] * SM_SCALE, -1), elem)
    return dict(s=s), {"p": q16(P, model, TOL_D, [0, 1], True, elem)}


def softmax_bwd_eval(case, elem, gscale=1.0, fault=None):
    rows, n = case[:2]
    sharp = case[2] if len(case) > 2 else 1.0
    P = rnd(torch.softmax(_scores("gauss", rows, n) * SM_SCALE * sharp, -1), elem)       # the kernel's input: P as stored
    dP = (seeded((rows, n), 2) * gscale).float().double()
    dS = SM_SCALE * P * (dP - (P * dP).sum(-1, keepdim=True))
    if gscale != 1.0:                                     # the 16-bit output must stay finite at the largest GradScaler factor
        assert float(dS.abs().max()) / gscale * GS_BASE * GS_FACTORS[-1] < 65504.0
    model = rnd(dS, elem)
    if fault == "first_256":
        model = torch.zeros_like(dS)
        model[:, :256] = rnd(SM_SCALE * P[:, :256] * (dP[:, :256] - (P[:, :256] * dP[:, :256]).sum(-1, keepdim=True)), elem)
    return dict(p=P, dp=dP), {"ds": q16(dS, model, TOL_D, [0, 1], True, elem)}


# ---- 1x1 convolutions between <= 8 channels (quant_conv / post_quant_conv): one thread per row, 256 rows per block, the
# per-block partials of dW / db folded by a second kernel
PW_CH = [(4, 4), (8, 8), (8, 4), (3, 8), (1, 1)]
PW_M = (1, 255, 256, 257, 4099)
PW_CASES = [(ci, co, M) for ci, co in PW_CH for M in PW_M]
PW_GS_CASE = (8, 4, 257)
PW_LDW = 64                                               # the padded K of the real weights (1x1 conv: Cin rounded up to 64)


def pw_eval(case, elem, gscale=1.0):
    Cin, Cout, M = case
    x = inp((M, Cin), 1, elem); w = inp((Cout, Cin), 2, elem, 1.0 / math.sqrt(Cin))
    bias = (0.1 * seeded((Cout,), 3)).double()
    dy = (seeded((M, Cout), 4) * gscale).float().double()
    ynb = x @ w.t(); y = ynb + bias
    ynb32 = x.float() @ w.float().t(); y32 = bias.float() + ynb32
    dx = dy @ w
    if gscale != 1.0:
        assert float(dx.abs().max()) / gscale * GS_BASE * GS_FACTORS[-1] < 65504.0
    row_ch = [0, 1]
    qty = {"y16": q16(y, rnd(y, elem), TOL_D, row_ch, True, elem), "y32": q32(y, y32, row_ch),
           "y16_nobias": q16(ynb, rnd(ynb, elem), TOL_D, row_ch, True, elem), "y32_nobias": q32(ynb, ynb32, row_ch),
           "dx": q16(dx, rnd(dx, elem), TOL_D, row_ch, True, elem),
           "dw": q32(dy.t() @ x, dy.float().t() @ x.float(), [0, 1]), "db": q32(dy.sum(0), dy.float().sum(0), [0])}
    return dict(x=x, w=w, bias=bias, dy=dy), qty


# ---- backward of the fp32 time-embedding linears y = W act(x) + b (M = batch): the dx kernel owns 8 columns k and up to 8
# samples per block and splits N over 128 lanes; the dw kernel one row n and 256 columns k per block.
#   B, N, K, silu_in, db_stride, which outputs
LSB_CASES = [
    (1, 1, 1, 0, 1, "both"), (1, 128, 8, 1, 1, "both"), (1, 127, 1283, 1, 1, "dx"),
    (3, 127, 7, 0, 3, "both"), (3, 129, 9, 1, 1, "both"), (3, 1000, 1, 1, 1, "both"),
    (8, 128, 320, 0, 1, "both"), (8, 1000, 1283, 1, 3, "both"), (8, 1, 1283, 0, 1, "both"),
    (9, 127, 7, 1, 1, "both"), (9, 129, 9, 0, 3, "both"), (9, 1000, 320, 1, 1, "both"), (9, 1, 1, 0, 1, "both"),
    (9, 128, 1283, 1, 1, "dx"), (9, 127, 9, 1, 3, "dw"), (9, 129, 7, 0, 1, "dx"),
    (17, 127, 1283, 1, 3, "both"), (17, 129, 7, 0, 1, "both"), (17, 1000, 9, 1, 1, "both"), (17, 128, 8, 0, 1, "both"),
    (17, 1, 320, 1, 1, "both"), (17, 1000, 1283, 0, 1, "dw"),
]
# SiLU on the input goes through the kernel's fast exponential: __expf(x) = v_exp_f32(fl(log2(e)) * x) - that much is the
# compiler's own header (__clang_hip_math.h: `__expf` = `__builtin_amdgcn_exp2f(__log2_e * x)`).  The accuracy of v_exp_f32 is
# taken as 1 ulp, i.e. a relative error <= 2^-23.  That figure is recalled from AMD's public CDNA3 instruction-set reference guide
# (V_EXP_F32, "1 ULP accuracy"); no ISA document was at hand to check it against when this was written, so it is an assumption
# of this bound, not a verified citation.  The argument carries the rounding of the constant (<= 2^-24 relative) and of the product
# (<= 2^-24): |d arg| <= |arg| 2^-23, which the exponential turns into a relative error of ln(2) |arg| 2^-23 = |x| 2^-23.  So
# exp(-x) is modelled with a relative error of at most (1 + |x|) 2^-23.
EXP_REL = lambda x: (1.0 + x.abs()) * 2.0 ** -23


def _silu_worst(x):
    """(worst |error| of SiLU(x), worst |error| of SiLU'(x)) over both signs of the exponential's error, in fp64"""
    e = torch.exp(-x); eta = EXP_REL(x)
    def f(ee):
        sg = 1.0 / (1.0 + ee)
        return x * sg, sg * (1.0 + x * (1.0 - sg))
    a0, d0 = f(e); ap, dp = f(e * (1 + eta)); am, dm = f(e * (1 - eta))
    return torch.maximum((ap - a0).abs(), (am - a0).abs()), torch.maximum((dp - d0).abs(), (dm - d0).abs())


def _away(v32, ref, mag):
    """the float32 value pushed by `mag` in the direction that takes it further from the reference"""
    v = v32.double()
    sgn = torch.where(v >= ref, 1.0, -1.0).double()
    return v + sgn * mag


def lsb_eval(case, elem, fault=None):
    B, N, K, silu, dbs, which = case
    x = seeded((B, K), 1).float().double(); dy = seeded((B, N), 2).float().double()
    w = inp((N, K), 3, elem, 1.0 / math.sqrt(K))
    sig = torch.sigmoid(x)
    act = x * sig if silu else x
    dact = sig * (1 + x * (1 - sig)) if silu else torch.ones_like(x)
    dw, db, g = dy.t() @ act, dy.sum(0), dy @ w
    dx = dact * g
    x32, dy32 = x.float(), dy.float()
    sig32 = 1.0 / (1.0 + torch.exp(-x32))
    act32 = x32 * sig32 if silu else x32
    dact32 = sig32 * (1.0 + x32 * (1.0 - sig32)) if silu else torch.ones_like(x32)
    dw32, g32 = dy32.t() @ act32, dy32 @ w.float()
    dx32 = dact32 * g32
    if silu:             # the float32 restatement with the exponential's documented error, signed against the reference
        ea, ed = _silu_worst(x)
        dw32 = _away(dw32, dw, dy.abs().t() @ ea)
        dx32 = _away(dx32, dx, g32.double().abs() * ed)
    if fault == "ninth_sample":                           # the second batch tile of the dx kernel never runs
        dx32 = dx32.clone(); dx32[8:] = 0
    qty = {}
    if which != "dx":
        qty["dw"] = q32(dw, dw32, [0, 1]); qty["db"] = q32(db, dy32.sum(0), [0])
    if which != "dw":
        qty["dx"] = q32(dx, dx32, [0, 1])
    return dict(x=x, dy=dy, w=w), qty


def lsb_name(c):
    return f"b{c[0]}_n{c[1]}_k{c[2]}_silu{c[3]}_dbs{c[4]}_{c[5]}"


# ---------------------------------------------------------------------------------------------- the table
def all_cases():
    """(key, thunk) for every (family, case, element[, gradient-scaling]) the GPU tests run"""
    out = []
    for elem in ("bf16", "fp16"):
        for c in ATTN_CASES: out.append((f"attn/{c[0]}/{elem}", lambda c=c, e=elem: attn_eval(c, e)))
        for c in GN_CASES: out.append((f"gn/{c[0]}/{elem}", lambda c=c, e=elem: gn_eval(c, e)))
        for c in LN_CASES: out.append((f"ln/{c[0]}x{c[1]}/{elem}", lambda c=c, e=elem: ln_eval(c, e)))
        for c in GEGLU_CASES: out.append((f"geglu/{c[0]}x{c[1]}/{elem}", lambda c=c, e=elem: geglu_eval(c, e)))
        for c in CONV_CASES + DGRAD_EXTRA: out.append((f"conv/{c[0]}/{elem}", lambda c=c, e=elem: conv_eval(c, e)))
        for c in COLSUM_CASES: out.append((f"colsum/{c[0]}/{elem}", lambda c=c, e=elem: colsum_eval(c, e)))
    # gradient scaling (fp16 build): the bounds of every factor are those of the factor-1 case
    out.append((f"attn/{ATTN_GS_CASE[0]}/fp16/gs", lambda: attn_eval(ATTN_GS_CASE, "fp16", GS_BASE)))
    out.append((f"gn/{GN_GS_CASE[0]}/fp16/gs", lambda: gn_eval(GN_GS_CASE, "fp16", GS_BASE)))
    out.append((f"ln/{LN_GS_CASE[0]}x{LN_GS_CASE[1]}/fp16/gs", lambda: ln_eval(LN_GS_CASE, "fp16", GS_BASE)))
    out.append((f"geglu/{GEGLU_GS_CASE[0]}x{GEGLU_GS_CASE[1]}/fp16/gs", lambda: geglu_eval(GEGLU_GS_CASE, "fp16", GS_BASE)))
    out.append((f"conv/{CONV_GS_CASE[0]}/fp16/gs", lambda: conv_eval(CONV_GS_CASE, "fp16", GS_BASE)))
    out.append((f"colsum/{COLSUM_GS_CASE[0]}/fp16/gs", lambda: colsum_eval(COLSUM_GS_CASE, "fp16", GS_BASE)))
    for n in MSE_SIZES: out.append((f"mse/{n}", lambda n=n: mse_eval(n)))
    # the small training kernels (test_train_small_gpu.py)
    for elem in ("bf16", "fp16"):
        for c in TRANSPOSE_CASES: out.append((f"transpose/{c[0]}x{c[1]}/{elem}", lambda c=c, e=elem: transpose_eval(c, e)))
        out.append((f"transpose_batch/{elem}", lambda e=elem: transpose_batch_eval(e)))
        for c in ADD_CASES: out.append((f"add/{c[0]}x{c[1]}/{elem}", lambda c=c, e=elem: add_eval(c, e)))
        for k in CAST_KINDS:
            for c in CAST_CASES: out.append((f"{k}/{c[0]}x{c[1]}/{elem}", lambda k=k, c=c, e=elem: cast_eval(k, c, e)))
        for c in SM_CASES: out.append((f"softmax/{c[0]}_{c[1]}x{c[2]}/{elem}", lambda c=c, e=elem: softmax_eval(c, e)))
        for c in SMB_CASES: out.append((f"softmax_bwd/{c[0]}x{c[1]}/{elem}", lambda c=c, e=elem: softmax_bwd_eval(c, e)))
        for c in PW_CASES: out.append((f"pw/{c[0]}to{c[1]}_m{c[2]}/{elem}", lambda c=c, e=elem: pw_eval(c, e)))
        for c in LSB_CASES: out.append((f"lsb/{lsb_name(c)}/{elem}", lambda c=c, e=elem: lsb_eval(c, e)))
    out.append((f"softmax_bwd/{SMB_GS_CASE[0]}x{SMB_GS_CASE[1]}/fp16/gs", lambda: softmax_bwd_eval(SMB_GS_CASE, "fp16", GS_BASE)))
    out.append((f"pw/{PW_GS_CASE[0]}to{PW_GS_CASE[1]}_m{PW_GS_CASE[2]}/fp16/gs", lambda: pw_eval(PW_GS_CASE, "fp16", GS_BASE)))
    return out


def measure_all():
    return {f"{key}:{name}": measure(q) for key, thunk in all_cases() for name, q in thunk()[1].items()}


def bounds(key, qty):
    """{name: (whole bound, slice bound)} of one evaluated case from the recorded floors"""
    return {name: tol_of(q, FLOORS[f"{key}:{name}"]) for name, q in qty.items()}


try:
    from train_floors import FLOORS  # the recorded table: "family/case/element:quantity" -> (whole, worst slice) figure
except ImportError:                  # only while the table is being regenerated
    FLOORS = {}

if __name__ == "__main__":                                   # regenerate train_floors.py's table
    for k, (w, s) in measure_all().items():
        print(f'    "{k}": ({w:.3e}, {s:.3e}),')
