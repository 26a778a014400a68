"""fp64 references, rounding-point restatements and the case / tolerance tables of the forward-kernel layout tests.

Shared by test_fwd_layout_gpu.py (HIP kernel vs fp64) and test_fwd_refs_host.py (restatement vs fp64, on the CPU).  The machinery is
train_refs.py's: every `*_eval(case, elem, fault=None)` returns (inputs, qty) with qty = {name: Q(ref, model, kind, base, dims, whole_ref)}.
The restatement rounds where the forward kernels are documented to round: P to the 16-bit element before P V; the normalised tensor once
in the halo / skinny conv; t = val * gelu(gate), h and y once each in the transformer chains; every 16-bit output once.
Bounds (train_refs.tol_of): the whole-tensor bound is the figure test_ops_gpu.py states for the kernel (`base`); the per-slice bound is
that figure, or 3 x the restatement's worst slice where that exceeds a third of it; fp32 outputs (kind "32"): 8 x the deviation of torch
float32 from fp64, never below 2^-20; kind "x": bit for bit.  fwd_floors.py records the measured restatement figures.
Halo conv, skinny conv and the chains: test_ops_gpu.py's oracle for these rounds the same intermediates, so their whole-tensor bound is taken against
the restatement itself (`whole_ref` = the clean model: the recorded whole figure is 0 by construction, and on the GPU that comparison is kernel against
restatement, as in test_ops_gpu.py); the independent check of these kernels is the per-slice one against fp64.
`fault=` injects one defect of the kind the GPU cases exist for into the restatement (test_fwd_refs_host.py)."""
import functools
import math

import torch
import torch.nn.functional as F

from train_refs import ELEMS, Q, inp, measure, q16, q32, qx, rnd, tol_of  # noqa: F401  (re-exported for the tests)
from util import seeded

TOL = 1e-3                                  # test_ops_gpu.py: conv / linear / GEGLU / GroupNorm / LayerNorm / chain residual stream
TOL_HALO_GN = 2e-3                          # halo / skinny conv behind GroupNorm; chain query / qkv
TOL_CHAIN_Y1 = 3e-3                         # chain mode 1 block output; proj_in behind the folded entry GroupNorm
TOL_ATTN = {"bf16": 4e-3, "fp16": 2e-3}     # d = 64 and wide-head attention
D = torch.float64


def nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


# ---------------------------------------------------------------------------------------------- d = 64 attention
ATTN_SCALE = 0.125
# name, B, H, Sq, Skv, kv_rows : the kernels tile 128 queries x 64 keys
ATTN64_CASES = [("exact_128x64", 2, 1, 128, 64, 64), ("129x65", 2, 5, 129, 65, 128), ("127x63", 1, 3, 127, 63, 64),
                ("200x150", 1, 2, 200, 150, 192), ("256x577", 2, 5, 256, 577, 640)]
# the balanced schedule takes Sq % 128 == 0 and at least 3 x CUs = 768 (query block, key tile) items.  768 items exactly: one item per slot,
# every query block (12 key tiles) is split over 12 slots; 832 items on 768 slots: parts of 1 and 2 tiles, the ragged last tile (41 keys) inside a part
BAL_CASES = [("bal_1024x768", 2, 4, 1024, 768, 768), ("bal_1024x809_ragged", 2, 4, 1024, 809, 832)]


def _heads(x, H):
    B, S, _ = x.shape
    return x.view(B, S, H, 64).transpose(1, 2)


def _attn_core(qh, kh, vh, scale, elem):
    s = qh @ kh.transpose(-1, -2) * scale
    ref = torch.softmax(s, -1) @ vh
    e = torch.exp(s - s.max(-1, keepdim=True).values)
    return ref, rnd((rnd(e, elem) @ vh) / e.sum(-1, keepdim=True), elem)


def attn64_eval(case, elem, fault=None):
    name, B, H, Sq, Skv, kvr = case
    C = H * 64
    k = seeded((B, Skv, C), 2)
    k[:, min(3, Skv - 1)] *= 6.0                              # a spiked key in the first key tile ...
    k[:, Skv - 1] *= 5.0                                      # ... and in the last one
    q, k, v = inp((B, Sq, C), 1, elem), rnd(k, elem), inp((B, Skv, C), 3, elem)
    kpad = inp((B, kvr - Skv, C), 98, elem, 2.0) if kvr > Skv else None      # rows [Skv, kv_rows): nothing may read them into the result
    vpad = inp((B, kvr - Skv, C), 97, elem, 2.0) if kvr > Skv else None
    qh, kh, vh = _heads(q, H), _heads(k, H), _heads(v, H)
    ref, mod = _attn_core(qh, kh, vh, ATTN_SCALE, elem)
    if fault == "pad_key_unmasked":                           # row Skv left unmasked for the query rows of the last query block
        r0 = (Sq - 1) // 128 * 128
        k1 = torch.cat([k, kpad[:, :1]], 1); v1 = torch.cat([v, vpad[:, :1]], 1)
        _, bad = _attn_core(qh[:, :, r0:], _heads(k1, H), _heads(v1, H), ATTN_SCALE, elem)
        mod = mod.clone(); mod[:, :, r0:] = bad
    u = lambda t: t.transpose(1, 2).contiguous()              # [B,Sq,H,64]
    qty = {"o": q16(u(ref), u(mod), TOL_ATTN[elem], [(0, 1), 2], True, elem)}
    return dict(q=q, k=k, v=v, kpad=kpad, vpad=vpad), qty


# ---------------------------------------------------------------------------------------------- wide-head attention
# attention_wide.hip: key tiles of 32 (the key mask), query blocks of 128 = 4 waves x 32 rows (the query clamp)
WIDE_S = (31, 32, 33, 127, 128, 129, 200)
WIDE_CASES = [(Dh, S) for Dh in (128, 256, 512) for S in WIDE_S]
WIDE_B = 2


def wide_eval(case, elem, fault=None):
    Dh, S = case
    k = seeded((WIDE_B, S, Dh), 2)
    k[0, min(37, S - 1)] *= 5.0                               # beyond the first key tile wherever S > 37: the in-place rescale branch
    q, k, v = inp((WIDE_B, S, Dh), 1, elem), rnd(k, elem), inp((WIDE_B, S, Dh), 3, elem)
    ref, mod = _attn_core(q, k, v, Dh ** -0.5, elem)
    if fault == "last_key_tile_dropped" and S > 32:           # the ragged last 32-key tile never enters
        _, mod = _attn_core(q, k[:, :(S - 1) // 32 * 32], v[:, :(S - 1) // 32 * 32], Dh ** -0.5, elem)
    return dict(q=q, k=k, v=v), {"o": q16(ref, mod, TOL_ATTN[elem], [(0, 1)], True, elem)}


# ---------------------------------------------------------------------------------------------- GroupNorm (forward)
# name, B, H, W, C0, C1, groups, silu, eps, offset (channel means = 30 x their standard deviation), path
# 192 | 128 at 32 groups: groups of 10 channels, group 19 = channels 190..199 straddles the sources (a split at a multiple of 8 can only
# straddle a group whose width does not divide it: 96 | 32 at 32 groups - groups of 4 - has no such group).
GNF_CASES = [
    ("hw1_silu", 3, 1, 1, 192, 128, 32, True, 1e-5, False, "slab"),
    ("hw35", 3, 5, 7, 192, 128, 32, False, 1e-6, False, "slab"),
    ("hw35_cancel_silu", 3, 5, 7, 192, 128, 32, True, 1e-6, True, "slab"),
    ("36x36_silu", 3, 36, 36, 192, 128, 32, True, 1e-5, False, "slab"),
    ("16x8_producer", 3, 16, 8, 192, 128, 32, True, 1e-5, False, "producer"),     # HW = 128: a producer GEMM's tiles stay inside a sample
    # groups of an odd width (160 channels at 32 groups: 5) have no register-resident slab instance (norm.hip gn_slab_launch): the two-launch path at
    # any size; 88 | 72: group 17 = channels 85..89 straddles the sources; 36 x 36 = 21 statistics chunks of 64 rows, the last one ragged
    ("two_launch_hw35", 3, 5, 7, 88, 72, 32, True, 1e-5, False, "two_launch"),
    ("two_launch_36x36", 3, 36, 36, 88, 72, 32, False, 1e-6, False, "two_launch"),
]


def gnf_eval(case, elem, fault=None):
    name, B, H, W, C0, C1, G, silu, eps, cancel, path = case
    C = C0 + C1
    x = seeded((B, C, H, W), 1) * (1.0 if cancel else 1.5) + (30.0 if cancel else 0.3)
    x = rnd(x, elem)
    gamma = (1.0 + 0.1 * seeded((C,), 2)).double(); beta = (0.1 * seeded((C,), 3)).double()
    u = F.group_norm(x, G, gamma, beta, eps)
    y = F.silu(u) if silu else u
    mod = rnd(y, elem)
    if fault == "first_source_stats":                         # the straddling group normalised with the statistics of its first source only
        cpg = C // G; g0 = C0 // cpg
        part = x[:, g0 * cpg:C0].reshape(B, -1)
        mean = part.mean(1).view(B, 1, 1, 1); var = part.var(1, unbiased=False).view(B, 1, 1, 1)
        sl = slice(g0 * cpg, (g0 + 1) * cpg)
        ub = (x[:, sl] - mean) / (var + eps).sqrt() * gamma[sl].view(1, -1, 1, 1) + beta[sl].view(1, -1, 1, 1)
        mod = mod.clone(); mod[:, sl] = rnd(F.silu(ub) if silu else ub, elem)
    nh = lambda t: t.permute(0, 2, 3, 1).reshape(B, H * W, G, C // G)
    return dict(x=x, gamma=gamma, beta=beta), {"y": q16(nh(y), nh(mod), TOL, [(0, 2), (2, 3)], True, elem)}


# ---------------------------------------------------------------------------------------------- LayerNorm (forward)
# one wave per row, four rows per block (rows 1 / 3 / 5 / 301: partial blocks); a lane holds octets lane + 64 j: C = 8 one lane, 512 one
# full pass, 520 a ragged second pass of one octet, 1280 three, 2048 all four
LNF_CASES = [(r, c) for r in (1, 3, 5, 301) for c in (8, 320, 512, 520, 1280, 2048)]


def lnf_eval(case, elem, fault=None):
    rows, C = case
    off = 20.0 * torch.where(torch.arange(rows) % 2 == 0, 1.0, -1.0).view(rows, 1)       # 20 x the row's standard deviation
    x = rnd(seeded((rows, C), 1) + off, elem)
    gamma = (1.0 + 0.1 * seeded((C,), 2)).double(); beta = (0.1 * seeded((C,), 3)).double()
    y = F.layer_norm(x, (C,), gamma, beta, 1e-5)
    mod = rnd(y, elem)
    if fault == "ragged_octet_mean":                          # the last octet (a lane's ragged second pass) left out of the row sum
        mean = x[:, :C - 8].sum(1, keepdim=True) / C
        var = ((x - mean) ** 2).mean(1, keepdim=True)
        mod = rnd((x - mean) / (var + 1e-5).sqrt() * gamma + beta, elem)
    return dict(x=x, gamma=gamma, beta=beta), {"y": q16(y, mod, TOL, [0], True, elem)}


# ---------------------------------------------------------------------------------------------- GEMM / implicit conv
# force_tn -> (rows, columns, K-tile, persistent stream-K, 160 / 320-column epilogue)   (csrc/gemm_tile.h DMX_GEMM_INSTANCES / gemm_plan.hip cfg_applicable)
GEMM_TN = {1: (128, 64, 32, 0, 0), 2: (128, 128, 32, 0, 0), 3: (256, 128, 64, 0, 0), 7: (256, 128, 64, 0, 0), 8: (128, 64, 64, 0, 0),
           9: (128, 128, 32, 0, 0), 10: (128, 128, 64, 0, 0), 11: (128, 160, 64, 0, 1), 12: (128, 320, 64, 0, 1), 13: (256, 160, 64, 1, 1),
           15: (256, 128, 64, 1, 0), 16: (256, 160, 64, 1, 1)}
GEMM_FAMILIES = ("base", "shortcut", "f32_N4", "f32_N3", "geglu", "act1", "rowstats_ln", "gn_stats", "splitk2", "splitk3", "s2_p1", "s2_asym",
                 "ups", "1x1", "streamk_tails")


def gemm_cannot_run(tn, fam):
    """the reason (instance tn, family) cannot run - gemm_plan.hip's cfg_applicable - or None.  The GPU test asserts the library agrees both ways."""
    bm, bn, bk, persist, col160 = GEMM_TN[tn]
    if fam in ("f32_N4", "f32_N3"):
        if col160: return "the 160 / 320-column epilogue has no fp32 output"
        if persist: return "stream-K owners finish through the coalesced 16-bit epilogue"
    if fam == "geglu" and col160 and tn != 12: return "of the 160-column tiles only 128x320 holds whole GEGLU groups"
    if fam == "act1" and col160: return "the 160 / 320-column epilogue has no GELU"
    if fam == "rowstats_ln" and col160: return "the 160 / 320-column epilogue emits no row statistics"
    if fam == "gn_stats" and tn in (7, 13, 16): return "the warp-specialised instance has no statistics twin; the persistent 160-column ones leave them to the consumer"
    if fam in ("splitk2", "splitk3") and persist: return "a persistent stream-K instance splits K itself (force_splitk is not a plan of its own)"
    if fam == "streamk_tails" and not persist: return "the shared-tile shape is the stream-K instances' case"
    return None


def _conv64(x, w, **kw):
    return F.conv2d(x, w, None, **kw)


@functools.lru_cache(maxsize=None)
def gemm_eval(fam, elem, bk, fault=None):
    """conv / linear families; two-source input 96 | 32 (K-tile 32) or 64 | 64 (K-tile 64).  Returns (inputs, qty, spec): spec holds what the
    wrapper call needs (kwargs by name); inputs are NCHW fp64 tensors / vectors."""
    C0, C1 = (96, 32) if bk == 32 else (64, 64)
    Cin = C0 + C1
    B, H, W, N = 3, 10, 10, 200
    if fam == "streamk_tails": B, H, W, C0, C1, N = 3, 24, 24, 128, 64, 328; Cin = 192
    if fam == "gn_stats": H, W = 16, 16                      # rows per sample a multiple of the 256-row tiles
    if fam in ("f32_N4", "f32_N3"): N = 4 if fam == "f32_N4" else 3
    ks = 1 if fam in ("1x1", "geglu", "act1", "rowstats_ln") else 3
    if fam in ("geglu", "rowstats_ln"): N = 256               # (rowstats_ln: the consumer's K, a multiple of every K-tile)
    x0, x1 = inp((B, C0, H, W), 1, elem), inp((B, C1, H, W), 2, elem)
    x = torch.cat([x0, x1], 1)
    w = inp((N, Cin, ks, ks), 3, elem, 1 / math.sqrt(Cin * ks * ks))
    bias = (0.1 * seeded((N,), 4)).float().double()
    inputs = dict(x0=x0, x1=x1, w=w, bias=bias)
    spec = dict(ksize=ks, pad=ks // 2, N=N)
    f32 = False
    xi, stride, pad = x, 1, ks // 2
    if fam == "s2_p1": stride = 2; spec.update(stride=2, pad=1)
    if fam == "s2_asym": stride = 2; pad = 0; xi = F.pad(x, (0, 1, 0, 1)); spec.update(stride=2, pad=0)
    if fam == "ups": xi = F.interpolate(x, scale_factor=2.0, mode="nearest"); spec.update(ups=True)
    y = F.conv2d(xi, w, bias, stride=stride, padding=pad)
    y32 = F.conv2d(xi.float(), w.float(), bias.float(), stride=stride, padding=pad)
    OH, OW = y.shape[2:]
    qty = {}
    if fam in ("base", "splitk2", "splitk3", "streamk_tails", "gn_stats"):
        temb = seeded((B, N), 5).float().double(); r = inp((B, N, OH, OW), 6, elem)
        inputs.update(rowbias=temb, res=r)
        y = y + temb[:, :, None, None] + r
        if fam[:6] == "splitk": spec.update(force_splitk=int(fam[6]))
        if fam == "gn_stats": spec.update(force_splitk=1)                       # (a split-K plan leaves the statistics to the reduce pass: none emitted)
    if fam == "shortcut":
        s0, s1 = inp((B, C0, H, W), 7, elem), inp((B, C1, H, W), 8, elem)
        wsc = inp((N, Cin, 1, 1), 9, elem, 1 / math.sqrt(Cin))
        inputs.update(sc0=s0, sc1=s1, wsc=wsc)
        y = y + F.conv2d(torch.cat([s0, s1], 1), wsc)
    if fam in ("f32_N4", "f32_N3"):
        f32 = True; spec.update(out_f32=True)
    if fam == "geglu":
        a, g = y.chunk(2, dim=1); y = a * F.gelu(g); spec.update(geglu=True)
    if fam == "act1":
        r = inp((B, N, OH, OW), 6, elem); inputs.update(res=r)
        y = F.gelu(y) + r; spec.update(act=1)
    if fam == "rowstats_ln":
        # producer: h = x W^T + b (rounded, with per-row (sum, sumsq) of the rounded row); consumer: LayerNorm(h) folded into a second linear
        hq = rnd(y, elem)                                                        # [B,N,H,W]: rows are pixels, N = 256 channels = the consumer's K
        gam = (1.0 + 0.2 * seeded((N,), 10)).double(); bet = (0.2 * seeded((N,), 11)).double()
        N2 = 200                                                                 # the consumer's width: an N tail for every column tile
        w2 = inp((N2, N), 12, elem, 1 / math.sqrt(N))
        wf = rnd(w2 * gam[None, :], elem); c1 = wf.sum(1).float().double(); c2 = (w2 * bet[None, :]).sum(1).float().double()
        inputs.update(wf=wf, c1=c1, c2=c2)
        def consumer(hrows):                                                     # hrows [M][N]
            mean = hrows.mean(1, keepdim=True); var = (hrows * hrows).mean(1, keepdim=True) - mean * mean
            return (var.clamp_min(0) + 1e-5).rsqrt() * (hrows @ wf.t() - mean * c1[None, :]) + c2[None, :]
        rows = lambda t: nhwc(t).reshape(-1, t.shape[1])
        z = consumer(rows(hq)); zm = rnd(z, elem)                                 # the consumer is its own launch: its input is the stored h
        qty["z"] = q16(z.view(B, OH, OW, N2), zm.view(B, OH, OW, N2), TOL if elem == "fp16" else TOL_HALO_GN, [(0, 1, 2), 3], True, elem)
        spec.update(rowstats=True)
        # the row statistics are sums of the ROUNDED outputs: compared with the GPU output's own sums (the test), like gn_stats
    if f32:
        qty["y"] = q32(nhwc(y), nhwc(y32), [(0, 1, 2), 3])
    else:
        ym = y
        if fault == "bias_dropped_on_tail":                    # the last 8-channel group of the N tail without its bias
            ym = y.clone(); ym[:, -8:] -= bias[-8:].view(1, -1, 1, 1)
        qty["y"] = q16(nhwc(y), rnd(nhwc(ym), elem), TOL, [(0, 1, 2), 3], True, elem)
    return inputs, qty, spec


# ---------------------------------------------------------------------------------------------- phase-decomposed upsampler
UPS2X_CASE = (2, 6, 10, 64, 72)


def ups2x_eval(elem, fault=None):
    B, H, W, Cin, N = UPS2X_CASE
    x = inp((B, Cin, H, W), 1, elem)
    g = torch.Generator().manual_seed(7)
    w = (torch.randint(-4, 5, (N, Cin, 3, 3), generator=g).float() / 64.0).double()      # tap sums exact in both 16-bit elements
    bias = (0.1 * seeded((N,), 3)).float().double()
    y = F.conv2d(F.interpolate(x, scale_factor=2.0, mode="nearest"), w, bias, padding=1)
    mod = rnd(y, elem)
    if fault == "phase_swapped_on_right_border":               # the last output column computed with the other horizontal phase's taps
        mod = mod.clone(); mod[:, :, :, -1] = mod[:, :, :, -2]
    return dict(x=x, w=w, bias=bias), {"y": q16(nhwc(y), nhwc(mod), TOL, [(0, 1, 2), 3], True, elem)}


# ---------------------------------------------------------------------------------------------- halo conv
HALO_SHAPES = [(8, 32), (16, 16), (16, 32), (32, 32)]          # one tile of either geometry; 2 and 4 tiles
HALO_N = (160, 128)
HALO_VARIANTS = ("plain", "gn_silu", "gn_shortcut", "gn_res_temb")
HALO_C = (192, 128)                                            # 32 groups of 10: group 19 straddles the sources


@functools.lru_cache(maxsize=None)
def halo_eval(shape, N, variant, elem, fault=None):
    H, W = shape
    B, (C0, C1) = 1, HALO_C
    Cin = C0 + C1
    x0 = rnd(seeded((B, C0, H, W), 1) * 1.5 + 0.3, elem); x1 = rnd(seeded((B, C1, H, W), 2) * 0.5 - 1.0, elem)
    x = torch.cat([x0, x1], 1)
    w = inp((N, Cin, 3, 3), 3, elem, 1 / math.sqrt(9 * Cin)); bias = (0.1 * seeded((N,), 4)).float().double()
    g = (1 + 0.1 * seeded((Cin,), 10)).double(); be = (0.1 * seeded((Cin,), 11)).double()
    inputs = dict(x0=x0, x1=x1, w=w, bias=bias, gamma=g, beta=be)
    gn = variant != "plain"
    h = hm = x
    if gn:
        h = F.silu(F.group_norm(x, 32, g, be, 1e-5)); hm = rnd(h, elem)        # the normalised tensor is rounded once (the staged tile)
    y = F.conv2d(h, w, bias, padding=1)
    if fault == "bottom_pad_normalised" and gn:                # the zero padding below the image replaced by the normalised value of zero
        xg = x.reshape(B, 32, -1); mean = xg.mean(-1); rstd = (xg.var(-1, unbiased=False) + 1e-5).rsqrt()
        a = rstd.repeat_interleave(Cin // 32, 1) * g; s = be - mean.repeat_interleave(Cin // 32, 1) * a
        hp = F.pad(hm, (1, 1, 1, 1)); hp[:, :, -1, 1:-1] = rnd(F.silu(s), elem)[:, :, None]
        ym = F.conv2d(hp, w, bias)
    else:
        ym = F.conv2d(hm, w, bias, padding=1)
    if variant == "gn_shortcut":
        s0, s1 = inp((B, C0, H, W), 7, elem), inp((B, C1, H, W), 8, elem); wsc = inp((N, Cin, 1, 1), 9, elem, 1 / math.sqrt(Cin))
        inputs.update(sc0=s0, sc1=s1, wsc=wsc)
        sc = F.conv2d(torch.cat([s0, s1], 1), wsc); y = y + sc; ym = ym + sc
    if variant == "gn_res_temb":
        temb = seeded((B, N), 5).float().double(); r = inp((B, N, H, W), 6, elem)
        inputs.update(rowbias=temb, res=r)
        y = y + temb[:, :, None, None] + r; ym = ym + temb[:, :, None, None] + r
    # the whole-tensor bound is taken against test_ops_gpu.py's oracle (_halo_ref: the normalised tensor rounded once), the slices against fp64
    mod = rnd(nhwc(ym), elem)
    whole = mod if fault is None else halo_eval(shape, N, variant, elem)[1]["y"].model
    return inputs, {"y": Q(nhwc(y), mod, "16", TOL_HALO_GN if gn else TOL, [(0, 1, 2), 3], whole)}


# ---------------------------------------------------------------------------------------------- transformer chains (C = 320)
XF_M = (64, 128, 320)
XF_MODES = ("0", "1", "2", "2gn")
XF_C = 320


def _fold(w, gamma, beta, elem, bias=None):
    wf = rnd(w * gamma[None, :], elem)
    c2 = (w * beta[None, :]).sum(1)
    return wf, wf.sum(1).float().double(), (c2 if bias is None else c2 + bias).float().double()


def _rows(h, fault):
    mean = h.mean(1, keepdim=True)
    rstd = ((h * h).mean(1, keepdim=True) - mean * mean).clamp_min(0).add(1e-5).rsqrt()
    if fault == "stats_from_row_plus_32":                      # row 5 takes (mean, rstd) of row 37: the other half of a wave's 32-row fragment group
        mean = mean.clone(); rstd = rstd.clone(); mean[5] = mean[37]; rstd[5] = rstd[37]
    return mean, rstd


@functools.lru_cache(maxsize=None)
def xf_eval(mode, M, elem, fault=None):
    C = XF_C
    off = 1.5 * seeded((M, 1), 30).double()                    # per-row offsets: the folded LayerNorm's mean term matters
    wo = inp((C, C), 14, elem, 1 / math.sqrt(C)); bo = (0.1 * seeded((C,), 15)).float().double()
    gamma = (1 + 0.2 * seeded((C,), 18)).double(); beta = (0.2 * seeded((C,), 19)).double()
    fb = elem == "fp16"
    tol_y = TOL if fb else (TOL_CHAIN_Y1 if mode in ("1", "2gn") else TOL_HALO_GN)
    tol_h = TOL if (fb or mode != "2gn") else TOL_CHAIN_Y1
    inputs = dict(wo=wo, bo=bo)
    if mode in ("0", "1"):
        a = inp((M, C), 11, elem); h0 = rnd(seeded((M, C), 12).double() + off, elem)
        inputs.update(a=a, res=h0)
        h = a @ wo.t() + bo + h0
    else:
        if mode == "2gn":
            HW = 64; Bn = M // HW
            x = rnd(seeded((Bn, HW, C), 41, 1.5) + seeded((1, 1, C), 42, 2.0), elem)
            gg = (1 + 0.3 * seeded((C,), 48)).double(); gb = (0.3 * seeded((C,), 49)).double()
            n = F.group_norm(x.permute(0, 2, 1), 32, gg, gb, 1e-6).permute(0, 2, 1).reshape(M, C)
            inputs.update(x=x.reshape(M, C), gg=gg, gb=gb, HW=HW)
            a, a_m = n, rnd(n, elem)                           # the normalised operand is materialised in the 16-bit element
        else:
            a = a_m = rnd(seeded((M, C), 31).double() + off, elem); inputs.update(x=a)
        h = a @ wo.t() + bo
    if mode in ("0", "1"):
        hm = rnd(h, elem)
    else:
        hm = rnd(a_m @ wo.t() + bo, elem)
    mean, rstd = _rows(h, None); mm, rm = _rows(hm, fault)
    if mode == "0":
        w1 = inp((C, C), 5, elem, 1 / math.sqrt(C)); wf, c1, c2 = _fold(w1, gamma, beta, elem)
    elif mode == "1":
        w1 = inp((8 * C, C), 16, elem, 1 / math.sqrt(C)); b1 = (0.1 * seeded((8 * C,), 17)).float().double()
        wf, c1, c2 = _fold(w1, gamma, beta, elem, b1)
    else:
        w1 = inp((3 * C, C), 34, elem, 1 / math.sqrt(C)); wf, c1, c2 = _fold(w1, gamma, beta, elem)
    inputs.update(wf=wf, c1=c1, c2=c2)
    u = rstd * (h @ wf.t() - mean * c1) + c2
    um = rm * (hm @ wf.t() - mm * c1) + c2
    if mode == "1":
        w2 = inp((C, 4 * C), 20, elem, 1 / math.sqrt(4 * C)); b2 = (0.1 * seeded((C,), 21)).float().double()
        wp = inp((C, C), 22, elem, 1 / math.sqrt(C)); bp = (0.1 * seeded((C,), 23)).float().double()
        xres = inp((M, C), 13, elem)
        inputs.update(w2=w2, b2=b2, wp=wp, bp=bp, xres=xres)
        val, gate = u.chunk(2, -1); y = ((val * F.gelu(gate)) @ w2.t() + b2 + h) @ wp.t() + bp + xres
        val, gate = um.chunk(2, -1); t = rnd(val * F.gelu(gate), elem)
        ym = rnd(rnd(t @ w2.t() + b2 + hm, elem) @ wp.t() + bp + xres, elem)
    else:
        y, ym = u, rnd(um, elem)
    # the whole-tensor bounds are taken against test_ops_gpu.py's oracles (h, t and y rounded once each), the slices against fp64
    wy = ym if fault is None else xf_eval(mode, M, elem)[1]["y"].model
    return inputs, {"h": Q(h, hm, "16", tol_h, [0, 1], hm), "y": Q(y, ym, "16", tol_y, [0, 1], wy)}


# ---------------------------------------------------------------------------------------------- small ones
# name, B, H, W, Cin, N, gn, force_S : the two smallest of test_ops_gpu.py's SKINNY_CASES
SKINNY_SMALL = [("gn_b1_8x8_S2", 1, 8, 8, 320, 64, True, 2), ("plain_b4_8x8_S1", 4, 8, 8, 256, 64, False, 1)]


def skinny_eval(case, elem, fault=None):
    name, B, H, W, Cin, N, gn, fS = case
    x = rnd(seeded((B, Cin, H, W), 1) * 1.5 + 0.3, elem)
    w = inp((N, Cin, 3, 3), 3, elem, 1 / math.sqrt(9 * Cin)); bias = (0.1 * seeded((N,), 4)).float().double()
    temb = seeded((B, N), 5).float().double(); r = inp((B, N, H, W), 6, elem)
    g = (1 + 0.1 * seeded((Cin,), 10)).double(); be = (0.1 * seeded((Cin,), 11)).double()
    h = hm = x
    if gn:
        h = F.silu(F.group_norm(x, 32, g, be, 1e-5)); hm = rnd(h, elem)
    y = F.conv2d(h, w, bias, padding=1) + temb[:, :, None, None] + r
    ym = F.conv2d(hm, w, bias, padding=1) + temb[:, :, None, None] + r
    ym0 = ym                                                  # (the whole-tensor bound: against test_ops_gpu.py's _halo_ref, as the halo conv)
    if fault == "last_pixel_tap":                              # the last pixel's out-of-image taps not zeroed
        ym = ym.clone(); ym[-1, :, -1, -1] += (w[:, :, 2, 2] @ hm[-1, :, 0, 0])
    return dict(x=x, w=w, bias=bias, rowbias=temb, res=r, gamma=g, beta=be), \
        {"y": Q(nhwc(y), rnd(nhwc(ym), elem), "16", TOL_HALO_GN if gn else TOL, [(0, 1, 2), 3], rnd(nhwc(ym0), elem))}


LS_CASES = [(1, 1280), (3, 1280), (1, 8), (3, 8)]             # B, N of linear_small behind the 320-wide time embedding
LS_T = (981, 1, 500)


def ls_eval(case, elem, fault=None):
    B, N = case
    half = 160
    freq = torch.exp(-math.log(10000) * torch.arange(half, dtype=torch.float32) / half)
    t = torch.tensor(LS_T[:B], dtype=torch.int64)
    arg32 = t[:, None].float() * freq[None]                    # the kernel's argument is the float32 product
    arg = arg32.double()
    emb = torch.cat([torch.cos(arg), torch.sin(arg)], -1); emb32 = torch.cat([torch.cos(arg32), torch.sin(arg32)], -1)
    w = inp((N, 320), 1, elem, 1 / math.sqrt(320)); bias = (0.1 * seeded((N,), 2)).float().double()
    # linear_small reads the embedding the kernel before it wrote (fp32): the reference starts from the float32 embedding
    e = emb32.double()
    y = F.silu(e) @ w.t() + bias
    y32 = F.linear(F.silu(emb32), w.float(), bias.float())
    if fault == "third_sample":
        y32 = y32.clone(); y32[B - 1] = y32[0]
    return dict(t=t, freq=freq, w=w, bias=bias, emb32=emb32), {"emb": q32(emb, emb32, [0]), "y": q32(y, y32, [0, 1])}


IM2COL_CASES = [(2, 6, 10, 9, 1, 128), (2, 6, 10, 9, 2, 128), (1, 5, 7, 4, 1, 64)]       # B, H, W, C, stride, Kpad : 9 C = 81 / 36 columns, then zeros


def im2col_eval(case, elem):
    B, H, W, C, st, Kpad = case
    x = inp((B, C, H, W), 1, elem)
    OH, OW = H // st, W // st
    cols = F.unfold(x, 3, padding=1, stride=st)                # [B][C*9][L], channel-major
    L = cols.shape[-1]
    cols = cols.view(B, C, 9, L).permute(0, 3, 2, 1).reshape(B, L, 9 * C)[:, :OH * OW]      # tap-major, as the packed weights
    want = torch.zeros(B, OH * OW, Kpad, dtype=D); want[:, :, :9 * C] = cols
    return dict(x=x), {"col": qx(want.view(B, OH, OW, Kpad))}


# ---------------------------------------------------------------------------------------------- the table
def all_cases():
    out = []
    for e in ("bf16", "fp16"):
        for c in ATTN64_CASES + BAL_CASES: out.append((f"attn64/{c[0]}/{e}", lambda c=c, e=e: attn64_eval(c, e)))
        for c in WIDE_CASES: out.append((f"wide/d{c[0]}_S{c[1]}/{e}", lambda c=c, e=e: wide_eval(c, e)))
        for c in GNF_CASES: out.append((f"gnf/{c[0]}/{e}", lambda c=c, e=e: gnf_eval(c, e)))
        for c in LNF_CASES: out.append((f"lnf/{c[0]}x{c[1]}/{e}", lambda c=c, e=e: lnf_eval(c, e)))
        for fam in GEMM_FAMILIES:
            for bk in ((64,) if fam == "streamk_tails" else (32, 64)):
                out.append((f"gemm/{fam}/k{bk}/{e}", lambda fam=fam, bk=bk, e=e: gemm_eval(fam, e, bk)[:2]))
        out.append((f"ups2x/{e}", lambda e=e: ups2x_eval(e)))
        for sh in HALO_SHAPES:
            for n in HALO_N:
                for v in HALO_VARIANTS: out.append((f"halo/{sh[0]}x{sh[1]}_n{n}_{v}/{e}", lambda sh=sh, n=n, v=v, e=e: halo_eval(sh, n, v, e)))
        for m in XF_MODES:
            for M in XF_M: out.append((f"xf/mode{m}_M{M}/{e}", lambda m=m, M=M, e=e: xf_eval(m, M, e)))
        for c in SKINNY_SMALL: out.append((f"skinny/{c[0]}/{e}", lambda c=c, e=e: skinny_eval(c, e)))
        for c in LS_CASES: out.append((f"ls/b{c[0]}_n{c[1]}/{e}", lambda c=c, e=e: ls_eval(c, e)))
        for c in IM2COL_CASES: out.append((f"im2col/{'x'.join(map(str, c))}/{e}", lambda c=c, e=e: im2col_eval(c, e)))
    return out


def measure_all():
    return {f"{key}:{name}": measure(q) for key, thunk in all_cases() for name, q in thunk()[1].items()}


def bounds(key, qty):
    return {name: tol_of(q, FLOORS[f"{key}:{name}"]) for name, q in qty.items()}


try:
    from fwd_floors import FLOORS    # "family/case/element:quantity" -> (whole, worst slice) figure of the restatement
except ImportError:                  # only while the table is being regenerated
    FLOORS = {}

if __name__ == "__main__":                                     # regenerate fwd_floors.py's table
    print('"""Measured figures (whole tensor, worst slice) of the restatements of fwd_refs.py against fp64, on the CPU: the per-slice bounds of\nthe forward layout tests are computed from them (fwd_refs.bounds); test_fwd_refs_host.py measures them again.  Regenerate: python tests/fwd_refs.py"""')
    print("FLOORS = {")
    for k, (w, s) in measure_all().items():
        print(f'    "{k}": ({w:.3e}, {s:.3e}),')
    print("}")
