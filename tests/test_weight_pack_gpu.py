"""The weight pack / fold kernels by themselves: elementwise.hip's packs (pack_conv_w, pack_conv_w_t, pack_rows, pack_rows_t, pack_geglu_bias,
cast_pad_rows), gemm.hip's dmx_ups_phase_weights_kernel and dmx_ln_fold_kernel, and the agreement of the three separately written index
maps of the parameter layouts (load_param's packs, dmx_master_pack_kernel, dmx_grad_unpack_kernel) on the tiny UNet.  Until now they were
helpers of other kernels' tests or ran behind model tolerances.

Every expectation is an index restatement written from the layout comments (taps-major conv rows, the 32 / 32 GEGLU interleave, the flipped
channel-transposed data-gradient filter, the phase table of the upsample conv), not from the kernels' loops; rounding is torch's
`.to(bfloat16 | float16)`; everything that only moves or rounds data is compared bit for bit.  Outputs are sentinel-filled and larger than
what is written (padded ldk / koff / ldo, rows behind the last): the guards must be intact and every output element written.  Both builds."""
import pytest
import torch

from test_train_small_gpu import call, refused, untouched
from util import SENTINEL_BITS, assert_guard_intact, seeded

pytestmark = pytest.mark.gpu
ELEMS = ["bf16", "fp16"]
DT = {"bf16": torch.bfloat16, "fp16": torch.float16}
U = 2.0 ** -24
GUARD = 64


@pytest.fixture(scope="module")
def cuda():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda")


def flat_poisoned(n, dtype, dev):
    """a flat sentinel-filled buffer of n elements between two guard bands; -> (buffer, the n-element span)"""
    it, sb = SENTINEL_BITS[dtype]
    buf = torch.full((n + 2 * GUARD,), sb, dtype=it, device=dev).view(dtype)
    return buf, buf[GUARD:GUARD + n]


def rows_view(span, rows, ld, col0, cols):
    return span.as_strided((rows, cols), (ld, 1), span.storage_offset() + col0)


def bits(t):
    return t.detach().cpu().contiguous().view(torch.int16 if t.element_size() == 2 else torch.int32)


def assert_bits(got, want, key):
    g, w = bits(got), bits(want)
    assert g.shape == w.shape and torch.equal(g, w), f"{key}: {int((g != w).sum())} of {w.numel()} elements differ"


def weights(shape, seed):
    return seeded(shape, seed) * 0.37 + 0.011           # nothing exactly representable in 16 bits: every element is rounded


# ---------------------------------------------------------------------------------------------- conv packs
# (Cout, Cin, ks, ldk, koff); the last is above the 8192-block grid cap (2 211 840 elements > 2 097 152): the grid-stride loop does the rest
CONV_CASES = [(3, 5, 3, 64, 7), (6, 3, 16, 768, 0), (8, 8, 1, 24, 16), (256, 960, 3, 8704, 8)]


def conv_rows(w):
    """out[n][tap * Cin + ci], tap = ky * ks + kx"""
    return w.permute(0, 2, 3, 1).reshape(w.shape[0], -1)


def conv_rows_t(w):
    """the data-gradient filter: spatially flipped, channel roles swapped: out[ci][tap * Cout + n] of flip(w)"""
    return w.flip(2, 3).permute(1, 2, 3, 0).reshape(w.shape[1], -1)


@pytest.mark.parametrize("elem", ELEMS)
@pytest.mark.parametrize("case", CONV_CASES, ids=[f"{c[0]}x{c[1]}x{c[2]}_ld{c[3]}_k{c[4]}" for c in CONV_CASES])
def test_pack_conv_weight(cuda, case, elem):
    from diffute_amd import ops
    Cout, Cin, ks, ldk, koff = case
    dt = DT[elem]
    w = weights((Cout, Cin, ks, ks), 11)
    wd = w.to(cuda)
    with ops.element_type(elem):
        K = ks * ks * Cin
        buf, span = flat_poisoned(Cout * ldk, dt, cuda)
        call("dmx_pack_conv_weight", wd, span, Cout, Cin, ks, ldk, koff)
        Kt = ks * ks * Cout
        ldt = ldk if ldk >= koff + Kt else koff + Kt + 8                      # the transposed rows are ks * ks * Cout long
        buft, spant = flat_poisoned(Cin * ldt, dt, cuda)
        call("dmx_pack_conv_weight_t", wd, spant, Cout, Cin, ks, ldt, koff)
        torch.cuda.synchronize()
    out = rows_view(span, Cout, ldk, koff, K); outt = rows_view(spant, Cin, ldt, koff, Kt)
    assert_guard_intact(buf, out, name=f"pack_conv_weight/{case}/{elem}")
    assert_guard_intact(buft, outt, name=f"pack_conv_weight_t/{case}/{elem}")
    assert_bits(out, conv_rows(w).to(dt), f"pack_conv_weight/{case}/{elem}")
    assert_bits(outt, conv_rows_t(w).to(dt), f"pack_conv_weight_t/{case}/{elem}")


@pytest.mark.parametrize("elem", ELEMS)
def test_pack_conv_plus_shortcut_row(cuda, elem):
    """one GEMM row = the 3x3 taps, then the 1x1 shortcut's channels at koff = 9 * Cin (two calls into the same rows, as the resnets' conv2 +
    conv_shortcut are loaded); the K padding behind them is not written"""
    from diffute_amd import ops
    Cout, Cin, Csc, ldk = 8, 5, 3, 64
    dt = DT[elem]
    w, ws = weights((Cout, Cin, 3, 3), 12), weights((Cout, Csc, 1, 1), 13)
    with ops.element_type(elem):
        buf, span = flat_poisoned(Cout * ldk, dt, cuda)
        call("dmx_pack_conv_weight", w.to(cuda), span, Cout, Cin, 3, ldk, 0)
        call("dmx_pack_conv_weight", ws.to(cuda), span, Cout, Csc, 1, ldk, 9 * Cin)
        torch.cuda.synchronize()
    out = rows_view(span, Cout, ldk, 0, 9 * Cin + Csc)
    assert_guard_intact(buf, out, name=f"conv+shortcut/{elem}")
    assert_bits(out, torch.cat([conv_rows(w), ws[:, :, 0, 0]], 1).to(dt), f"conv+shortcut/{elem}")


# ---------------------------------------------------------------------------------------------- linear packs
def geglu_rows(w):
    """[a0..a31 | b0..b31 | a32..a63 | b32..b63 | ...]: 32-row groups of the value half a = w[:R/2] and the gate half b = w[R/2:] in turn"""
    R = w.shape[0]
    return w.reshape(2, R // 64, 32, -1).transpose(0, 1).reshape(w.shape)


@pytest.mark.parametrize("elem", ELEMS)
@pytest.mark.parametrize("case", [(5, 7, 16, 0), (128, 40, 48, 1), (2560, 320, 328, 1)], ids=["5x7_ld16", "geglu128", "geglu2560"])
def test_pack_linear_weight(cuda, case, elem):
    from diffute_amd import ops
    rows, cols, ldo, geglu = case
    dt = DT[elem]
    w = weights((rows, cols), 14)
    with ops.element_type(elem):
        buf, span = flat_poisoned(rows * ldo, dt, cuda)
        call("dmx_pack_linear_weight", w.to(cuda), span, rows, cols, ldo, geglu)
        torch.cuda.synchronize()
    out = rows_view(span, rows, ldo, 0, cols)
    assert_guard_intact(buf, out, name=f"pack_linear_weight/{case}/{elem}")
    assert_bits(out, (geglu_rows(w) if geglu else w).to(dt), f"pack_linear_weight/{case}/{elem}")
    if geglu:                           # (the restatement is a permutation: every source row exactly once)
        assert sorted(geglu_rows(torch.arange(rows).float().reshape(rows, 1)).flatten().tolist()) == list(range(rows))


@pytest.mark.parametrize("elem", ELEMS)
@pytest.mark.parametrize("case", [(33, 65, 40), (32, 32, 32), (1, 40, 8)], ids=["33x65", "32x32", "1x40_ld8"])
def test_pack_linear_weight_t(cuda, case, elem):
    from diffute_amd import ops
    rows, cols, ldo = case
    dt = DT[elem]
    w = weights((rows, cols), 15)
    with ops.element_type(elem):
        buf, span = flat_poisoned(cols * ldo, dt, cuda)
        call("dmx_pack_linear_weight_t", w.to(cuda), span, rows, cols, ldo)
        torch.cuda.synchronize()
    out = rows_view(span, cols, ldo, 0, rows)
    assert_guard_intact(buf, out, name=f"pack_linear_weight_t/{case}/{elem}")
    assert_bits(out, w.t().contiguous().to(dt), f"pack_linear_weight_t/{case}/{elem}")


@pytest.mark.parametrize("elem", ELEMS)
@pytest.mark.parametrize("n", [128, 2560])
def test_pack_geglu_bias(cuda, n, elem):
    from diffute_amd import ops
    b = weights((n,), 16)
    with ops.element_type(elem):
        buf, span = flat_poisoned(n, torch.float32, cuda)
        call("dmx_pack_geglu_bias", b.to(cuda), span, n)
        torch.cuda.synchronize()
    assert_guard_intact(buf, span, name=f"pack_geglu_bias/{n}/{elem}")
    assert_bits(span, geglu_rows(b.reshape(n, 1)).reshape(n), f"pack_geglu_bias/{n}/{elem}")


@pytest.mark.parametrize("elem", ELEMS)
def test_geglu_packing_refuses_partial_groups(cuda, elem):
    """rows % 64 != 0: the interleave is no permutation (rows = 96 would read rows 48..63 twice and never rows 80..95) - refused, nothing written"""
    from diffute_amd import ops
    dt = DT[elem]
    w = weights((96, 8), 17).to(cuda)
    with ops.element_type(elem):
        buf, span = flat_poisoned(96 * 8, dt, cuda)
        assert "64" in refused("dmx_pack_linear_weight", w, span, 96, 8, 8, 1)
        bufb, spanb = flat_poisoned(96, torch.float32, cuda)
        assert "64" in refused("dmx_pack_geglu_bias", w, spanb, 96)
        torch.cuda.synchronize()
        assert untouched(buf) and untouched(bufb)
        call("dmx_pack_linear_weight", w, span, 96, 8, 8, 0)              # the plain pack takes any row count
        torch.cuda.synchronize()
    assert_bits(span.reshape(96, 8), w.cpu().to(dt), f"pack_linear_weight/96 rows, no geglu/{elem}")


# ---------------------------------------------------------------------------------------------- context cast
@pytest.mark.parametrize("elem", ELEMS)
@pytest.mark.parametrize("in16", [0, 1], ids=["from_fp32", "from_16"])
@pytest.mark.parametrize("case", [(1, 3, 8, 5), (2, 577, 640, 1024)], ids=["1x3to8x5", "2x577to640x1024"])      # the second: 1 310 720 elements > 4096 blocks x 256
def test_cast_pad_rows(cuda, case, in16, elem):
    from diffute_amd import ops
    B, S, Spad, C = case
    dt = DT[elem]
    x = weights((B, S, C), 18)
    src = x.to(dt) if in16 else x
    with ops.element_type(elem):
        buf, span = flat_poisoned(B * Spad * C, dt, cuda)
        call("dmx_test_cast_pad_rows", src.to(cuda), in16, span, B, S, Spad, C)
        torch.cuda.synchronize()
    assert_guard_intact(buf, span, name=f"cast_pad_rows/{case}/{elem}")
    want = torch.zeros(B, Spad, C, dtype=dt); want[:, :S] = x.to(dt)
    assert_bits(span.reshape(B, Spad, C), want, f"cast_pad_rows/{case}/in16={in16}/{elem}")
    assert not bits(span.reshape(B, Spad, C)[:, S:]).any(), "rows >= S must be zero"


# ---------------------------------------------------------------------------------------------- upsample phase weights
# conv3x3(nearest_x2(x)) at output parity pa only sees two source rows; the taps that land on the same one: pa = 0: {ky=0} | {ky=1,2}, pa = 1: {ky=0,1} | {ky=2}
PHASE_TAPS = {0: ([0], [1, 2]), 1: ([0, 1], [2])}


@pytest.mark.parametrize("elem", ELEMS)
@pytest.mark.parametrize("case", [(8, 8, 72), (24, 16, 160)], ids=["8x8_ld72", "24x16_ld160"])
def test_pack_ups_phase_weights(cuda, case, elem):
    from diffute_amd import ops
    N, Cin, ldw3 = case
    dt = DT[elem]
    w3 = weights((N, ldw3), 19).to(dt)                       # [n][(ky * 3 + kx) * Cin + ci], junk behind 9 * Cin
    with ops.element_type(elem):
        buf, span = flat_poisoned(4 * N * 4 * Cin, dt, cuda)
        call("dmx_pack_ups_phase_weights", w3.to(cuda), ldw3, span, N, Cin)
        torch.cuda.synchronize()
    assert_guard_intact(buf, span, name=f"ups_phase_weights/{case}/{elem}")
    got = span.reshape(4, N, 4, Cin)
    taps = w3[:, :9 * Cin].float().reshape(N, 3, 3, Cin)
    for pa in (0, 1):
        for pb in (0, 1):
            for ty in (0, 1):
                for tx in (0, 1):
                    acc = torch.zeros(N, Cin)
                    for ky in PHASE_TAPS[pa][ty]:                  # fp32 sum of the 16-bit taps, ky then kx, one rounding at the end
                        for kx in PHASE_TAPS[pb][tx]:
                            acc = acc + taps[:, ky, kx]
                    assert_bits(got[2 * pa + pb, :, 2 * ty + tx], acc.to(dt), f"ups_phase_weights/{case}/{elem}: phase ({pa},{pb}) tap ({ty},{tx})")


# ---------------------------------------------------------------------------------------------- folded LayerNorm weights
@pytest.mark.parametrize("elem", ELEMS)
@pytest.mark.parametrize("with_bias", [0, 1], ids=["nobias", "bias"])
@pytest.mark.parametrize("case", [(5, 8), (4, 512), (7, 520), (960, 320)], ids=lambda c: f"{c[0]}x{c[1]}")
def test_ln_fold(cuda, case, with_bias, elem):
    """W' = round16(W * gamma) bit for bit; c1 = the row sums of the ROUNDED W' and c2 = W beta (+ bias) against fp64 within
    (K / 8 + 7) u sum |terms|: a per-lane chain of up to K / 512 * 8 adds, 6 shuffle adds, 1 - the bound is far below the difference between
    the row sums of the rounded and the unrounded W * gamma, which is asserted to be visible"""
    from diffute_amd import ops
    N, K = case
    dt = DT[elem]
    key = f"ln_fold/{N}x{K}/bias={with_bias}/{elem}"
    w = weights((N, K), 20).to(dt)
    gamma = 1.0 + 0.3 * seeded((K,), 21); beta = 0.2 * seeded((K,), 22); bias = 0.5 * seeded((N,), 23)
    extra = 3
    with ops.element_type(elem):
        bufw, spanw = flat_poisoned((N + extra) * K, dt, cuda)
        buf1, span1 = flat_poisoned(N + extra, torch.float32, cuda)
        buf2, span2 = flat_poisoned(N + extra, torch.float32, cuda)
        call("dmx_test_ln_fold", w.to(cuda), spanw, gamma.to(cuda), beta.to(cuda), bias.to(cuda) if with_bias else None, span1, span2, N, K)
        torch.cuda.synchronize()
    assert_guard_intact(bufw, spanw[:N * K], name=key + " W'")                   # rows n >= N of the longer outputs are untouched
    assert_guard_intact(buf1, span1[:N], name=key + " c1")
    assert_guard_intact(buf2, span2[:N], name=key + " c2")
    wf = w.float()
    wg = (wf * gamma).to(dt)                                                     # fp32 product, then the 16-bit rounding: the kernel's two roundings
    assert_bits(spanw[:N * K].reshape(N, K), wg, key + " W'")
    c = (K / 8 + 7) * U
    c1, c2 = span1[:N].cpu().double(), span2[:N].cpu().double()
    r1 = wg.double().sum(1); b1 = c * wg.double().abs().sum(1)
    terms = wf.double() * beta.double()
    r2 = terms.sum(1) + (bias.double() if with_bias else 0.0); b2 = c * (terms.abs().sum(1) + (bias.double().abs() if with_bias else 0.0))
    e1, e2 = ((c1 - r1).abs() / b1).max(), ((c2 - r2).abs() / b2).max()
    print(f"{key}: worst |error| / bound c1 {float(e1):.3f} c2 {float(e2):.3f}")
    assert float(e1) <= 1.0, f"{key}: c1 is {float(e1):.3f} x its bound"
    assert float(e2) <= 1.0, f"{key}: c2 is {float(e2):.3f} x its bound"
    unrounded = (wf.double() * gamma.double()).sum(1)
    assert bool(((c1 - unrounded).abs() > b1).any()), f"{key}: these inputs do not tell the sum of the rounded W' from the sum of W * gamma"


# ---------------------------------------------------------------------------------------------- three index maps, one layout
@pytest.mark.parametrize("elem", ELEMS)
def test_pack_import_export_agree_on_the_tiny_unet(cuda, elem):
    """load_param's packs (weights arena), master_import (packed fp32 arena) and grad_export (back to torch layouts) are three separately
    written index maps of the same layouts (conv taps-major with koff, GEGLU interleave, ld): export(import(x)) == x for every parameter, and
    the weights arena after a re-pack holds the rounded master at the element the optimizer's chunk table maps each arena element to"""
    from test_adamw_gpu import rig_for
    rig = rig_for(elem, cuda)
    u = rig.unet
    params = u._param_list()
    xs = [weights(tuple(p.shape), 100 + i).to(cuda) for i, p in enumerate(params)]
    arena = u._import_arena(xs)
    back = u._export_arena(arena, [torch.full_like(x, float("nan")) for x in xs])
    torch.cuda.synchronize()
    for k, x, b in zip(u._keys, xs, back):
        assert torch.equal(x.view(torch.int32), b.view(torch.int32)), f"{k}: grad_export(master_import(x)) != x"
    assert bool((arena[~rig.real] == 0).all()), "master_import wrote outside the elements it writes for all-ones parameters"
    u.mark_parameters_changed(); u._ensure_packed()                 # the AdamW tests of this session may have stepped this arena
    masters = rig.gather(u._import_arena(params))
    real = rig.gather(rig.real)
    torch.cuda.synchronize()
    got16 = u._arena.view(torch.int16)[rig.idx16]; want16 = masters[rig.is16].to(rig.dt).view(torch.int16)
    got32 = u._arena.view(torch.int32)[rig.idx32]; want32 = masters[~rig.is16].view(torch.int32)
    bad16 = (got16 != want16) & real[rig.is16]; bad32 = (got32 != want32) & real[~rig.is16]
    assert not bool(bad16.any()) and not bool(bad32.any()), f"{int(bad16.sum())} 16-bit / {int(bad32.sum())} fp32 weights differ from the rounded masters"
