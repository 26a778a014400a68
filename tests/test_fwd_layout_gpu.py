"""The forward kernels per slice, the way the executors call them: operands (and residuals) that are column slices of wider buffers of
finite junk, outputs written into poisoned buffers with guard bands (everything inside written, nothing outside), two runs bit-equal,
on both builds.  fwd_refs.py holds the cases, the fp64 references and the bounds: the whole-tensor figure test_ops_gpu.py states for the
kernel, and a per-slice bound (per query row / head, per channel / (sample, group), per row / column, per output pixel / channel) that is
the same figure or 3 x the rounding-point restatement's worst slice (fwd_floors.py); fp32 outputs 8 x torch float32's deviation from fp64.
Each check prints one line `key:quantity whole <error>/<bound> slice <error>/<bound>` (pytest -rA shows them)."""
import pytest
import torch

import fwd_refs as R
from test_train_layout_gpu import bits, check as _check, host, wide
from util import assert_guard_intact, poisoned, seeded

pytestmark = pytest.mark.gpu
ELEMS = ["bf16", "fp16"]


def check(key, qty, got):
    _check(key, qty, got, R.bounds(key, qty))


def same(a, b, what):
    assert torch.equal(bits(a), bits(b)), f"{what}: differs between two runs"


def v4(o, B, H, W):
    """the [B*H*W][C] rows of a guarded buffer as NHWC (explicit strides: a view would give size-1 dimensions the dense stride)"""
    ld = o.stride(0)
    return o.as_strided((B, H, W, o.shape[1]), (H * W * ld, W * ld, ld, 1))


def f32(t, dev):
    return t.float().to(dev).contiguous()


# ---------------------------------------------------------------------------------------------- d = 64 attention
def _kv(inputs, name, pad):
    return inputs[name] if inputs[pad] is None else torch.cat([inputs[name], inputs[pad]], 1)


@pytest.mark.parametrize("elem", ELEMS)
@pytest.mark.parametrize("case", R.ATTN64_CASES, ids=[c[0] for c in R.ATTN64_CASES])
def test_attention_vt_form(cuda, case, elem):
    from diffute_amd import ops
    name, B, H, Sq, Skv, kvr = case
    C = H * 64
    inputs, qty = R.attn64_eval(case, elem)
    dt = R.ELEMS[elem]
    with ops.element_type(elem):
        q = wide(inputs["q"].reshape(B * Sq, C), dt, cuda)
        k = wide(_kv(inputs, "k", "kpad").reshape(B * kvr, C), dt, cuda, pad=16, seed=96)
        vt = wide(_kv(inputs, "v", "vpad").reshape(B * kvr, C).t().contiguous(), dt, cuda, seed=95)      # [C][B * kv_rows]: columns [Skv, kv_rows) of a sample hold junk
        obuf, o = poisoned((B * Sq, C), dt, cuda)
        ops.attention(q, k, vt, B, H, Sq, Skv, R.ATTN_SCALE, kv_rows=kvr, skv_stride=kvr, out=o)
        o2 = ops.attention(q, k, vt, B, H, Sq, Skv, R.ATTN_SCALE, kv_rows=kvr, skv_stride=kvr)
        torch.cuda.synchronize()
    key = f"attn64/{name}/{elem}"
    assert_guard_intact(obuf, o, name=key); same(o, o2, key)
    check(key, qty, {"o": o})


@pytest.mark.parametrize("elem", ELEMS)
@pytest.mark.parametrize("case", R.BAL_CASES, ids=[c[0] for c in R.BAL_CASES])
def test_attention_balanced_schedule_per_row(cuda, case, elem):
    from diffute_amd import ops
    name, B, H, Sq, Skv, kvr = case
    C = H * 64
    inputs, qty = R.attn64_eval(case, elem)
    dt = R.ELEMS[elem]
    with ops.element_type(elem):
        lib = ops.lib()
        q = wide(inputs["q"].reshape(B * Sq, C), dt, cuda)
        kv = torch.cat([_kv(inputs, "k", "kpad"), _kv(inputs, "v", "vpad")], -1).reshape(B * kvr, 2 * C).to(cuda).to(dt)
        obuf, o = poisoned((B * Sq, C), dt, cuda)
        old = lib.dmx_set_attn_balanced(2)
        try:
            assert lib.dmx_attention_fwd_v_balanced_workspace_bytes(B, H, Sq, Skv) > 0, "the balanced schedule does not take this shape"
            assert ops.attention_v_balanced(q, kv[:, :C], kv[:, C:], B, H, Sq, Skv, R.ATTN_SCALE, kv_rows=kvr, out=o) is not None
            o2 = ops.attention_v_balanced(q, kv[:, :C], kv[:, C:], B, H, Sq, Skv, R.ATTN_SCALE, kv_rows=kvr)
        finally:
            lib.dmx_set_attn_balanced(old)
        torch.cuda.synchronize()
    key = f"attn64/{name}/{elem}"
    assert_guard_intact(obuf, o, name=key); same(o, o2, key)
    check(key, qty, {"o": o})


@pytest.mark.parametrize("elem", ELEMS)
@pytest.mark.parametrize("case", R.WIDE_CASES, ids=[f"d{c[0]}_S{c[1]}" for c in R.WIDE_CASES])
def test_attention_wide_per_row(cuda, case, elem):
    from diffute_amd import ops
    Dh, S = case
    B = R.WIDE_B
    inputs, qty = R.wide_eval(case, elem)
    dt = R.ELEMS[elem]
    with ops.element_type(elem):
        qkv = (seeded((B * S, 3 * Dh + 16), 99) * 3.0)
        for i, n in enumerate("qkv"):
            qkv[:, 8 + i * Dh:8 + (i + 1) * Dh] = inputs[n].reshape(B * S, Dh)
        qkv = qkv.to(cuda).to(dt)
        q, k, v = (qkv[:, 8 + i * Dh:8 + (i + 1) * Dh] for i in range(3))
        obuf, o = poisoned((B * S, Dh), dt, cuda)
        ops.attention_wide(q, k, v, B, S, S, Dh, Dh ** -0.5, out=o)
        o2 = ops.attention_wide(q, k, v, B, S, S, Dh, Dh ** -0.5)
        torch.cuda.synchronize()
    key = f"wide/d{Dh}_S{S}/{elem}"
    assert_guard_intact(obuf, o, name=key); same(o, o2, key)
    check(key, qty, {"o": o})


# ---------------------------------------------------------------------------------------------- GroupNorm / LayerNorm
@pytest.mark.parametrize("elem", ELEMS)
@pytest.mark.parametrize("case", R.GNF_CASES, ids=[c[0] for c in R.GNF_CASES])
def test_groupnorm_forward_layout(cuda, case, elem):
    from diffute_amd import ops
    name, B, H, W, C0, C1, G, silu, eps, cancel, path = case
    C = C0 + C1
    inputs, qty = R.gnf_eval(case, elem)
    dt = R.ELEMS[elem]
    key = f"gnf/{name}/{elem}"
    with ops.element_type(elem):
        xn = R.nhwc(inputs["x"])
        x0 = wide(xn[..., :C0], dt, cuda, pad=16, seed=92); x1 = wide(xn[..., C0:], dt, cuda, pad=40, seed=94)
        g, b = f32(inputs["gamma"], cuda), f32(inputs["beta"], cuda)
        ybuf, y = poisoned((B * H * W, C), dt, cuda)
        ops.groupnorm(x0, g, b, G, eps, silu, x1=x1, out=v4(y, B, H, W))
        y2 = ops.groupnorm(x0, g, b, G, eps, silu, x1=x1)
        if path == "producer":          # identity 1x1 convs as the producers of both sources: their outputs are the inputs, bit for bit
            srcs = []
            for x, c in ((x0, C0), (x1, C1)):
                w = torch.zeros(c, c, 1, 1); w[torch.arange(c), torch.arange(c), 0, 0] = 1.0
                py, pst = ops.conv_gemm(x, ops.pack_conv_weight(w.to(cuda)), c, ksize=1, pad=0, gn_stats=True)
                assert pst is not None, f"{key}: the producer should emit statistics at 128 rows per sample"
                same(py, x, f"{key}: identity producer")
                srcs.append((py, pst))
            (s0, st0), (s1, st1) = srcs
        else:
            s0, s1, st0, st1 = x0, x1, ops.colstats(x0), ops.colstats(x1)
        fbuf, yf = poisoned((B * H * W, C), dt, cuda, pad_cols=16)
        ops.groupnorm_from_stats(s0, st0, g, b, G, eps, silu, x1=s1, st1=st1, out=v4(yf, B, H, W))
        yf2 = ops.groupnorm_from_stats(s0, st0, g, b, G, eps, silu, x1=s1, st1=st1)
        torch.cuda.synchronize()
    assert_guard_intact(ybuf, y, name=key + " groupnorm"); assert_guard_intact(fbuf, yf, name=key + " from_stats")
    same(v4(y, B, H, W), y2, key); same(v4(yf, B, H, W), yf2, key + " from_stats")
    check(key, qty, {"y": y})
    print("from_stats:"); check(key, qty, {"y": yf})


@pytest.mark.parametrize("elem", ELEMS)
@pytest.mark.parametrize("case", R.LNF_CASES, ids=[f"{c[0]}x{c[1]}" for c in R.LNF_CASES])
def test_layernorm_forward_layout(cuda, case, elem):
    from diffute_amd import ops
    rows, C = case
    inputs, qty = R.lnf_eval(case, elem)
    dt = R.ELEMS[elem]
    with ops.element_type(elem):
        x = wide(inputs["x"], dt, cuda, pad=16)
        ybuf, y = poisoned((rows, C), dt, cuda)
        assert len({x.stride(0), y.stride(0), C}) == 3
        ops.layernorm(x, f32(inputs["gamma"], cuda), f32(inputs["beta"], cuda), out=y)
        y2 = ops.layernorm(x, f32(inputs["gamma"], cuda), f32(inputs["beta"], cuda))
        torch.cuda.synchronize()
    key = f"lnf/{rows}x{C}/{elem}"
    assert_guard_intact(ybuf, y, name=key); same(y, y2, key)
    check(key, qty, {"y": y})


# ---------------------------------------------------------------------------------------------- GEMM / implicit conv
def _stat_check(key, yv, s_hip, q_hip, red):
    """sums / sums of squares a kernel emitted against the ROUNDED output's own, in fp64 (the figures of test_groupnorm_statistics_from_the_producer)"""
    yd = host(yv)
    s_ref = yd.sum(red); q_ref = (yd * yd).sum(red)
    es = float(((s_hip - s_ref).abs() / (1e-5 * yd.abs().sum(red) + 1e-4)).max()); eq = float(((q_hip - q_ref).abs() / q_ref).max())
    print(f"{key}: sums {es:.3e}/1 sums of squares {eq:.3e}/1e-5")
    assert es <= 1.0 and eq <= 1e-5, f"{key}: emitted statistics differ from the rounded output's own"


def run_gemm(fam, tn, elem, dev):
    from diffute_amd import ops
    bk = R.GEMM_TN[tn][2]
    inputs, qty, spec = R.gemm_eval(fam, elem, bk)
    dt = R.ELEMS[elem]
    key = f"gemm/{fam}/k{bk}/{elem}"
    reason = R.gemm_cannot_run(tn, fam)
    if reason and fam in ("splitk2", "splitk3", "streamk_tails"):
        return False
    up = lambda name, pad, seed: wide(R.nhwc(inputs[name]), dt, dev, pad=pad, seed=seed) if name in inputs else None
    x0, x1 = up("x0", 8, 90), up("x1", 16, 91)
    kw = dict(x1=x1, ksize=spec["ksize"], stride=spec.get("stride", 1), pad=spec["pad"], ups=spec.get("ups", False), force_tn=tn,
              force_splitk=spec.get("force_splitk", 0), res=up("res", 24, 92), sc0=up("sc0", 8, 93), sc1=up("sc1", 32, 94),
              out_f32=spec.get("out_f32", False), geglu=spec.get("geglu", False), act=spec.get("act", 0))
    if "rowbias" in inputs: kw["rowbias"] = f32(inputs["rowbias"], dev)
    N = spec["N"]
    if fam == "geglu":
        w = ops.pack_linear_weight(inputs["w"][:, :, 0, 0].float().to(dev), geglu=True); kw["bias"] = ops.pack_geglu_bias(f32(inputs["bias"], dev))
    else:
        w = ops.pack_conv_weight(inputs["w"].float().to(dev), shortcut_w=inputs["wsc"].float().to(dev) if "wsc" in inputs else None)
        kw["bias"] = f32(inputs["bias"], dev)
    ref = qty["y"].ref
    Bo, OH, OW, No = ref.shape
    obuf, o = poisoned((Bo * OH * OW, No), torch.float32 if kw["out_f32"] else dt, dev)
    o4 = v4(o, Bo, OH, OW)
    extra = dict(rowstats=True) if fam == "rowstats_ln" else dict(gn_stats=True) if fam == "gn_stats" else {}
    if reason and fam != "gn_stats":                # cfg_applicable refuses the pair: the library must say so, not run another instance
        with pytest.raises(RuntimeError, match="cannot run this problem"):
            ops.conv_gemm(x0, w, N, out=o4, **kw, **extra)
        return False
    r = ops.conv_gemm(x0, w, N, out=o4, **kw, **extra)
    r2 = ops.conv_gemm(x0, w, N, **kw, **extra)
    torch.cuda.synchronize()
    st = r[1] if extra else None
    assert_guard_intact(obuf, o, name=f"{key} tn={tn}")
    same(o4, r2[0] if extra else r2, f"{key} tn={tn}")
    print(f"tn={tn}:"); check(key, {"y": qty["y"]}, {"y": o})
    if fam == "gn_stats":
        if reason:
            assert st is None, f"{key} tn={tn}: expected no statistics ({reason})"
            return False
        assert st is not None, f"{key} tn={tn}: this plan should emit statistics"
        assert torch.equal(st, r2[1]), f"{key} tn={tn}: statistics differ between two runs"
        s_hip, q_hip = ops.stat_sums(st)                                   # [B][N], no pooling
        _stat_check(f"{key} tn={tn}", o4.permute(0, 3, 1, 2), s_hip, q_hip, (2, 3))
    if fam == "rowstats_ln":
        sums = host(st).sum(0)                                             # [tiles][M][2] -> per row
        _stat_check(f"{key} tn={tn} rows", o, sums[:, 0], sums[:, 1], (1,))
        zbuf, z = poisoned((Bo * OH * OW, 200), dt, dev)
        wf = ops.pack_linear_weight(inputs["wf"].float().to(dev))
        ops.conv_gemm(o4, wf, 200, ksize=1, pad=0, force_tn=tn, ln=(st, f32(inputs["c1"], dev), f32(inputs["c2"], dev), 1e-5), out=v4(z, Bo, OH, OW))
        torch.cuda.synchronize()
        assert_guard_intact(zbuf, z, name=f"{key} tn={tn} consumer")
        check(key, {"z": qty["z"]}, {"z": z})
    return True


@pytest.mark.parametrize("elem", ELEMS)
@pytest.mark.parametrize("tn", sorted(R.GEMM_TN))
def test_conv_gemm_every_instance_every_epilogue(cuda, tn, elem):
    """every epilogue family on every tile instance cfg_applicable accepts (fwd_refs.gemm_cannot_run is the table of the pairs that cannot
    run, with the reason); no instance drops out silently: each runs the base family and at least one other"""
    from diffute_amd import ops
    with ops.element_type(elem):
        ran = [fam for fam in R.GEMM_FAMILIES if run_gemm(fam, tn, elem, cuda)]
    print(f"tn={tn} {elem}: ran {ran}")
    assert "base" in ran and len(ran) >= 2, f"tile instance {tn} ran only {ran}"


@pytest.mark.parametrize("elem", ELEMS)
def test_conv_ups2x_per_pixel(cuda, elem):
    from diffute_amd import ops
    B, H, W, Cin, N = R.UPS2X_CASE
    inputs, qty = R.ups2x_eval(elem)
    dt = R.ELEMS[elem]
    with ops.element_type(elem):
        x = wide(R.nhwc(inputs["x"]), dt, cuda)
        wp = ops.pack_ups_phase_weights(ops.pack_conv_weight(inputs["w"].float().to(cuda)), N, Cin)
        obuf, o = poisoned((B * 4 * H * W, N), dt, cuda)
        ops.conv_ups2x(x, wp, N, bias=f32(inputs["bias"], cuda), out=v4(o, B, 2 * H, 2 * W))
        o2 = ops.conv_ups2x(x, wp, N, bias=f32(inputs["bias"], cuda))
        torch.cuda.synchronize()
    key = f"ups2x/{elem}"
    assert_guard_intact(obuf, o, name=key); same(v4(o, B, 2 * H, 2 * W), o2, key)
    check(key, qty, {"y": o})


# ---------------------------------------------------------------------------------------------- halo conv
HALO_INSTANCES = {160: ((0, 0), (160, 4), (160, 12), (160, 8)), 128: ((0, 0), (128, 4), (128, 12))}      # (force_bn, force_waves) of HALO_CASES


@pytest.mark.parametrize("elem", ELEMS)
@pytest.mark.parametrize("N", R.HALO_N)
@pytest.mark.parametrize("shape", R.HALO_SHAPES, ids=[f"{s[0]}x{s[1]}" for s in R.HALO_SHAPES])
def test_conv3x3_gn_halo_per_pixel(cuda, shape, N, elem):
    from diffute_amd import ops
    H, W = shape
    dt = R.ELEMS[elem]
    C0, C1 = R.HALO_C
    ran = 0
    with ops.element_type(elem):
        for variant in R.HALO_VARIANTS:
            inputs, qty = R.halo_eval(shape, N, variant, elem)
            key = f"halo/{H}x{W}_n{N}_{variant}/{elem}"
            up = lambda name, pad, seed: wide(R.nhwc(inputs[name]), dt, cuda, pad=pad, seed=seed) if name in inputs else None
            x0, x1 = up("x0", 8, 90), up("x1", 16, 91)
            kw = dict(x1=x1, bias=f32(inputs["bias"], cuda), res=up("res", 24, 92), sc0=up("sc0", 8, 93), sc1=up("sc1", 32, 94), out_stats=True)
            if "rowbias" in inputs: kw["rowbias"] = f32(inputs["rowbias"], cuda)
            if variant != "plain":
                kw.update(gn=(f32(inputs["gamma"], cuda), f32(inputs["beta"], cuda), 32, 1e-5, True), st0=ops.colstats(x0), st1=ops.colstats(x1))
            w = ops.pack_conv_weight(inputs["w"].float().to(cuda), shortcut_w=inputs["wsc"].float().to(cuda) if "wsc" in inputs else None)
            for bn, waves in (HALO_INSTANCES[N] if elem == "bf16" else ((0, 0),)):
                for split in (0, 1, 2, 4, 8):
                    if (bn, waves) != (0, 0) and split not in (0, 2):
                        continue
                    obuf, o = poisoned((H * W, N), dt, cuda)
                    ikw = dict(force_split=split, force_bn=bn, force_waves=waves)
                    try:
                        _, st = ops.conv3x3_gn(x0, w, N, out=v4(o, 1, H, W), **kw, **ikw)
                    except RuntimeError as ex:
                        assert "does not take this problem" in str(ex) and (split, bn, waves) != (0, 0, 0), f"{key}: {ex}"
                        continue
                    o2, st2 = ops.conv3x3_gn(x0, w, N, **kw, **ikw)
                    torch.cuda.synchronize()
                    tag = f"{key} split={split} bn={bn} waves={waves}"
                    assert_guard_intact(obuf, o, name=tag); same(v4(o, 1, H, W), o2, tag)
                    assert torch.equal(st, st2), f"{tag}: statistics differ between two runs"
                    print(tag); check(key, qty, {"y": o})
                    s_hip, q_hip = ops.stat_sums(st)
                    _stat_check(tag, v4(o, 1, H, W).permute(0, 3, 1, 2), s_hip, q_hip, (2, 3))
                    ran += 1
    assert ran >= len(R.HALO_VARIANTS)


# ---------------------------------------------------------------------------------------------- transformer chains
@pytest.mark.parametrize("elem", ELEMS)
@pytest.mark.parametrize("M", R.XF_M)
@pytest.mark.parametrize("mode", R.XF_MODES)
def test_xf_chain_per_row(cuda, mode, M, elem):
    from diffute_amd import ops
    C = R.XF_C
    inputs, qty = R.xf_eval(mode, M, elem)
    dt = R.ELEMS[elem]
    d16 = lambda t: t.to(cuda).to(dt).contiguous()
    with ops.element_type(elem):
        assert ops.lib().dmx_xf_chain_ok(M, C) == 1
        wo, bo = d16(inputs["wo"]), f32(inputs["bo"], cuda)
        c1, c2 = f32(inputs["c1"], cuda), f32(inputs["c2"], cuda)
        kw = {}
        if mode in ("0", "1"):
            x = wide(inputs["a"], dt, cuda, pad=16, seed=90); res = wide(inputs["res"], dt, cuda, pad=24, seed=91)
        else:
            x = wide(inputs["x"], dt, cuda, pad=16, seed=90); res = None
        if mode == "1":
            kw = dict(wf1=ops.pack_linear_weight(d16(inputs["wf"]).float(), geglu=True), wf2=d16(inputs["w2"]), bf2=f32(inputs["b2"], cuda),
                      wpo=d16(inputs["wp"]), bpo=f32(inputs["bp"], cuda), xres=wide(inputs["xres"], dt, cuda, pad=32, seed=92))
            c1, c2 = ops.pack_geglu_bias(c1), ops.pack_geglu_bias(c2)
        else:
            kw = dict(w1=d16(inputs["wf"]))
        if mode == "2gn":
            HW = inputs["HW"]
            st = ops.colstats(x.view(M // HW, 1, HW, C))
            kw["gn"] = (st, f32(inputs["gg"], cuda), f32(inputs["gb"], cuda), 32, HW, 1e-6)
        Ny = 3 * C if mode in ("2", "2gn") else C
        hbuf, h = poisoned((M, C), dt, cuda); ybuf, y = poisoned((M, Ny), dt, cuda, pad_cols=16)
        ops.xf_chain(int(mode[0]), x, res, wo, bo, c1, c2, h_out=h, y_out=y, **kw)
        h2, y2 = ops.xf_chain(int(mode[0]), x, res, wo, bo, c1, c2, **kw)
        torch.cuda.synchronize()
    key = f"xf/mode{mode}_M{M}/{elem}"
    assert_guard_intact(hbuf, h, name=key + " h"); assert_guard_intact(ybuf, y, name=key + " y")
    same(h, h2, key + " h"); same(y, y2, key + " y")
    check(key, qty, {"h": h, "y": y})


# ---------------------------------------------------------------------------------------------- small ones
@pytest.mark.parametrize("elem", ELEMS)
@pytest.mark.parametrize("case", R.SKINNY_SMALL, ids=[c[0] for c in R.SKINNY_SMALL])
def test_skinny_conv_per_pixel(cuda, case, elem):
    from diffute_amd import ops
    name, B, H, W, Cin, N, gn, fS = case
    inputs, qty = R.skinny_eval(case, elem)
    dt = R.ELEMS[elem]
    with ops.element_type(elem):
        x = wide(R.nhwc(inputs["x"]), dt, cuda)
        sg = dict(x=x, taps=9)
        if gn:
            sg.update(st=ops.colstats(x), gamma=f32(inputs["gamma"], cuda), beta=f32(inputs["beta"], cuda), gn_c0=0)
        wp = ops.skinny_pack(ops.pack_conv_weight(inputs["w"].float().to(cuda)), [(Cin, 9, Cin, 0)])
        kw = dict(gn=(32, Cin, 1e-5, True) if gn else None, bias=f32(inputs["bias"], cuda), rowbias=f32(inputs["rowbias"], cuda),
                  res=wide(R.nhwc(inputs["res"]), dt, cuda, pad=24, seed=92), force_S=fS)
        obuf, o = poisoned((B * H * W, N), dt, cuda)
        ops.skinny_conv([sg], wp, N, out=v4(o, B, H, W), **kw)
        o2 = ops.skinny_conv([sg], wp, N, **kw)
        torch.cuda.synchronize()
    key = f"skinny/{name}/{elem}"
    assert_guard_intact(obuf, o, name=key); same(v4(o, B, H, W), o2, key)
    check(key, qty, {"y": o})


@pytest.mark.parametrize("elem", ELEMS)
@pytest.mark.parametrize("case", R.LS_CASES, ids=[f"b{c[0]}_n{c[1]}" for c in R.LS_CASES])
def test_time_embedding_linear_small(cuda, case, elem):
    from diffute_amd import ops
    B, N = case
    inputs, qty = R.ls_eval(case, elem)
    dt = R.ELEMS[elem]
    with ops.element_type(elem):
        emb = ops.timestep_embedding(inputs["t"].to(cuda), inputs["freq"].to(cuda), B, 320)
        x = wide(inputs["emb32"], torch.float32, cuda)                    # the float32 embedding of the reference, row stride 336
        ybuf, y = poisoned((B, N), torch.float32, cuda)
        w = wide(inputs["w"], dt, cuda, pad=16, seed=93)
        ops.linear_small(x, w, f32(inputs["bias"], cuda), silu_in=True, out=y)
        y2 = ops.linear_small(x, w, f32(inputs["bias"], cuda), silu_in=True)
        torch.cuda.synchronize()
    key = f"ls/b{B}_n{N}/{elem}"
    assert_guard_intact(ybuf, y, name=key); same(y, y2, key)
    check(key, qty, {"emb": emb, "y": y})


@pytest.mark.parametrize("elem", ELEMS)
@pytest.mark.parametrize("case", R.IM2COL_CASES, ids=["x".join(map(str, c)) for c in R.IM2COL_CASES])
def test_im2col_small_exact(cuda, case, elem):
    from diffute_amd import ops
    B, H, W, C, st, Kpad = case
    inputs, qty = R.im2col_eval(case, elem)
    dt = R.ELEMS[elem]
    with ops.element_type(elem):
        col = ops.im2col_small(nhwc=wide(R.nhwc(inputs["x"]), dt, cuda), stride=st, Kpad=Kpad)
        torch.cuda.synchronize()
    want = qty["col"].ref.to(dt)
    assert torch.equal(bits(col), bits(want)), f"im2col {case}: not bit-equal to the unfolded input"
    assert not bits(col[..., 9 * C:]).any(), f"im2col {case}: the Kpad tail is not bit-zero"
