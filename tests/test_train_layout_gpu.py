"""The training (backward) kernels the way the training graph calls them: operands that are column slices of fused / wider
buffers, outputs written into poisoned buffers with guard bands, ragged tiles, spiked keys, gradient scaling, on both builds.

Every case (train_refs.py holds the case tables, the fp64 references and the bounds) checks
  * the whole-tensor bound of test_train_ops_gpu.py (TOL_W / TOL_D / TOL_N / TOL_A, forward 4e-3, fp16 forward attention 2e-3),
  * a per-slice bound (util.slice_err: per query / key row and per head; per channel and per (sample, group); per row and
    per column; per output channel and per tap) - the per-kernel number, or 3 x the worst slice of the rounding-point
    restatement where that exceeds a third of it; fp32 outputs (lse, dgamma, dbeta, saved stats, colsum, wgrad, loss): 8 x the
    deviation of torch float32 from fp64, never below 2^-20.  The recorded figures are train_floors.py's,
  * that every output element was written and nothing outside the logical output was (util.poisoned / assert_guard_intact),
  * where stated, bit-equality of two runs / of accumulate=1 with "previous + fresh".
Each check prints one line `key:quantity whole <error>/<bound> slice <error>/<bound>` (pytest -rA shows them)."""
import pytest
import torch

import train_refs as R
from util import assert_close, assert_close_slices, assert_guard_intact, poisoned, seeded

pytestmark = pytest.mark.gpu
ELEMS = ["bf16", "fp16"]


@pytest.fixture(scope="module")
def cuda():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda")


def host(t):
    return t.detach().double().cpu()


def bits(t):
    return t.detach().cpu().contiguous().view(torch.int16 if t.element_size() == 2 else torch.int32)


def wide(t, dt, dev, pad=8, seed=99):
    """`t` (CPU, [..., C]) as a column slice of a wider device tensor whose other columns hold finite junk"""
    C = t.shape[-1]
    w = (seeded(tuple(t.shape[:-1]) + (C + 2 * pad,), seed) * 3.0).to(dev).to(dt)
    w[..., pad:pad + C] = t.to(dev).to(dt)
    return w[..., pad:pad + C]


def assert_close_f64(hip, ref, tol, name=""):
    """assert_close for fp32 outputs: the same figure taken in double (assert_close's float32 cast would round the fp64 reference)"""
    assert hip.shape == ref.shape, f"{name}: shape {tuple(hip.shape)} vs {tuple(ref.shape)}"
    assert torch.isfinite(hip).all(), f"{name}: non-finite values in HIP output"
    e = R.rel_l2_f64(hip, ref)
    assert e <= tol, f"{name}: rel-L2 {e:.3e} > {tol:.1e} (max abs diff {float((hip - ref).abs().max()):.3e})"
    return e


def check(key, qty, got, bounds=None):
    """whole-tensor and per-slice parity of every quantity in `got` ({name: tensor in the reference's layout}); one line per
    quantity with both figures, every miss is reported.  `bounds`: {name: (whole, slice)}, train_refs.bounds by default
    (test_fwd_layout_gpu.py passes fwd_refs.bounds)"""
    bounds = R.bounds(key, qty) if bounds is None else bounds
    misses = []
    for name, t in got.items():
        q = qty[name]; wt, st = bounds[name]
        t = host(t).reshape(q.ref.shape)
        fig = []
        for fn, args in ((assert_close if q.kind == "16" else assert_close_f64, (t, q.whole_ref, wt, f"{key}:{name}")),
                         (assert_close_slices, (t, q.ref, st, q.dims, f"{key}:{name}"))):
            try:
                fig.append(f"{fn(*args):.3e}")
            except AssertionError as ex:
                fig.append("MISS"); misses.append(str(ex))
        print(f"{key}:{name} whole {fig[0]}/{wt:.2e} slice {fig[1]}/{st:.2e}")
    assert not misses, "\n".join(misses)


# ---------------------------------------------------------------------------------------------- attention
def run_attention(case, elem, dev, gscale=1.0):
    from diffute_amd import ops
    name, layout, B, H, Sq, Skv = case
    C = H * 64
    inputs, qty = R.attn_eval(case, elem, gscale)
    dt = R.ELEMS[elem]
    f2 = lambda t: t.reshape(-1, C)
    with ops.element_type(elem):
        if layout == "self":                                    # q | k | v from one [B*S][3C] buffer, dq | dk | dv into one
            qkv = torch.cat([f2(inputs["q"]), f2(inputs["k"]), f2(inputs["v"])], -1).to(dev).to(dt)
            q, k, v = qkv[:, :C], qkv[:, C:2 * C], qkv[:, 2 * C:]
            sp = Skv
            gbuf, g = poisoned((B * Sq, 3 * C), dt, dev)
            dq, dk, dv = g[:, :C], g[:, C:2 * C], g[:, 2 * C:]
            dq_guard = None
        else:                                                   # k | v from one [B*sp][2C] context projection, sp > Skv
            sp = (Skv + 63) // 64 * 64
            kv = (seeded((B, sp, 2 * C), 98) * 2.0).to(dt)       # rows [Skv, sp): finite values nothing may read into the result
            kv[:, :Skv, :C] = inputs["k"].to(dt); kv[:, :Skv, C:] = inputs["v"].to(dt)
            kv = kv.reshape(B * sp, 2 * C).to(dev)
            k, v = kv[:, :C], kv[:, C:]
            q = wide(f2(inputs["q"]), dt, dev)
            gbuf, g = poisoned((B * sp, 2 * C), dt, dev)
            g.zero_()                                           # the executor pre-zeroes dkv: the padded rows must stay zero
            dk, dv = g[:, :C], g[:, C:]
            dq_guard, dq = poisoned((B * Sq, C), dt, dev)
        do = wide(f2(inputs["do"]), dt, dev, pad=16, seed=97)
        obuf, o = poisoned((B * Sq, C + 16), dt, dev)           # o and do share one row stride in the C-ABI
        o = o[:, :C]
        lbuf, lse = poisoned((B * H, Sq), torch.float32, dev, pad_cols=0)
        assert o.stride(0) == do.stride(0)
        ops.attention_train(q, k, v, B, H, Sq, Skv, R.ATTN_SCALE, kv_rows=sp, out=o, lse=lse.view(B, H, Sq))
        ops.attention_bwd(q, k, v, o, do, lse.view(B, H, Sq), B, H, Sq, Skv, R.ATTN_SCALE, kv_rows=sp, dq=dq, dk=dk, dv=dv)
        # a second run into fresh buffers: bit-identical
        g2buf, g2 = poisoned(tuple(g.shape), dt, dev)
        if layout == "self":
            dq2, dk2, dv2 = g2[:, :C], g2[:, C:2 * C], g2[:, 2 * C:]
        else:
            g2.zero_(); dk2, dv2 = g2[:, :C], g2[:, C:]; dq2 = torch.empty_like(dq)
        o2 = torch.empty_like(obuf)[2:2 + B * Sq, 8:8 + C]; lse2 = torch.empty(B, H, Sq, dtype=torch.float32, device=dev)
        ops.attention_train(q, k, v, B, H, Sq, Skv, R.ATTN_SCALE, kv_rows=sp, out=o2, lse=lse2)
        ops.attention_bwd(q, k, v, o2, do, lse2, B, H, Sq, Skv, R.ATTN_SCALE, kv_rows=sp, dq=dq2, dk=dk2, dv=dv2)
        torch.cuda.synchronize()
    key = f"attn/{name}/{elem}" + ("/gs" if gscale != 1.0 else "")
    # guards: nothing outside the logical outputs, everything inside written
    assert_guard_intact(gbuf, g, name=key + " gradient buffer")
    if dq_guard is not None:
        assert_guard_intact(dq_guard, dq, name=key + " dq")
    assert_guard_intact(obuf, o, name=key + " o")
    assert_guard_intact(lbuf, lse, name=key + " lse")
    live = lambda t: t.reshape(B, sp, C)[:, :Skv]
    if sp > Skv:
        for nm, t in (("dk", dk), ("dv", dv)):
            assert not bits(t.reshape(B, sp, C)[:, Skv:]).any(), f"{key}: padded context rows of {nm} are no longer bit-zero"
    for a, b_, nm in ((o, o2, "o"), (lse.view(B, H, Sq), lse2, "lse"), (dq, dq2, "dq"), (dk, dk2, "dk"), (dv, dv2, "dv")):
        assert torch.equal(bits(a), bits(b_)), f"{key}: {nm} differs between two runs"
    check(key, qty, {"o": o, "lse": lse, "dq": dq, "dk": live(dk), "dv": live(dv)})


@pytest.mark.parametrize("elem", ELEMS)
@pytest.mark.parametrize("case", R.ATTN_CASES, ids=[c[0] for c in R.ATTN_CASES])
def test_attention_layout(cuda, case, elem):
    run_attention(case, elem, cuda)


# ---------------------------------------------------------------------------------------------- GroupNorm
def run_groupnorm(case, elem, dev, gscale=1.0):
    from diffute_amd import ops
    name, B, H, W, C, G, silu, c0 = case
    inputs, qty = R.gn_eval(case, elem, gscale)
    dt = R.ELEMS[elem]
    nhwc = lambda t: t.permute(0, 2, 3, 1).contiguous()
    with ops.element_type(elem):
        x = wide(nhwc(inputs["x"]), dt, dev); dy = wide(nhwc(inputs["dy"]), dt, dev, seed=96); r = wide(nhwc(inputs["r"]), dt, dev, seed=95)
        gamma, beta = inputs["gamma"].float().to(dev), inputs["beta"].float().to(dev)
        sl = (lambda t: (t[..., :c0], t[..., c0:])) if c0 else (lambda t: (t, None))
        x0, x1 = sl(x); r0, r1 = sl(r)
        if c0:                                                   # the skip and hidden tensors are separate buffers with their own strides
            x0 = wide(nhwc(inputs["x"])[..., :c0], dt, dev, pad=16, seed=92); x1 = wide(nhwc(inputs["x"])[..., c0:], dt, dev, pad=40, seed=94)
            r0 = wide(nhwc(inputs["r"])[..., :c0], dt, dev, pad=48, seed=91); r1 = wide(nhwc(inputs["r"])[..., c0:], dt, dev, pad=32, seed=93)
            assert len({x0.stride(-2), x1.stride(-2), r0.stride(-2), r1.stride(-2), dy.stride(-2)}) == 5
        ybuf, y = poisoned((B * H * W, C), dt, dev)
        sbuf, st = poisoned((B * G, 2), torch.float32, dev, pad_cols=0)
        ops.groupnorm_train(x0, gamma, beta, G, 1e-5, silu, x1=x1, out=y.view(B, H, W, C), stats=st.view(B, G, 2))
        dbuf, dx = poisoned((B * H * W, C), dt, dev)
        dx0, dx1 = sl(dx.view(B, H, W, C))                       # the two sources' gradients: slices of one wider tensor
        gbuf, dg = poisoned((C,), torch.float32, dev); bbuf, db = poisoned((C,), torch.float32, dev)
        ops.groupnorm_bwd(x0, dy, gamma, beta, G, silu, st.view(B, G, 2), x1=x1, res0=r0, res1=r1, dx0=dx0, dx1=dx1, into=(dg, db))
        # accumulate = 1 onto a non-zero gradient: exactly previous + fresh (one fp32 add per channel)
        prev_g = seeded((C,), 7).to(dev) * gscale; prev_b = seeded((C,), 8).to(dev) * gscale
        ag, ab = prev_g.clone(), prev_b.clone()
        dxb = torch.empty(B, H, W, C, dtype=dt, device=dev)
        ops.groupnorm_bwd(x0, dy, gamma, beta, G, silu, st.view(B, G, 2), x1=x1, res0=r0, res1=r1, dx0=sl(dxb)[0], dx1=sl(dxb)[1],
                          into=(ag, ab), accumulate=True)
        torch.cuda.synchronize()
    key = f"gn/{name}/{elem}" + ("/gs" if gscale != 1.0 else "")
    for buf, view, nm in ((ybuf, y, "y"), (sbuf, st, "stats"), (dbuf, dx, "dx"), (gbuf, dg, "dgamma"), (bbuf, db, "dbeta")):
        assert_guard_intact(buf, view, name=f"{key} {nm}")
    assert torch.equal(bits(ag), bits(prev_g + dg)) and torch.equal(bits(ab), bits(prev_b + db)), f"{key}: accumulate != previous + fresh"
    assert torch.equal(bits(dxb.view(-1, C)), bits(dx)), f"{key}: dx differs between two runs"
    check(key, qty, {"y": y, "dx": dx, "dgamma": dg, "dbeta": db, "stats": st})


@pytest.mark.parametrize("elem", ELEMS)
@pytest.mark.parametrize("case", R.GN_CASES, ids=[c[0] for c in R.GN_CASES])
def test_groupnorm_layout(cuda, case, elem):
    run_groupnorm(case, elem, cuda)


# ---------------------------------------------------------------------------------------------- LayerNorm / GEGLU
def run_layernorm(case, elem, dev, gscale=1.0):
    from diffute_amd import ops
    rows, C = case
    inputs, qty = R.ln_eval(case, elem, gscale)
    dt = R.ELEMS[elem]
    with ops.element_type(elem):
        x = wide(inputs["x"], dt, dev, pad=16); dy = wide(inputs["dy"], dt, dev, pad=24, seed=96); r = wide(inputs["r"], dt, dev, pad=32, seed=95)
        gamma = inputs["gamma"].float().to(dev)
        dbuf, dx = poisoned((rows, C), dt, dev)                      # row strides: x C+32, dy C+48, res C+64, dx C+16
        assert len({x.stride(0), dy.stride(0), r.stride(0), dx.stride(0)}) == 4
        gbuf, dg = poisoned((C,), torch.float32, dev); bbuf, db = poisoned((C,), torch.float32, dev)
        ops.layernorm_bwd(x, dy, gamma, res=r, dx=dx, into=(dg, db))
        prev_g = seeded((C,), 7).to(dev) * gscale; prev_b = seeded((C,), 8).to(dev) * gscale
        ag, ab = prev_g.clone(), prev_b.clone()
        dx2, _, _ = ops.layernorm_bwd(x, dy, gamma, res=r, into=(ag, ab), accumulate=True)
        torch.cuda.synchronize()
    key = f"ln/{rows}x{C}/{elem}" + ("/gs" if gscale != 1.0 else "")
    for buf, view, nm in ((dbuf, dx, "dx"), (gbuf, dg, "dgamma"), (bbuf, db, "dbeta")):
        assert_guard_intact(buf, view, name=f"{key} {nm}")
    assert torch.equal(bits(ag), bits(prev_g + dg)) and torch.equal(bits(ab), bits(prev_b + db)), f"{key}: accumulate != previous + fresh"
    assert torch.equal(bits(dx2), bits(dx)), f"{key}: dx differs between two runs"
    check(key, qty, {"dx": dx, "dgamma": dg, "dbeta": db})


@pytest.mark.parametrize("elem", ELEMS)
@pytest.mark.parametrize("case", R.LN_CASES, ids=[f"{c[0]}x{c[1]}" for c in R.LN_CASES])
def test_layernorm_bwd_layout(cuda, case, elem):
    run_layernorm(case, elem, cuda)


def run_geglu(case, elem, dev, gscale=1.0):
    from diffute_amd import ops
    rows, C2 = case
    inputs, qty = R.geglu_eval(case, elem, gscale)
    dt = R.ELEMS[elem]
    with ops.element_type(elem):
        h = wide(inputs["h"], dt, dev, pad=16); dy = wide(inputs["dy"], dt, dev, pad=24, seed=96)
        ybuf, y = poisoned((rows, C2), dt, dev)                      # row strides: h 2 C2 + 32, dy C2 + 48, y C2 + 16, dh 2 C2 + 16
        hbuf, dh = poisoned((rows, 2 * C2), dt, dev)
        assert len({h.stride(0), dy.stride(0), y.stride(0), dh.stride(0)}) == 4
        ops.geglu_fwd(h, out=y)
        ops.geglu_bwd(h, dy, dx=dh)
        torch.cuda.synchronize()
    key = f"geglu/{rows}x{C2}/{elem}" + ("/gs" if gscale != 1.0 else "")
    assert_guard_intact(ybuf, y, name=key + " y"); assert_guard_intact(hbuf, dh, name=key + " dh")
    check(key, qty, {"y": y, "dh": dh})


@pytest.mark.parametrize("elem", ELEMS)
@pytest.mark.parametrize("case", R.GEGLU_CASES, ids=[f"{c[0]}x{c[1]}" for c in R.GEGLU_CASES])
def test_geglu_layout(cuda, case, elem):
    run_geglu(case, elem, cuda)


# ---------------------------------------------------------------------------------------------- wgrad / dgrad / colsum
def run_conv(case, elem, dev, gscale=1.0):
    from diffute_amd import ops
    name, B, H, W, Cin, Cout, st, pad, asym = case
    inputs, qty = R.conv_eval(case, elem, gscale)
    dt = R.ELEMS[elem]
    nhwc = lambda t: t.permute(0, 2, 3, 1).contiguous()
    got = {}
    key = f"conv/{name}/{elem}" + ("/gs" if gscale != 1.0 else "")
    with ops.element_type(elem):
        x = wide(nhwc(inputs["x"]), dt, dev); dy = wide(nhwc(inputs["dy"]), dt, dev, seed=96); r = wide(nhwc(inputs["r"]), dt, dev, seed=95)
        if Cin % 64 == 0:                                            # (the weight gradient wants 64-channel sources)
            wbuf, dw = poisoned((Cout, 9 * Cin), torch.float32, dev, pad_cols=0)
            ops.conv_wgrad(x, dy, ksize=3, stride=st, pad=pad, out=dw)
            acc = (seeded((Cout, 9 * Cin), 7) * gscale).to(dev); prev = acc.clone()
            ops.conv_wgrad(x, dy, ksize=3, stride=st, pad=pad, into=acc)
            torch.cuda.synchronize()
            assert_guard_intact(wbuf, dw, name=key + " dw")
            assert torch.equal(bits(acc), bits(prev + dw)), f"{key}: wgrad accumulate != previous + fresh"
            got["dw"] = dw
        wt = ops.pack_conv_weight_t(inputs["w"].float().to(dev))
        xbuf, dx = poisoned((B * H * W, Cin), dt, dev)
        ops.conv_dgrad(dy, wt, Cin, ksize=3, stride=st, pad=pad, dx=dx.view(B, H, W, Cin))
        rbuf, dxr = poisoned((B * H * W, Cin), dt, dev)
        ops.conv_dgrad(dy, wt, Cin, ksize=3, stride=st, pad=pad, res=r, dx=dxr.view(B, H, W, Cin))
        torch.cuda.synchronize()
    assert_guard_intact(xbuf, dx, name=key + " dx"); assert_guard_intact(rbuf, dxr, name=key + " dx + res")
    got["dx"] = dx; got["dx_res"] = dxr
    check(key, qty, got)


ALL_CONV = R.CONV_CASES + R.DGRAD_EXTRA


@pytest.mark.parametrize("elem", ELEMS)
@pytest.mark.parametrize("case", ALL_CONV, ids=[c[0] for c in ALL_CONV])
def test_conv_wgrad_dgrad_layout(cuda, case, elem):
    run_conv(case, elem, cuda)


def run_colsum(case, elem, dev, gscale=1.0):
    from diffute_amd import ops
    name, G, rpg, N = case
    inputs, qty = R.colsum_eval(case, elem, gscale)
    dt = R.ELEMS[elem]
    with ops.element_type(elem):
        dy = wide(inputs["dy"].reshape(G * rpg, N), dt, dev)
        obuf, out = poisoned((G, N), torch.float32, dev)             # ldo > N
        ops.colsum(dy, groups=G, out=out)
        acc = (seeded((G, N), 7) * gscale).to(dev); prev = acc.clone()
        ops.colsum(dy, groups=G, into=acc)
        torch.cuda.synchronize()
    key = f"colsum/{name}/{elem}" + ("/gs" if gscale != 1.0 else "")
    assert_guard_intact(obuf, out, name=key)
    assert torch.equal(bits(acc), bits(prev + out)), f"{key}: accumulate != previous + fresh"
    check(key, qty, {"colsum": out})


@pytest.mark.parametrize("elem", ELEMS)
@pytest.mark.parametrize("case", R.COLSUM_CASES, ids=[c[0] for c in R.COLSUM_CASES])
def test_colsum_layout(cuda, case, elem):
    run_colsum(case, elem, cuda)


# ---------------------------------------------------------------------------------------------- the exact helpers of dgrad
@pytest.mark.parametrize("elem", ELEMS)
def test_zero_insert2_exact(cuda, elem):
    from diffute_amd import ops
    dt = R.ELEMS[elem]
    B, OH, OW, C = 3, 5, 7, 24
    src = R.inp((B, OH, OW, C), 1, elem)
    with ops.element_type(elem):
        zbuf, z = poisoned((B * 4 * OH * OW, C), dt, cuda, pad_cols=0)
        ops.zero_insert2(wide(src, dt, cuda), out=z.view(B, 2 * OH, 2 * OW, C))
        torch.cuda.synchronize()
    assert_guard_intact(zbuf, z, name="zero_insert2")
    want = torch.zeros(B, 2 * OH, 2 * OW, C, dtype=dt)
    want[:, ::2, ::2] = src.to(dt)
    assert torch.equal(bits(z.view(B, 2 * OH, 2 * OW, C)), bits(want))


@pytest.mark.parametrize("f32", [False, True], ids=["in16", "in32"])
@pytest.mark.parametrize("elem", ELEMS)
def test_sumpool2_exact(cuda, elem, f32):
    from diffute_amd import ops
    dt = R.ELEMS[elem]
    B, H, W, C = 3, 5, 7, 24
    du = seeded((B, 2 * H, 2 * W, C), 1) if f32 else R.inp((B, 2 * H, 2 * W, C), 1, elem).float()
    prev = R.inp((B, H, W, C), 2, elem).float()
    s = torch.zeros(B, H, W, C)
    for dy, dx in ((0, 0), (0, 1), (1, 0), (1, 1)):                  # the kernel's order: one fp32 add per tap
        s = s + du[:, dy::2, dx::2]
    with ops.element_type(elem):
        dud = (du.to(cuda) if f32 else du.to(cuda).to(dt))
        dud = wide(dud.cpu(), dud.dtype, cuda)
        obuf, o = poisoned((B * H * W, C), dt, cuda)
        ops.sumpool2(dud, dx=o.view(B, H, W, C))
        abuf, a = poisoned((B * H * W, C), dt, cuda)
        a.view(B, H, W, C).copy_(prev.to(dt))
        ops.sumpool2(dud, dx=a.view(B, H, W, C), accumulate=True)
        torch.cuda.synchronize()
    assert_guard_intact(obuf, o, name="sumpool2"); assert_guard_intact(abuf, a, name="sumpool2 accumulate")
    assert torch.equal(bits(o.view(B, H, W, C)), bits(s.to(dt))), "sumpool2 is not bit-equal to the fp32 2x2 sum"
    assert torch.equal(bits(a.view(B, H, W, C)), bits((s + prev).to(dt))), "sumpool2 accumulate is not bit-equal"


# ---------------------------------------------------------------------------------------------- loss
@pytest.mark.parametrize("gs", [1.0, 65536.0], ids=["gs1", "gs65536"])
@pytest.mark.parametrize("n", R.MSE_SIZES)
def test_mse_loss(cuda, n, gs):
    from diffute_amd import ops
    inputs, qty = R.mse_eval(n)
    p, t = inputs["pred"], inputs["target"]
    pd, td = p.float().to(cuda), t.float().to(cuda)
    lbuf, loss = poisoned((1,), torch.float32, cuda)
    dbuf, dp = poisoned((1, n), torch.float32, cuda, pad_cols=0)
    ops.mse_loss(pd, td, grad_scale=gs, dpred=dp.view(n), loss=loss)
    loss2, dp2 = ops.mse_loss(pd, td, grad_scale=gs)
    # dpred = NULL: only the loss is written
    lbuf3, loss3 = poisoned((1,), torch.float32, cuda)
    ops.mse_loss(pd, td, grad_scale=gs, dpred=None, loss=loss3)
    torch.cuda.synchronize()
    assert_guard_intact(lbuf, loss, name="mse loss"); assert_guard_intact(dbuf, dp, name="mse dpred"); assert_guard_intact(lbuf3, loss3, name="mse loss (no dpred)")
    assert torch.equal(bits(loss), bits(loss2)) and torch.equal(bits(loss), bits(loss3)) and torch.equal(bits(dp.view(n)), bits(dp2)), "mse_loss differs between runs"
    assert torch.equal(bits(pd), bits(p.float())) and torch.equal(bits(td), bits(t.float())), "mse_loss wrote to its inputs"
    check(f"mse/{n}", qty, {"loss": loss})
    want = 2.0 * (p - t) / n * gs                                     # one fp32 rounding per operation: three half-ulps < 2^-22
    err = ((host(dp.view(n)) - want).abs() / want.abs().clamp_min(1e-300)).max()
    print(f"mse/{n} gs={gs}: dpred worst relative error {float(err):.3e}/{2.0 ** -22:.2e}")
    assert torch.isfinite(dp).all() and float(err) <= 2.0 ** -22, f"mse dpred: relative error {float(err):.3e} > 2^-22"


# ---------------------------------------------------------------------------------------------- gradient scaling (fp16 build)
@pytest.mark.parametrize("factor", R.GS_FACTORS, ids=["x1", "x2^10", "x2^16"])
@pytest.mark.parametrize("kernel", ["attention", "groupnorm", "layernorm", "geglu", "conv", "colsum"])
def test_fp16_gradient_scaling(cuda, kernel, factor):
    """the upstream gradient ~ N(0, 2^-7) times the GradScaler factor (2^10 .. 2^16): relative errors are scale-free, so every
    factor must meet the bounds of the factor-1 case, and stay finite"""
    run, case = {"attention": (run_attention, R.ATTN_GS_CASE), "groupnorm": (run_groupnorm, R.GN_GS_CASE), "layernorm": (run_layernorm, R.LN_GS_CASE),
                 "geglu": (run_geglu, R.GEGLU_GS_CASE), "conv": (run_conv, R.CONV_GS_CASE), "colsum": (run_colsum, R.COLSUM_GS_CASE)}[kernel]
    run(case, "fp16", cuda, gscale=R.GS_BASE * factor)
