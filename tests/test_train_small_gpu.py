"""The small kernels of the training graphs, one by one, through the dmx_test_* entries of the C-ABI: the W^T transposes (single and
batched), the gradient add, the row softmax and its backward (the VAE's single-head attention), the 1x1 convolutions between <= 8
channels, the backward of the fp32 time-embedding linears and the casts around the posterior mode.  Until now they ran only inside
the tiny VAE / UNet training steps (whole-gradient bounds of 5e-2).

Conventions are test_train_layout_gpu.py's: train_refs.py holds the cases, the fp64 references and the bounds (kernels that only
move or cast data are compared bit for bit); every input is a column slice of a wider junk-filled tensor, every output goes into
a sentinel-filled buffer with guard bands, every case runs twice into fresh buffers and must repeat bit for bit; both builds.
Each check prints `key:quantity whole <error>/<bound> slice <error>/<bound>` (pytest -rA shows them)."""
import ctypes

import pytest
import torch

import train_refs as R
from test_train_layout_gpu import bits, check, host, wide
from util import SENTINEL_BITS, assert_guard_intact, poisoned, seeded, slice_err

pytestmark = pytest.mark.gpu
ELEMS = ["bf16", "fp16"]


@pytest.fixture(scope="module")
def cuda():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda")


def call(name, *args):
    """one dmx_test_* entry of the active build on the current stream; raises with the library's message"""
    from diffute_amd import _cabi, ops
    l = ops.lib()
    _cabi.check(getattr(l, name)(*[_cabi.ptr(a) if isinstance(a, torch.Tensor) or a is None else a for a in args], _cabi.current_stream()), name, l)


def refused(name, *args):
    """the entry must refuse these arguments on the host: a non-zero code and a message"""
    from diffute_amd import _cabi, ops
    l = ops.lib()
    rc = getattr(l, name)(*[_cabi.ptr(a) if isinstance(a, torch.Tensor) or a is None else a for a in args], _cabi.current_stream())
    msg = l.dmx_last_error()
    assert rc != 0 and msg, f"{name}: expected a refusal, got code {rc}"
    return msg.decode()


def untouched(buf):
    it, sb = SENTINEL_BITS[buf.dtype]
    return bool((buf.detach().cpu().contiguous().view(it) == sb).all())


def check_exact(key, qty, got):
    """bit-equality with the single torch operation; the figures are printed in the common format"""
    for name, t in got.items():
        want = qty[name].ref.to(t.dtype)
        h = host(t).reshape(want.shape)
        e = R.rel_l2_f64(h, want.double()); s = slice_err(h, want.double(), 0)[0]
        print(f"{key}:{name} whole {e:.3e}/{0.0:.2e} slice {s:.3e}/{0.0:.2e}")
        assert torch.equal(bits(t.reshape(want.shape)), bits(want)), f"{key}:{name}: not bit-equal ({int((bits(t.reshape(want.shape)) != bits(want)).sum())} elements differ)"


def same(key, pairs):
    for nm, a, b in pairs:
        assert torch.equal(bits(a), bits(b)), f"{key}: {nm} differs between two runs"


# ---------------------------------------------------------------------------------------------- transposes
@pytest.mark.parametrize("elem", ELEMS)
@pytest.mark.parametrize("case", R.TRANSPOSE_CASES, ids=[f"{c[0]}x{c[1]}" for c in R.TRANSPOSE_CASES])
def test_transpose_single(cuda, case, elem):
    from diffute_amd import ops
    Rr, C = case
    inputs, qty = R.transpose_eval(case, elem)
    dt = R.ELEMS[elem]
    key = f"transpose/{Rr}x{C}/{elem}"
    with ops.element_type(elem):
        x = wide(inputs["x"], dt, cuda, pad=3)                       # ldin = C + 6
        runs = []
        for _ in range(2):
            buf, out = poisoned((C, Rr), dt, cuda)                   # ldout = R + 16
            call("dmx_test_transpose_bf16", x, x.stride(0), out, out.stride(0), Rr, C)
            runs.append((buf, out))
        torch.cuda.synchronize()
    for buf, out in runs:
        assert_guard_intact(buf, out, name=key)
    same(key, [("out", runs[0][1], runs[1][1])])
    check_exact(key, qty, {"out": runs[0][1]})


def _arena(jobs, xs, dt, dev, seed):
    """inputs in one junk-filled arena, outputs in one sentinel-filled arena, each job at its stride and base offset"""
    def layout(sizes_offs):
        pos, out = 16, []
        for size, off in sizes_offs:
            out.append(pos + off); pos = (pos + off + size + 16 + 7) // 8 * 8
        return out, pos + 16
    ins, nin = layout([(j[0] * j[2], j[4]) for j in jobs])
    outs, nout = layout([(j[1] * j[3], j[5]) for j in jobs])
    ain = (seeded((nin,), seed) * 3.0).to(dev).to(dt)
    it, sb = SENTINEL_BITS[dt]
    aout = torch.full((nout,), sb, dtype=it, device=dev).view(dt)
    assert ain.data_ptr() % 16 == 0 and aout.data_ptr() % 16 == 0
    vin = [ain.as_strided((j[0], j[1]), (j[2], 1), o) for j, o in zip(jobs, ins)]
    vout = [aout.as_strided((j[1], j[0]), (j[3], 1), o) for j, o in zip(jobs, outs)]
    for v, x, j, o in zip(vin, xs, jobs, ins):
        v.copy_(x.to(dt))
        assert (v.data_ptr() // 2) % 8 == j[4] % 8
    return ain, aout, vin, vout


def _run_batch(jobs, vin, vout, table):
    from diffute_amd import _cabi, ops
    arr = (_cabi.TestTrJob * len(jobs))()
    for a, j, i, o in zip(arr, jobs, vin, vout):
        a.in_ = i.data_ptr(); a.ldin = j[2]; a.out = o.data_ptr(); a.ldout = j[3]; a.R = j[0]; a.C = j[1]
    l = ops.lib()
    _cabi.check(l.dmx_test_transpose_batch(ctypes.cast(arr, ctypes.c_void_p), len(jobs), _cabi.ptr(table), table.numel(), _cabi.current_stream()), "transpose_batch", l)


@pytest.mark.parametrize("elem", ELEMS)
def test_transpose_batch(cuda, elem):
    """one launch over ten jobs (vector and element paths on either side, ragged tiles, one-tile jobs at both ends of the bisection),
    then - with the entry's copy of the uploaded table alive - the same batch again, the same length at other addresses and another
    length: the unchanged-table path and both ways of noticing a change"""
    from diffute_amd import ops
    dt = R.ELEMS[elem]
    it, sb = SENTINEL_BITS[dt]
    key = f"transpose_batch/{elem}"
    with ops.element_type(elem):
        table = torch.zeros(81920, dtype=torch.uint8, device=cuda)
        _run_batch([], [], [], table)                                # forget whatever an earlier test left
        inputs, qty = R.transpose_batch_eval(elem)
        ain, aout, vin, vout = _arena(R.TRB_JOBS, inputs["xs"], dt, cuda, 50)
        _run_batch(R.TRB_JOBS, vin, vout, table)
        torch.cuda.synchronize()
        assert_guard_intact(aout, vout, name=key)
        check_exact(key, qty, {f"out{i}": v for i, v in enumerate(vout)})
        first = [v.clone() for v in vout]
        # the same batch again: the table is not uploaded; every output is written again
        aout.view(it).fill_(sb)
        _run_batch(R.TRB_JOBS, vin, vout, table)
        torch.cuda.synchronize()
        assert_guard_intact(aout, vout, name=key + " again")
        same(key, [(f"out{i}", a, b) for i, (a, b) in enumerate(zip(first, vout))])
        # the same length, other addresses and other data
        aout.view(it).fill_(sb)
        inputs2, qty2 = R.transpose_batch_eval(elem, seed=100)
        ain2, aout2, vin2, vout2 = _arena(R.TRB_JOBS, inputs2["xs"], dt, cuda, 51)
        _run_batch(R.TRB_JOBS, vin2, vout2, table)
        torch.cuda.synchronize()
        assert_guard_intact(aout2, vout2, name=key + " moved")
        assert untouched(aout), f"{key}: the moved batch wrote to the previous batch's outputs"
        check_exact(key + "/moved", qty2, {f"out{i}": v for i, v in enumerate(vout2)})
        # another length
        sub = R.TRB_JOBS[1:8]
        inputs3, qty3 = R.transpose_batch_eval(elem, jobs=sub, seed=200)
        ain3, aout3, vin3, vout3 = _arena(sub, inputs3["xs"], dt, cuda, 52)
        aout2.view(it).fill_(sb)
        _run_batch(sub, vin3, vout3, table)
        torch.cuda.synchronize()
        assert_guard_intact(aout3, vout3, name=key + " shorter")
        assert untouched(aout2), f"{key}: the shorter batch wrote to the previous batch's outputs"
        check_exact(key + "/shorter", qty3, {f"out{i}": v for i, v in enumerate(vout3)})
        _run_batch([], [], [], table)


# ---------------------------------------------------------------------------------------------- add, casts
@pytest.mark.parametrize("elem", ELEMS)
@pytest.mark.parametrize("case", R.ADD_CASES, ids=[f"{c[0]}x{c[1]}" for c in R.ADD_CASES])
def test_add(cuda, case, elem):
    from diffute_amd import ops
    rows, C = case
    inputs, qty = R.add_eval(case, elem)
    dt = R.ELEMS[elem]
    key = f"add/{rows}x{C}/{elem}"
    with ops.element_type(elem):
        a = wide(inputs["a"], dt, cuda, pad=16); b = wide(inputs["b"], dt, cuda, pad=24, seed=96)
        runs = []
        for _ in range(2):
            buf, out = poisoned((rows, C), dt, cuda)
            assert len({a.stride(0), b.stride(0), out.stride(0)}) == 3
            call("dmx_test_add_bf16", a, a.stride(0), b, b.stride(0), out, out.stride(0), rows, C)
            runs.append((buf, out))
        torch.cuda.synchronize()
    for buf, out in runs:
        assert_guard_intact(buf, out, name=key)
    same(key, [("out", runs[0][1], runs[1][1])])
    check_exact(key, qty, {"out": runs[0][1]})


@pytest.mark.parametrize("elem", ELEMS)
@pytest.mark.parametrize("case", R.CAST_CASES, ids=[f"{c[0]}x{c[1]}" for c in R.CAST_CASES])
@pytest.mark.parametrize("kind", R.CAST_KINDS)
def test_casts(cuda, kind, case, elem):
    from diffute_amd import ops
    M, C = case
    inputs, qty = R.cast_eval(kind, case, elem)
    dt = R.ELEMS[elem]
    key = f"{kind}/{M}x{C}/{elem}"
    with ops.element_type(elem):
        runs = []
        for _ in range(2):
            if kind == "slice_cast":
                x = wide(inputs["x"], torch.float32, cuda)               # the fp32 moments [M][2C], ldin = 2C + 16
                buf, out = poisoned((M, C), dt, cuda)
                call("dmx_test_slice_cast", x, x.stride(0), out, out.stride(0), M, C)
            elif kind == "mode_bwd":
                x = wide(inputs["x"], dt, cuda)
                buf, out = poisoned((M, 2 * C), torch.float32, cuda, pad_cols=0)      # dense output
                call("dmx_test_mode_bwd", x, x.stride(0), out, M, C)
            else:
                x = wide(inputs["x"], dt, cuda)
                buf, out = poisoned((M, C), torch.float32, cuda, pad_cols=0)
                call("dmx_test_bf16_to_f32_rows", x, x.stride(0), out, M, C)
            runs.append((buf, out))
        torch.cuda.synchronize()
    for buf, out in runs:
        assert_guard_intact(buf, out, name=key)
    same(key, [("out", runs[0][1], runs[1][1])])
    check_exact(key, qty, {"out": runs[0][1]})
    if kind == "mode_bwd":
        assert not bits(runs[0][1][:, C:]).any(), f"{key}: the log-variance half is not bit-zero"


# ---------------------------------------------------------------------------------------------- row softmax
@pytest.mark.parametrize("elem", ELEMS)
@pytest.mark.parametrize("case", R.SM_CASES, ids=[f"{c[0]}_{c[1]}x{c[2]}" for c in R.SM_CASES])
def test_softmax_rows(cuda, case, elem):
    from diffute_amd import ops
    pattern, rows, n = case
    inputs, qty = R.softmax_eval(case, elem)
    dt = R.ELEMS[elem]
    key = f"softmax/{pattern}_{rows}x{n}/{elem}"
    with ops.element_type(elem):
        s = wide(inputs["s"], torch.float32, cuda)
        runs = []
        for _ in range(2):
            buf, p = poisoned((rows, n), dt, cuda)
            call("dmx_test_softmax_rows", s, s.stride(0), p, p.stride(0), rows, n, R.SM_SCALE)
            runs.append((buf, p))
        torch.cuda.synchronize()
    for buf, p in runs:
        assert_guard_intact(buf, p, name=key)
    same(key, [("p", runs[0][1], runs[1][1])])
    check(key, qty, {"p": runs[0][1]})
    u = 2.0 ** -9 if elem == "bf16" else 2.0 ** -11                      # unit roundoff of the 16-bit element
    dev1 = float((host(runs[0][1]).sum(-1) - 1.0).abs().max())
    print(f"{key}:p row sums off 1 by {dev1:.3e}/{n * u:.2e}")
    assert dev1 <= n * u, f"{key}: a row of P sums to 1 -/+ {dev1:.3e} > n u = {n * u:.3e}"


def run_softmax_bwd(case, elem, dev, gscale=1.0):
    from diffute_amd import ops
    rows, n = case[:2]
    inputs, qty = R.softmax_bwd_eval(case, elem, gscale)
    dt = R.ELEMS[elem]
    key = f"softmax_bwd/{rows}x{n}/{elem}" + ("/gs" if gscale != 1.0 else "")
    with ops.element_type(elem):
        p = wide(inputs["p"], dt, dev); dp = wide(inputs["dp"], torch.float32, dev, pad=16, seed=96)
        runs = []
        for _ in range(2):
            buf, ds = poisoned((rows, n), dt, dev, pad_cols=24)
            assert len({p.stride(0), dp.stride(0), ds.stride(0)}) == 3
            call("dmx_test_softmax_bwd_rows", p, p.stride(0), dp, dp.stride(0), ds, ds.stride(0), rows, n, R.SM_SCALE)
            runs.append((buf, ds))
        torch.cuda.synchronize()
    for buf, ds in runs:
        assert_guard_intact(buf, ds, name=key)
    same(key, [("ds", runs[0][1], runs[1][1])])
    check(key, qty, {"ds": runs[0][1]})


@pytest.mark.parametrize("elem", ELEMS)
@pytest.mark.parametrize("case", R.SMB_CASES, ids=[f"{c[0]}x{c[1]}" for c in R.SMB_CASES])
def test_softmax_bwd_rows(cuda, case, elem):
    run_softmax_bwd(case, elem, cuda)


# ---------------------------------------------------------------------------------------------- 1x1 convolutions, <= 8 channels
def _pw_operands(inputs, Cin, Cout, dt, dev):
    x = wide(inputs["x"], dt, dev)
    wfull = (seeded((Cout, R.PW_LDW), 97) * 3.0).to(dev).to(dt)          # rows of the padded K of the real weights; junk behind Cin
    wfull[:, :Cin] = inputs["w"].to(dev).to(dt)
    return x, wfull, inputs["bias"].float().to(dev)


@pytest.mark.parametrize("elem", ELEMS)
@pytest.mark.parametrize("case", R.PW_CASES, ids=[f"{c[0]}to{c[1]}_m{c[2]}" for c in R.PW_CASES])
def test_pointwise_small_fwd(cuda, case, elem):
    from diffute_amd import ops
    Cin, Cout, M = case
    inputs, qty = R.pw_eval(case, elem)
    dt = R.ELEMS[elem]
    key = f"pw/{Cin}to{Cout}_m{M}/{elem}"
    got, guards, again = {}, [], []
    with ops.element_type(elem):
        x, w, bias = _pw_operands(inputs, Cin, Cout, dt, cuda)
        for name, b, f32 in (("y16", bias, 0), ("y32", bias, 1), ("y16_nobias", None, 0), ("y32_nobias", None, 1)):
            for rep in range(2):
                buf, y = poisoned((M, Cout), torch.float32 if f32 else dt, cuda)
                call("dmx_test_pointwise_small_fwd", x, x.stride(0), w, R.PW_LDW, b, y, y.stride(0), M, Cin, Cout, f32)
                guards.append((buf, y, name))
                if rep == 0: got[name] = y
                else: again.append((name, got[name], y))
        torch.cuda.synchronize()
    for buf, y, name in guards:
        assert_guard_intact(buf, y, name=f"{key} {name}")
    same(key, again)
    check(key, qty, got)


def run_pointwise_bwd(case, elem, dev, gscale=1.0):
    from diffute_amd import ops
    Cin, Cout, M = case
    inputs, qty = R.pw_eval(case, elem, gscale)
    dt = R.ELEMS[elem]
    key = f"pw/{Cin}to{Cout}_m{M}/{elem}" + ("/gs" if gscale != 1.0 else "")
    with ops.element_type(elem):
        x, w, _ = _pw_operands(inputs, Cin, Cout, dt, dev)
        dy = wide(inputs["dy"], torch.float32, dev, pad=16, seed=96)
        wsb = int(ops.lib().dmx_test_pointwise_small_bwd_workspace_bytes(M, Cin, Cout))
        assert wsb == (M + 255) // 256 * (Cout * Cin + Cout) * 4
        ws = torch.empty(wsb, dtype=torch.uint8, device=dev)
        runs = []
        for with_dx in (True, True, False):                          # twice in full, then dx = NULL: dw and db alone
            xb, dx = poisoned((M, Cin), dt, dev)
            wb, dw = poisoned((Cout, Cin), torch.float32, dev)
            bb, db = poisoned((Cout,), torch.float32, dev)
            call("dmx_test_pointwise_small_bwd", x, x.stride(0), dy, dy.stride(0), w, R.PW_LDW, dx if with_dx else None, dx.stride(0),
                 dw, dw.stride(0), db, M, Cin, Cout, ws, wsb)
            runs.append((xb, dx, wb, dw, bb, db))
        torch.cuda.synchronize()
    for i, (xb, dx, wb, dw, bb, db) in enumerate(runs):
        if i < 2: assert_guard_intact(xb, dx, name=f"{key} dx")
        else: assert untouched(xb), f"{key}: dx = NULL, yet its buffer was written"
        assert_guard_intact(wb, dw, name=f"{key} dw"); assert_guard_intact(bb, db, name=f"{key} db")
    same(key, [("dx", runs[0][1], runs[1][1])] + [(nm, runs[0][j], runs[i][j]) for i in (1, 2) for nm, j in (("dw", 3), ("db", 5))])
    check(key, {k: qty[k] for k in ("dx", "dw", "db")}, {"dx": runs[0][1], "dw": runs[0][3], "db": runs[0][5]})


@pytest.mark.parametrize("elem", ELEMS)
@pytest.mark.parametrize("case", R.PW_CASES, ids=[f"{c[0]}to{c[1]}_m{c[2]}" for c in R.PW_CASES])
def test_pointwise_small_bwd(cuda, case, elem):
    run_pointwise_bwd(case, elem, cuda)


@pytest.mark.parametrize("elem", ELEMS)
def test_pointwise_small_refusals(cuda, elem):
    """more than 8 input channels, and a backward workspace one byte short: refused on the host with a message, nothing launched,
    nothing written"""
    from diffute_amd import ops
    dt = R.ELEMS[elem]
    M = 300
    with ops.element_type(elem):
        x = torch.zeros(M, 32, dtype=dt, device=cuda); w = torch.zeros(8, R.PW_LDW, dtype=dt, device=cuda)
        dy = torch.zeros(M, 32, dtype=torch.float32, device=cuda)
        yb, y = poisoned((M, 8), dt, cuda)
        msg = refused("dmx_test_pointwise_small_fwd", x, 32, w, R.PW_LDW, None, y, y.stride(0), M, 9, 8, 0)
        print(f"pw/refusal/{elem}: Cin = 9 forward: {msg}")
        xb, dx = poisoned((M, 9), dt, cuda); wb, dw = poisoned((8, 9), torch.float32, cuda); bb, db = poisoned((8,), torch.float32, cuda)
        ws = torch.empty(1 << 16, dtype=torch.uint8, device=cuda)
        msg = refused("dmx_test_pointwise_small_bwd", x, 32, dy, 32, w, R.PW_LDW, dx, dx.stride(0), dw, dw.stride(0), db, M, 9, 8, ws, ws.numel())
        print(f"pw/refusal/{elem}: Cin = 9 backward: {msg}")
        need = int(ops.lib().dmx_test_pointwise_small_bwd_workspace_bytes(M, 8, 8))
        msg = refused("dmx_test_pointwise_small_bwd", x, 32, dy, 32, w, R.PW_LDW, dx, dx.stride(0), dw, dw.stride(0), db, M, 8, 8, ws, need - 1)
        print(f"pw/refusal/{elem}: workspace {need - 1} of {need} bytes: {msg}")
        torch.cuda.synchronize()
    for b in (yb, xb, wb, bb):
        assert untouched(b), "a refused call wrote to an output"


# ---------------------------------------------------------------------------------------------- backward of the small fp32 linears
@pytest.mark.parametrize("elem", ELEMS)
@pytest.mark.parametrize("case", R.LSB_CASES, ids=[R.lsb_name(c) for c in R.LSB_CASES])
def test_linear_small_bwd(cuda, case, elem):
    from diffute_amd import ops
    B, N, K, silu, dbs, which = case
    inputs, qty = R.lsb_eval(case, elem)
    dt = R.ELEMS[elem]
    key = f"lsb/{R.lsb_name(case)}/{elem}"
    want_dw, want_dx = which != "dx", which != "dw"
    f32 = torch.float32
    with ops.element_type(elem):
        x = wide(inputs["x"], f32, cuda); dy = wide(inputs["dy"], f32, cuda, pad=16, seed=96); w = wide(inputs["w"], dt, cuda, pad=24, seed=95)
        xa = x if (want_dw or silu) else None                         # dx alone without SiLU never reads x
        wb, dw = poisoned((N, K), f32, cuda)
        bbuf = torch.full((N * dbs + 16,), SENTINEL_BITS[f32][1], dtype=torch.int32, device=cuda).view(f32)
        db = bbuf[8:8 + N * dbs:dbs]
        xb, dx = poisoned((B, K), f32, cuda, pad_cols=16)
        call("dmx_test_linear_small_bwd", xa, x.stride(0), dy, dy.stride(0), w if want_dx else None, w.stride(0),
             dw if want_dw else None, dw.stride(0), db if want_dw else None, dbs, dx if want_dx else None, dx.stride(0), B, N, K, silu, 0)
        # a second run into fresh buffers: bit-identical
        wb2, dw2 = poisoned((N, K), f32, cuda)
        bbuf2 = torch.full((N * dbs + 16,), SENTINEL_BITS[f32][1], dtype=torch.int32, device=cuda).view(f32)
        db2 = bbuf2[8:8 + N * dbs:dbs]
        xb3, dx3 = poisoned((B, K), f32, cuda, pad_cols=16)
        call("dmx_test_linear_small_bwd", xa, x.stride(0), dy, dy.stride(0), w if want_dx else None, w.stride(0),
             dw2 if want_dw else None, dw2.stride(0), db2 if want_dw else None, dbs, dx3 if want_dx else None, dx3.stride(0), B, N, K, silu, 0)
        # accumulate = 1 onto a non-zero gradient (dense buffers; db at its stride): previous + fresh, one fp32 add each; dx is written as before
        prev_w = seeded((N, K), 7).to(cuda); prev_b = seeded((N,), 8).to(cuda)
        aw = prev_w.clone(); ab = torch.zeros(N * dbs, device=cuda); ab[::dbs] = prev_b
        xb2, dx2 = poisoned((B, K), f32, cuda)
        call("dmx_test_linear_small_bwd", xa, x.stride(0), dy, dy.stride(0), w if want_dx else None, w.stride(0),
             aw if want_dw else None, K, ab if want_dw else None, dbs, dx2 if want_dx else None, dx2.stride(0), B, N, K, silu, 1)
        torch.cuda.synchronize()
    got = {}
    if want_dw:
        assert_guard_intact(wb, dw, name=f"{key} dw"); assert_guard_intact(bbuf, db, name=f"{key} db")
        assert_guard_intact(wb2, dw2, name=f"{key} dw (second run)"); assert_guard_intact(bbuf2, db2, name=f"{key} db (second run)")
        same(key, [("dw", dw, dw2), ("db", db, db2)])
        assert torch.equal(bits(aw), bits(prev_w + dw)) and torch.equal(bits(ab[::dbs]), bits(prev_b + db)), f"{key}: accumulate != previous + fresh"
        if dbs > 1:
            assert not bits(ab.view(N, dbs)[:, 1:]).any(), f"{key}: db written between its strided elements"
        got["dw"] = dw; got["db"] = db
    else:
        assert untouched(wb) and untouched(bbuf) and untouched(wb2) and untouched(bbuf2), f"{key}: dw = NULL, yet dw / db were written"
    if want_dx:
        assert_guard_intact(xb, dx, name=f"{key} dx"); assert_guard_intact(xb3, dx3, name=f"{key} dx (second run)")
        assert_guard_intact(xb2, dx2, name=f"{key} dx (accumulate run)")
        same(key, [("dx", dx, dx3), ("dx", dx, dx2)])
        got["dx"] = dx
    else:
        assert untouched(xb) and untouched(xb2) and untouched(xb3), f"{key}: dx = NULL, yet dx was written"
    check(key, qty, got)


# ---------------------------------------------------------------------------------------------- gradient scaling (fp16 build)
@pytest.mark.parametrize("factor", R.GS_FACTORS, ids=["x1", "x2^10", "x2^16"])
@pytest.mark.parametrize("kernel", ["softmax_bwd", "pointwise_bwd"])
def test_fp16_gradient_scaling(cuda, kernel, factor):
    """as test_train_layout_gpu.py's: the upstream gradient ~ N(0, 2^-7) times the GradScaler factor; every factor meets the bounds of
    the factor-1 case and stays finite"""
    run, case = {"softmax_bwd": (run_softmax_bwd, R.SMB_GS_CASE), "pointwise_bwd": (run_pointwise_bwd, R.PW_GS_CASE)}[kernel]
    run(case, "fp16", cuda, gscale=R.GS_BASE * factor)
