"""The fused AdamW (csrc/optim.hip: build_chunks, dmx_sqnorm_part_kernel, dmx_clip_coef_kernel, dmx_adamw_kernel) through the C entries
dmx_unet_optim_table / dmx_unet_adamw_step[_scaled] alone: no backward, no FusedAdamW.  The arenas (masters, exp_avg, exp_avg_sq, ema,
grads) are the test's own, sentinel-filled outside the chunk table's ranges; the weights arena is the tiny UNet's.

Every optimizer step is compared PER ELEMENT with adamw_restatement.step64 (fp64) restarted from the state the kernel itself left, so
errors do not compound: p, exp_avg, exp_avg_sq and ema each within the rounding bound derived in adamw_restatement.py's docstring
(c u x the sum of the magnitudes of the expression's terms, c = 24 / 5 / 7 / 4 rounded operations; test_adamw_host.py shows on the same
inputs that an honest fp32 evaluation stays inside it and that swapped betas, bc2 for sqrt(bc2), eps inside the root, decay after the
update, clipping by the scaled norm, a dropped bc1 and an EMA of the old p do not).  On top of the bound, the fp32 restatement in the
kernel's order (step32) must match BIT FOR BIT: -ffp-contract=off and correctly rounded `/` and sqrtf make the kernel a sequence of single
IEEE operations (EXPERIMENTS.md records that it held on both builds).  Steps 1, 2, 3 and 1000; gradients log-uniform over 1e-8 .. 1e2.

The compute copies (the 16-bit / fp32 weights the kernel writes into the weights arena at the table's arena_off) are compared bit for
bit with the rounded p the kernel produced, every other byte of the weights arena with its snapshot."""

import numpy as np
import pytest
import torch

import adamw_restatement as A
from util import SENTINEL_BITS

pytestmark = pytest.mark.gpu
ELEMS = ["bf16", "fp16"]
TINY_UNET = dict(block_out_channels=(64, 128, 256, 256), attention_head_dim=(1, 2, 4, 4), cross_attention_dim=128)      # test_models_gpu.py's
SENT = SENTINEL_BITS[torch.float32][1]
CHUNK_DT = np.dtype([("index", "<u8"), ("count", "<u4"), ("is_bf16", "<u4"), ("arena_off", "<u8")])
_RIGS = {}
_INPUTS = {}


class Rig:
    """one tiny UNet on one build, its chunk table read back, and the index maps between the packed fp32 arenas (compact order: the
    table's elements in ascending arena order) and the weights arena"""

    def __init__(self, elem, dev):
        import diffute_amd as D
        from diffute_amd import _cabi
        self.elem, self.dev = elem, dev
        self.dt = _cabi.torch_elem(elem)
        u = D.UNet2DConditionModel(**TINY_UNET).cuda().requires_grad_(False)
        if elem == "fp16":
            u.to(dtype=torch.float16)
        u._ensure_packed()
        self.unet, self.lib, self.h = u, u._lib, u._h
        lib = self.lib
        self.nchunks = int(lib.dmx_unet_optim_chunks(self.h))
        self.table = torch.zeros(int(lib.dmx_unet_optim_table_bytes(self.h)), dtype=torch.uint8, device=dev)
        _cabi.check(lib.dmx_unet_optim_table(self.h, _cabi.ptr(self.table), self.table.numel(), _cabi.current_stream()), "optim_table", lib)
        torch.cuda.synchronize()
        self.chunks = np.frombuffer(self.table.cpu().numpy().tobytes(), dtype=CHUNK_DT)
        self.nfloats = int(lib.dmx_unet_grad_bytes(self.h)) // 4
        c = self.chunks
        idx, cnt = c["index"].astype(np.int64), c["count"].astype(np.int64)
        assert (idx + cnt <= self.nfloats).all() and (cnt > 0).all(), "a chunk leaves the packed arena"            # before anything indexes with it
        delta = np.zeros(self.nfloats + 1, dtype=np.int32)
        np.add.at(delta, idx, 1); np.add.at(delta, idx + cnt, -1)
        self.cover = torch.from_numpy(np.cumsum(delta[:-1], dtype=np.int32)).to(dev)                                 # chunks covering each arena element
        self.in_table = self.cover > 0
        self.N = int(cnt.sum())
        order = np.argsort(idx, kind="stable")
        start = np.zeros(len(c), dtype=np.int64); start[order] = np.concatenate([[0], np.cumsum(cnt[order])[:-1]])
        is16 = np.repeat(c["is_bf16"][order] != 0, cnt[order])
        within = np.arange(self.N, dtype=np.int64) - np.repeat(start[order], cnt[order])
        off = np.repeat(c["arena_off"][order].astype(np.int64), cnt[order]) + within * np.where(is16, 2, 4)          # byte in the weights arena
        self.is16 = torch.from_numpy(is16).to(dev)
        off = torch.from_numpy(off).to(dev)
        self.idx16 = off[self.is16] // 2
        self.idx32 = off[~self.is16] // 4
        self.off_ok = bool((off[self.is16] % 2 == 0).all() and (off[~self.is16] % 4 == 0).all())
        self.arena_bytes = u._arena.numel()
        # the elements master_import writes: all-ones parameters into a zeroed arena
        ones = u._import_arena([torch.ones_like(p) for p in u._param_list()])
        torch.cuda.synchronize()
        self.real = ones != 0
        self.ones = ones

    def gather(self, arena):
        return arena[self.in_table]

    def fresh(self, values=None):
        """a sentinel-filled packed arena with `values` (compact order) at the table's elements"""
        a = torch.full((self.nfloats,), SENT, dtype=torch.int32, device=self.dev).view(torch.float32)
        if values is not None:
            a[self.in_table] = values
        return a

    def outside_untouched(self, arena):
        return bool((arena.view(torch.int32)[~self.in_table] == SENT).all())

    def expected_weights(self, snapshot, p_new):
        """the weights arena after a step: the snapshot with the rounded p_new (compact) at the table's arena_off"""
        e = snapshot.clone()
        e.view(torch.int16)[self.idx16] = p_new[self.is16].to(self.dt).view(torch.int16)
        e.view(torch.int32)[self.idx32] = p_new[~self.is16].view(torch.int32)
        return e


def rig_for(elem, dev):
    if elem not in _RIGS:
        _RIGS[elem] = Rig(elem, dev)
    return _RIGS[elem]


def inputs_for(rig):
    """the GPU test's inputs in compact order (shared by both builds): parameters, EMA shadow and one gradient per step, zero at the row
    paddings (table elements no parameter maps to)"""
    key = rig.N
    if key not in _INPUTS:
        p0, e0 = A.gen_params(rig.N)
        _INPUTS[key] = dict(p=p0, e=e0, g={t: A.gen_grad(rig.N, t) for t in A.STEPS})
    keep = rig.gather(rig.real).to(torch.float32)
    i = _INPUTS[key]
    return dict(p=i["p"].to(rig.dev) * keep, e=i["e"].to(rig.dev) * keep, g={t: g.to(rig.dev) * keep for t, g in i["g"].items()})


@pytest.fixture(scope="module")
def cuda():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda")


def garbage_grads(rig, g_compact):
    """the gradient arena: large finite garbage outside the table's ranges (its square overflows fp32: a norm that read it would be inf)"""
    a = torch.full((rig.nfloats,), 3e30, dtype=torch.float32, device=rig.dev)
    a[1::2] = -3e30
    a[rig.in_table] = g_compact
    return a


class State:
    def __init__(self, rig, p, e):
        self.rig = rig
        self.p, self.m, self.v = rig.fresh(p), rig.fresh(torch.zeros_like(p)), rig.fresh(torch.zeros_like(p))
        self.ema = None if e is None else rig.fresh(e)
        it = torch.int32
        self.scal_buf = torch.full((16,), SENT, dtype=it, device=rig.dev).view(torch.float32); self.scal = self.scal_buf[4:7]
        self.ws_buf = torch.full((rig.nchunks + 16,), SENT, dtype=it, device=rig.dev).view(torch.float32); self.ws = self.ws_buf[8:8 + rig.nchunks]

    def arenas(self):
        return [a for a in (self.p, self.m, self.v, self.ema) if a is not None]

    def compact(self):
        r = self.rig
        return dict(p=r.gather(self.p), m=r.gather(self.m), v=r.gather(self.v), ema=None if self.ema is None else r.gather(self.ema))

    def clone(self):
        s = State.__new__(State); s.rig = self.rig
        s.p, s.m, s.v = self.p.clone(), self.m.clone(), self.v.clone()
        s.ema = None if self.ema is None else self.ema.clone()
        s.scal_buf = torch.full_like(self.scal_buf.view(torch.int32), SENT).view(torch.float32); s.scal = s.scal_buf[4:7]
        s.ws_buf = torch.full_like(self.ws_buf.view(torch.int32), SENT).view(torch.float32); s.ws = s.ws_buf[8:8 + self.rig.nchunks]
        return s

    def step(self, grads, hp, t, max_norm, decay, inv_scale=None):
        from diffute_amd import _cabi
        r = self.rig
        head = (r.h, _cabi.ptr(r.table), r.nchunks, _cabi.ptr(self.p), _cabi.ptr(self.m), _cabi.ptr(self.v), _cabi.ptr(grads),
                hp["lr"], hp["b1"], hp["b2"], hp["eps"], hp["wd"], t, max_norm, _cabi.ptr(self.scal), _cabi.ptr(self.ws), r.nchunks * 4,
                _cabi.ptr(self.ema), decay)
        if inv_scale is None:
            _cabi.check(r.lib.dmx_unet_adamw_step(*head, _cabi.current_stream()), "adamw_step", r.lib)
        else:
            _cabi.check(r.lib.dmx_unet_adamw_step_scaled(*head, inv_scale, _cabi.current_stream()), "adamw_step_scaled", r.lib)
        _cabi.synchronize()
        return [float(x) for x in self.scal.cpu()]

    def guards_ok(self, wrote_found):
        sb = self.scal_buf.view(torch.int32).cpu(); wb = self.ws_buf.view(torch.int32).cpu()
        n = self.rig.nchunks
        ok = bool((sb[:4] == SENT).all() and (sb[(7 if wrote_found else 6):] == SENT).all() and (wb[:8] == SENT).all() and (wb[8 + n:] == SENT).all())
        return ok and all(self.rig.outside_untouched(a) for a in self.arenas())


def bits_equal(a, b):
    return torch.equal(a.view(torch.int32), b.view(torch.int32))


def checked_step(rig, st, g_compact, cfg, t, key, scaled_twin=None):
    """one step of `st` on gradient g_compact under configuration cfg, every check of the module docstring; returns the figures"""
    mult, wd, decay, scale = cfg
    hp = A.hyper(wd)
    inv_scale = None if scale is None else 1.0 / scale
    s_ = 1.0 if inv_scale is None else inv_scale
    g_arena_c = g_compact if scale is None else g_compact * scale                 # a power of two: exact
    grads = garbage_grads(rig, g_arena_c)
    grads_before = grads.clone()
    norm = A.grad_norm64(g_arena_c, s_)
    max_norm = A.f32(mult * norm)
    restated = A.clip_coef(norm, max_norm) * s_
    dec = 0.0 if decay is None else A.f32(decay)
    pre = st.compact()
    snap = rig.unet._arena.clone()
    scal = st.step(grads, hp, t, max_norm, dec, inv_scale)
    got = st.compact()
    assert st.guards_ok(inv_scale is not None), f"{key}: a sentinel outside the table's ranges (or around scalars / workspace) was overwritten"
    assert bits_equal(grads, grads_before), f"{key}: the gradient arena was written"
    print(f"{key}: norm {scal[0]:.8e} vs fp64 {norm:.8e}, factor {scal[1]:.8e} vs restated {restated:.8e}")
    assert abs(scal[0] - norm) <= A.COEF_TOL * norm, f"{key}: scalars[0] {scal[0]!r} vs the fp64 norm over the table's elements {norm!r}"
    assert abs(scal[1] - restated) <= A.COEF_TOL * restated, f"{key}: scalars[1] {scal[1]!r} vs the restated factor {restated!r}"
    if mult == 0.0 or mult > 1.0:
        assert scal[1] == A.f32(s_), f"{key}: no clipping asked for / needed, the coefficient must be exactly 1 (factor {scal[1]!r})"
    if inv_scale is not None:
        assert scal[2] == 0.0, f"{key}: found_inf set on a finite gradient"
    ratios, ref, bnd = A.check_step(got, pre, g_arena_c, scal[1], restated, hp, t, dec)
    print(f"{key}: worst |error| / bound " + " ".join(f"{k} {v[0]:.3f}@{v[1]}" for k, v in ratios.items()))
    for k, (ratio, i) in ratios.items():
        assert ratio <= 1.0, f"{key}: {k} is {ratio:.3f} x its bound at compact element {i}"
    # the kernel's order in fp32, one IEEE operation at a time: bit for bit (on the device, and on the CPU for every 16th element and both ends)
    s32 = A.step32(pre["p"], pre["m"], pre["v"], g_arena_c, pre["ema"], scal[1], hp["lr"], hp["b1"], hp["b2"], hp["eps"], hp["wd"], t, dec)
    sel = torch.cat([torch.arange(0, 4096), torch.arange(4096, rig.N - 4096, 16), torch.arange(rig.N - 4096, rig.N)]).to(rig.dev)
    c = lambda x: None if x is None else x[sel].cpu()
    c32 = A.step32(c(pre["p"]), c(pre["m"]), c(pre["v"]), c(g_arena_c), c(pre["ema"]), scal[1], hp["lr"], hp["b1"], hp["b2"], hp["eps"], hp["wd"], t, dec)
    diff = {k: (int((got[k].view(torch.int32) != s32[k].view(torch.int32)).sum()), int((got[k][sel].cpu().view(torch.int32) != c32[k].view(torch.int32)).sum()))
            for k in ("p", "m", "v", "ema") if got[k] is not None}
    print(f"{key}: elements differing from the same-order fp32 restatement (device, CPU sample of {sel.numel()}): {diff}")
    for k, (nd, nc) in diff.items():
        assert nd == 0 and nc == 0, f"{key}: {k} differs from the same-order fp32 restatement in {nd} elements (device) / {nc} (CPU sample)"
    assert rig.off_ok
    assert torch.equal(rig.unet._arena, rig.expected_weights(snap, got["p"])), f"{key}: the weights arena is not the snapshot + the rounded new parameters at arena_off"
    if scaled_twin is not None:                 # the unscaled call on the same state and gradient: the scaled one lands inside the same bound around ITS reference
        tw_ratios = A.worst_ratios(got, scaled_twin["ref"], scaled_twin["bnd"])
        print(f"{key}: scaled call vs the unscaled call's reference " + " ".join(f"{k} {v[0]:.3f}" for k, v in tw_ratios.items()))
        for k, (ratio, i) in tw_ratios.items():
            assert ratio <= 1.0, f"{key}: scaled {k} is {ratio:.3f} x the bound around the unscaled reference at compact element {i}"
        assert abs(scal[0] - scaled_twin["scal"][0]) <= 2 * A.COEF_TOL * norm
    return dict(ref=ref, bnd=bnd, scal=scal, ratios=ratios)


# ---------------------------------------------------------------------------------------------- chunk table
@pytest.mark.parametrize("elem", ELEMS)
def test_chunk_table(cuda, elem):
    from diffute_amd import _cabi
    rig = rig_for(elem, cuda)
    lib, c = rig.lib, rig.chunks
    assert len(c) == rig.nchunks and rig.table.numel() == 24 * rig.nchunks and CHUNK_DT.itemsize == 24
    idx, cnt = c["index"].astype(np.int64), c["count"].astype(np.int64)
    assert ((cnt > 0) & (cnt <= 65536)).all()
    assert (idx[1:] >= idx[:-1] + cnt[:-1]).all(), "chunks are not sorted and disjoint"
    assert int(rig.cover.max()) == 1
    assert int(lib.dmx_unet_optim_elements(rig.h)) == int(cnt.sum()) == rig.N
    assert set(np.unique(c["is_bf16"])) == {0, 1}
    esz = np.where(c["is_bf16"] != 0, 2, 4)
    assert (c["arena_off"].astype(np.int64) + cnt * esz <= rig.arena_bytes).all() and rig.off_ok
    assert (cnt < 65536).any(), "no ragged chunk in this configuration"
    # the compute copies of different elements never overlap
    use = torch.zeros(rig.arena_bytes // 2, dtype=torch.int32, device=cuda)
    one16 = torch.ones(rig.idx16.numel(), dtype=torch.int32, device=cuda); one32 = torch.ones(rig.idx32.numel(), dtype=torch.int32, device=cuda)
    use.index_add_(0, rig.idx16, one16); use.index_add_(0, rig.idx32 * 2, one32); use.index_add_(0, rig.idx32 * 2 + 1, one32)
    assert int(use.max()) == 1
    # every element master_import writes lies in exactly one chunk; what the table covers beyond them are row paddings: zero in the model's masters
    assert bool((rig.ones[rig.real] == 1.0).all())
    assert bool((rig.cover[rig.real] == 1).all()), "a parameter element outside the chunk table"
    assert int(rig.real.sum()) == sum(p.numel() for p in rig.unet.parameters())
    pad = rig.in_table & ~rig.real
    masters = rig.unet._import_arena(rig.unet._param_list())
    torch.cuda.synchronize()
    assert 0 < int(pad.sum()) < rig.N // 100 and bool((masters.view(torch.int32)[pad] == 0).all())
    # a table buffer one byte short is refused and not written
    small = torch.full((rig.table.numel(),), 0x5A, dtype=torch.uint8, device=cuda)
    rc = lib.dmx_unet_optim_table(rig.h, _cabi.ptr(small), small.numel() - 1, _cabi.current_stream())
    torch.cuda.synchronize()
    assert rc != 0 and lib.dmx_last_error() and bool((small == 0x5A).all())


# ---------------------------------------------------------------------------------------------- optimizer steps
@pytest.mark.parametrize("elem", ELEMS)
@pytest.mark.parametrize("config", list(A.CONFIGS))
def test_steps(cuda, elem, config):
    rig = rig_for(elem, cuda)
    cfg = A.CONFIGS[config]
    inp = inputs_for(rig)
    st = State(rig, inp["p"], None if cfg[2] is None else inp["e"])
    for t in A.STEPS:
        key = f"adamw/{config}/t{t}/{elem}"
        twin = None
        if cfg[3] is not None:
            tw = st.clone()
            twin = checked_step(rig, tw, inp["g"][t], cfg[:3] + (None,), t, key + "/unscaled")
            tw = None
        checked_step(rig, st, inp["g"][t], cfg, t, key, scaled_twin=twin)


@pytest.mark.parametrize("elem", ELEMS)
def test_overflowed_gradient_skips_the_step(cuda, elem):
    """GradScaler's contract on the scaled entry: an inf / NaN anywhere in the table's ranges sets scalars[2] and leaves all four fp32
    arenas and the weights arena bit-identical; the clean step after it clears the flag and updates as usual"""
    rig = rig_for(elem, cuda)
    cfg = A.CONFIGS["scaled_clip_wd_ema"]
    mult, wd, decay, scale = cfg
    hp = A.hyper(wd)
    inp = inputs_for(rig)
    st = State(rig, inp["p"], inp["e"])
    c = rig.chunks
    ragged = [i for i in range(len(c)) if c["count"][i] < 65536]
    fp32 = [i for i in range(len(c)) if c["is_bf16"][i] == 0]
    assert ragged and fp32
    last, f = c[ragged[-1]], c[fp32[len(fp32) // 2]]
    cases = [("+inf, last element of the ragged last chunk", int(last["index"] + last["count"] - 1), float("inf")),
             ("NaN in an fp32 chunk", int(f["index"] + f["count"] // 2), float("nan")),
             ("-inf, element 0 of chunk 0", int(c["index"].min()), float("-inf"))]
    for t, (what, pos, bad) in zip((1, 2, 3), cases):
        assert bool(rig.real[pos]), "the poisoned element must be a parameter element"
        key = f"adamw/overflow/{what}/{elem}"
        grads = garbage_grads(rig, inp["g"][t] * scale)
        grads[pos] = bad
        before = [a.clone() for a in st.arenas()]
        snap = rig.unet._arena.clone()
        norm = A.grad_norm64(inp["g"][t])
        scal = st.step(grads, hp, t, A.f32(mult * norm), A.f32(decay), 1.0 / scale)
        assert scal[2] == 1.0, f"{key}: scalars[2] = {scal[2]!r}"
        for a, b in zip(st.arenas(), before):
            assert bits_equal(a, b), f"{key}: an fp32 arena changed in a skipped step"
        assert torch.equal(rig.unet._arena, snap), f"{key}: the weights arena changed in a skipped step"
        assert st.guards_ok(True)
        checked_step(rig, st, inp["g"][t], cfg, t, key + "/clean step after")        # scalars[2] == 0 and a normal update
    # the unscaled entry does not touch scalars[2]
    st.scal_buf.view(torch.int32).fill_(SENT)
    st.step(garbage_grads(rig, inp["g"][1]), hp, 4, 0.0, A.f32(decay))
    assert st.guards_ok(False)
