"""Shared helpers for the parity tests (the oracle is the checker, never the thing under test)."""
import torch


def bf(x):
    """round to bf16 and back (fp32 container)"""
    return x.to(torch.bfloat16).to(torch.float32)


def rel_l2(a, b):
    a = a.detach().float().cpu(); b = b.detach().float().cpu()
    return float((a - b).norm() / b.norm().clamp_min(1e-30))


def assert_close(hip, ref, tol, name=""):
    """relative L2 error of the HIP result vs the oracle <= tol, and everything finite."""
    h = hip.detach().float().cpu()
    assert h.shape == ref.shape, f"{name}: shape {tuple(h.shape)} vs {tuple(ref.shape)}"
    assert torch.isfinite(h).all(), f"{name}: non-finite values in HIP output"
    e = rel_l2(h, ref)
    assert e <= tol, f"{name}: rel-L2 {e:.3e} > {tol:.1e} (max abs diff {float((h - ref.float()).abs().max()):.3e})"
    return e


def seeded(shape, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(shape, generator=g) * scale


# ---------------------------------------------------------------------------- training gradients against the oracle
def oracle_unet_train_grads(model, cfg_oracle, x, t, ctx, target, emulate_bf16=False):
    """loss and parameter gradients of the oracle (torch autograd on the CPU restatement; with emulate_bf16 the forward
    rounds where the HIP path materialises bf16, the backward stays fp32 - casts are straight-through).  `model` is a model or its
    state_dict."""
    from oracle import unet as OU
    sd = model.state_dict() if hasattr(model, "state_dict") else model
    P = {k: v.detach().cpu().float().clone().requires_grad_(True) for k, v in sd.items()}
    with torch.enable_grad():
        pred = OU.unet_forward.__wrapped__(P, cfg_oracle, x.cpu(), t.cpu(), ctx.cpu(), emulate_bf16=emulate_bf16)
        loss = torch.mean((pred.float() - target.cpu().float()) ** 2)
        loss.backward()
    return float(loss.detach()), pred.detach(), {k: p.grad for k, p in P.items()}


def grad_errors(grads, ref, not_ranked=lambda k: False):
    """{name: gradient} against the oracle's -> (rel-L2 of the whole gradient vector, [(rel-L2, name)] worst first); parameters for which
    `not_ranked(name)` holds count in the whole vector but are left out of the ranking"""
    errs = []
    num = den = 0.0
    for k, gh in grads.items():
        assert gh is not None, f"no gradient for {k}"
        gh = gh.detach().float().cpu(); gr = ref[k]
        assert torch.isfinite(gh).all(), f"{k}: non-finite gradient"
        num += float((gh - gr).pow(2).sum()); den += float(gr.pow(2).sum())
        if not not_ranked(k):
            errs.append((rel_l2(gh, gr), k))
    errs.sort(reverse=True)
    return (num / den) ** 0.5, errs


# ---------------------------------------------------------------------------- local (per-slice) parity
def _slice_norms(hip, ref, dim):
    h = hip.detach().double().cpu(); r = ref.detach().double().cpu()
    keep = sorted(d % r.dim() for d in ((dim,) if isinstance(dim, int) else dim))
    red = [d for d in range(r.dim()) if d not in keep]
    num = (h - r).pow(2).sum(red).sqrt() if red else (h - r).abs()
    den = r.pow(2).sum(red).sqrt() if red else r.abs()
    return num, den


def slice_err(hip, ref, dim):
    """worst slice along `dim` (an int, or a tuple of dims that index the slices together) of
    ||h_s - r_s|| / max(||r_s||, rho), rho = RMS over slices of ||r_s||.  No slice is excluded: the floor rho keeps
    near-zero slices from dominating.  Returns (error, index of the worst slice)."""
    num, den = _slice_norms(hip, ref, dim)
    rho = float(den.pow(2).mean().sqrt())
    e = num / den.clamp_min(max(rho, 1e-300))
    i = int(e.argmax())
    idx = tuple(int(v) for v in torch.unravel_index(torch.tensor(i), e.shape)) if e.dim() else ()
    return float(e.flatten()[i]) if e.dim() else float(e), (idx[0] if len(idx) == 1 else idx)


def assert_close_slices(hip, ref, tol, dims, name=""):
    """slice_err <= tol on each listed dim (entries of `dims` are ints or tuples); reports the worst slice's index.
    Returns the worst error over the dims."""
    h = hip.detach().double().cpu()
    assert h.shape == ref.shape, f"{name}: shape {tuple(h.shape)} vs {tuple(ref.shape)}"
    assert torch.isfinite(h).all(), f"{name}: non-finite values in HIP output"
    worst = 0.0
    for d in dims:
        e, i = slice_err(h, ref, d)
        assert e <= tol, f"{name}: worst slice along dim {d} is index {i}: rel-L2 {e:.3e} > {tol:.1e}"
        worst = max(worst, e)
    return worst


# ---------------------------------------------------------------------------- poisoned outputs with guard bands
# a finite, distinctive bit pattern (not NaN, so isfinite checks stay meaningful): 0x7A5A is 2.8e35 in bf16 and 5.2e4
# in fp16, 0x7A5A5A5A is 2.8e35 in fp32 - far above every test output, so an unwritten element also fails parity
SENTINEL_BITS = {torch.bfloat16: (torch.int16, 0x7A5A), torch.float16: (torch.int16, 0x7A5A), torch.float32: (torch.int32, 0x7A5A5A5A)}


def poisoned(shape, dtype, dev, pad_rows=2, pad_cols=8):
    """an output buffer larger than the logical output [..., rows, cols] (a 1-D shape is one row), all of it filled with
    the sentinel: `pad_rows` rows before and after, `pad_cols` columns left and right.  Returns (buffer, logical view);
    the view's row stride is cols + 2 * pad_cols (keep pad_cols a multiple of 8: the kernels want 16-byte rows)."""
    shape = tuple(shape)
    lead, rows, cols = (shape[:-2], shape[-2], shape[-1]) if len(shape) > 1 else ((), 1, shape[0])
    it, bits = SENTINEL_BITS[dtype]
    buf = torch.full(lead + (rows + 2 * pad_rows, cols + 2 * pad_cols), bits, dtype=it, device=dev).view(dtype)
    view = buf[..., pad_rows:pad_rows + rows, pad_cols:pad_cols + cols]
    return buf, (view if len(shape) > 1 else view[0])


def assert_guard_intact(buf, view, sentinel=None, name=""):
    """every element of `buf` outside `view` (any view into it, or a list of views) still holds the sentinel - nothing was
    written out of range - and no element inside it does: every output element was written."""
    it, bits = SENTINEL_BITS[buf.dtype]
    bits = bits if sentinel is None else sentinel
    inside = torch.zeros(buf.numel(), dtype=torch.bool)
    for v in (view if isinstance(view, (list, tuple)) else [view]):
        off = (v.data_ptr() - buf.data_ptr()) // buf.element_size()
        torch.as_strided(inside, v.shape, v.stride(), off).fill_(True)
    raw = buf.detach().cpu().contiguous().view(it).flatten()
    hit = (raw != bits) & ~inside
    if hit.any():
        i = int(hit.nonzero()[0]); ld = buf.shape[-1]
        raise AssertionError(f"{name}: {int(hit.sum())} elements outside the output were overwritten, first at row {i // ld} column {i % ld} of the guarded buffer")
    left = (raw == bits) & inside
    assert not left.any(), f"{name}: {int(left.sum())} output elements were never written (first flat index {int(left.nonzero()[0])})"
