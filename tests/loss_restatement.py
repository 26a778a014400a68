"""dmx_diffusion_loss (include/diffute_hip.h) restated in numpy, for tests/test_diffusion_loss_host.py and tests/test_diffusion_loss_gpu.py.

    restate       the float32 restatement: every line one rounded fp32 operation in the header's order -> dpred and the per-element terms
    fold          the loss from a [B, 5] record array, the header's serial fold in float32
    sums64        the per-sample sums in float64 from the same fp32 inputs
    snr_weights   the Min-SNR-gamma table, written from the paper's formula and not from diffute_amd/schedulers.py
    depth / bound the kernel's documented reduction shape and the error bound that follows from it
    verify        what the GPU test asserts of one call's outputs; the host test shows that it refuses six injected faults (model_kernel)

The float64 sums take the TARGET as the fp32 number the kernel forms (for a v model: the fp32 get_velocity tensor the plain objective
materialises, pinned bit for bit by its own test), and evaluate everything after it in float64: the objective is a function of pred and that
fp32 target, and only then is every term's relative error bounded - a float64 target would differ from the fp32 one by roundings relative
to |target|, not to |pred - target|.

The bound.  u = 2^-24.  Every term is non-negative and is computed from the fp32 target with r roundings:
    q = fl(fl(p - tau)^2)                                r = 2 + 1 = 3  (the rounding of d counts twice in d^2)      sq_all
    fl(M q)                                              r = 4                                                      sq_mask
    m = fl(1 + fl(lambda M)): 2 roundings;  fl(m q)      r = 2 + 3 + 1 = 6                                          sq_weighted
    M                                                    r = 0                                                      mask_sum
and passes through at most k additions (depth).  Hence |S32 - S64| <= ((1 + u)^(k + r) - 1) S64 <= n u / (1 - n u) S64 with n = k + r
(Higham, Accuracy and Stability of Numerical Algorithms, lemma 3.1).  The issue's "(k + 4) u S64" counted 4 roundings for every field; the
derivation gives 3 / 4 / 6 / 0, so sq_all and mask_sum are held to less and sq_weighted to the two more its factor m really costs."""
import numpy as np

F = np.float32
U = 2.0 ** -24
CHUNK = 2048                      # DMX_LOSS_CHUNK (the host test compares it with the header's)
FIELDS = ("sq_all", "sq_mask", "sq_weighted", "mask_sum", "weight")         # DMX_LOSS_SQ_ALL .. DMX_LOSS_WEIGHT
ROUNDINGS = dict(sq_all=3, sq_mask=4, sq_weighted=6, mask_sum=0)


def snr_weights(abar, snr_gamma, prediction_type):
    """float64 [T] from alphas_cumprod.  Hang et al. 2023, eq. (8)/(10) as diffusers' training scripts apply them."""
    abar = np.asarray(abar, np.float64)
    if snr_gamma is None:
        return np.ones_like(abar)
    snr = abar / (1 - abar)
    out = np.empty_like(abar)
    for i, s in enumerate(snr):
        top = s if s < snr_gamma else snr_gamma
        out[i] = top / s if prediction_type == "epsilon" else top / (s + 1)
    return out


def depth(span):
    """k: 8 serial adds per thread + an 8-level tree over 256 threads + the ceil(span / CHUNK) chunk sums added serially"""
    return 8 + 8 + -(-span // CHUNK)


def bound(k, roundings):
    n = k + roundings
    return n * U / (1 - n * U)


def _tables(case):
    t = np.asarray(case["t"], np.int64)
    T = len(case["sa"])
    ok = (t >= 0) & (t < T)
    tc = np.clip(t, 0, T - 1)
    w = np.where(ok, case["wt"][tc], F(np.nan)).astype(F)
    return tc, w


def _target32(case, tc):
    noise, x0 = case["noise"], case["x0"]
    if not case["v_prediction"]:
        return noise
    sa, sb = case["sa"][tc].astype(F)[:, None, None, None], case["sb"][tc].astype(F)[:, None, None, None]
    return (sa * noise).astype(F) - (sb * x0).astype(F)


def _mask(case):
    B, C, h, w = case["pred"].shape
    return np.zeros((B, 1, h, w), F) if case["mask"] is None else case["mask"].astype(F)


def restate(case, grad_scale=1.0):
    """-> dict(dpred, q, Mq, mq, M, weight), float32, each array one fp32 operation per line"""
    pred = case["pred"]
    B, C, h, w = pred.shape
    N = B * C * h * w
    tc, wgt = _tables(case)
    tau = _target32(case, tc)
    M = np.broadcast_to(_mask(case), pred.shape)
    lam = F(case["mask_weight"])
    with np.errstate(invalid="ignore"):
        d = (pred - tau).astype(F)
        q = (d * d).astype(F)
        m = (F(1) + (lam * M).astype(F)).astype(F)
        e = (wgt[:, None, None, None] * m).astype(F)
        gs = F(2.0 * float(grad_scale) / N)
        dpred = ((d * e).astype(F) * gs).astype(F)
    return dict(dpred=dpred, q=q, Mq=(M * q).astype(F), mq=(m * q).astype(F), M=np.ascontiguousarray(M), weight=wgt)


def fold(records, N):
    """the scalar loss from the records: acc = fadd(acc, fmul(weight[b], sq_weighted[b])) in row order, then fmul(acc, (float)(1.0 / N))"""
    acc = F(0)
    with np.errstate(invalid="ignore"):
        for r in np.asarray(records, F):
            acc = F(acc + F(r[4] * r[2]))
        return F(acc * F(1.0 / N))


def sums64(case):
    """float64 [B, 4]: sq_all, sq_mask, sq_weighted, mask_sum from the fp32 inputs (the target as the fp32 number, see the module docstring)"""
    pred = case["pred"]
    B = pred.shape[0]
    tc, _ = _tables(case)
    d = pred.astype(np.float64) - _target32(case, tc).astype(np.float64)
    q = d * d
    M = _mask(case).astype(np.float64)
    m = 1.0 + float(F(case["mask_weight"])) * M
    return np.stack([q.reshape(B, -1).sum(1), (M * q).reshape(B, -1).sum(1), (m * q).reshape(B, -1).sum(1), M.reshape(B, -1).sum(1)], 1)


def bits(a):
    return np.ascontiguousarray(np.asarray(a, F)).view(np.uint32)


def verify(case, dpred, records, loss, grad_scale=1.0):
    """the checks of one call: dpred bit for bit against restate(), each sum inside its bound against sums64(), the weight field bit for bit,
    the loss bit for bit against fold() of the records given.  dpred may be None (a loss-only call)."""
    pred = case["pred"]
    B, C, h, w = pred.shape
    r = restate(case, grad_scale)
    records = np.asarray(records, F)
    assert records.shape == (B, len(FIELDS)), records.shape
    if dpred is not None:
        both_nan = np.isnan(np.asarray(dpred, F)).reshape(-1) & np.isnan(r["dpred"]).reshape(-1)        # (a NaN's payload is not specified)
        bad = (bits(dpred).reshape(-1) != bits(r["dpred"]).reshape(-1)) & ~both_nan
        assert not bad.any(), f"dpred differs from the float32 restatement at {int(bad.sum())} of {bad.size} elements (first: {int(np.argmax(bad))})"
    want = sums64(case)
    k = depth(C * h * w)
    for f, name in enumerate(FIELDS[:4]):
        err = np.abs(records[:, f].astype(np.float64) - want[:, f])
        lim = bound(k, ROUNDINGS[name]) * want[:, f]
        assert (err <= lim).all(), f"{name}: |S32 - S64| = {err} exceeds (k={k} + {ROUNDINGS[name]}) u S64 = {lim}"
    nan = np.isnan(r["weight"])
    assert (np.isnan(records[:, 4]) == nan).all() and (bits(records[:, 4])[~nan] == bits(r["weight"])[~nan]).all(), \
        f"weight field {records[:, 4]} differs from the table's {r['weight']}"
    want_loss = fold(records, B * C * h * w)
    got = F(np.asarray(loss, F).reshape(-1)[0])
    assert (np.isnan(got) and np.isnan(want_loss)) or bits(got) == bits(want_loss), f"loss {got!r} differs from the fold of its own records {want_loss!r}"


def make_case(tables, shape, t, mask_kind, prediction_type="epsilon", snr_gamma=None, mask_weight=0.0, seed=0):
    """One call's inputs.  tables: dict(abar, sa, sb) - the scheduler's alphas_cumprod and its two fp32 coefficient tables, as numpy.
    mask_kind: None, "zero", "one" or "rect" (a rectangle that touches neither the first row nor the last column, one per sample)."""
    B, C, h, w = shape
    rng = np.random.default_rng(seed)
    pred, x0, noise = (rng.standard_normal(shape).astype(F) for _ in range(3))
    if mask_kind is None:
        mask = None
    else:
        mask = np.full((B, 1, h, w), 1 if mask_kind == "one" else 0, F)
        if mask_kind == "rect":
            for b in range(B):
                mask[b, 0, 1 + b % 2:max(h // 2 + b, 2 + b % 2), 0:max(w - 2 - b, 1)] = 1
    return dict(pred=pred, x0=x0, noise=noise, mask=mask, t=np.asarray(t, np.int64), abar=np.asarray(tables["abar"]), sa=np.asarray(tables["sa"], F),
                sb=np.asarray(tables["sb"], F), wt=snr_weights(tables["abar"], snr_gamma, prediction_type).astype(F), snr_gamma=snr_gamma,
                v_prediction=prediction_type == "v_prediction", mask_weight=float(mask_weight))


FAULTS = ("epsilon_weight_snr_plus_1", "no_min", "mask_not_broadcast", "lambda_outside_box", "v_target_swapped_signs", "normalise_by_hw")


def model_kernel(case, fault=None, grad_scale=1.0):
    """An honest host model of the entry - the terms in float32, each sum accumulated in float64 and rounded once - with one fault injected:
    -> (dpred, records, loss).  fault=None passes verify(); each of FAULTS must not."""
    c = dict(case)
    B, C, h, w = c["pred"].shape
    N = B * C * h * w
    if fault in ("epsilon_weight_snr_plus_1", "no_min"):
        snr = c["abar"].astype(np.float64) / (1 - c["abar"].astype(np.float64))
        g = c["snr_gamma"]
        c["wt"] = ((np.minimum(snr, g) / (snr + 1)) if fault == "epsilon_weight_snr_plus_1" else g / snr).astype(F)
    if fault == "mask_not_broadcast":                # the emphasis and the masked sum reach channel 0 only
        M = np.zeros(c["pred"].shape, F); M[:, :1] = _mask(c)
    elif fault == "lambda_outside_box":
        M = np.broadcast_to(F(1) - _mask(c), c["pred"].shape)
    else:
        M = np.broadcast_to(_mask(c), c["pred"].shape)
    tc, wgt = _tables(c)
    tau = _target32(c, tc)
    if fault == "v_target_swapped_signs":
        tau = (-tau).astype(F)
    norm = h * w if fault == "normalise_by_hw" else N
    lam = F(c["mask_weight"])
    d = (c["pred"] - tau).astype(F)
    q = (d * d).astype(F)
    m = (F(1) + (lam * M).astype(F)).astype(F)
    dpred = ((d * (wgt[:, None, None, None] * m).astype(F)).astype(F) * F(2.0 * grad_scale / norm)).astype(F)
    s = lambda a: a.astype(np.float64).reshape(B, -1).sum(1)      # noqa: E731
    Mq = (np.broadcast_to(_mask(c), q.shape) * q) if fault == "lambda_outside_box" else M * q
    records = np.stack([s(q), s(Mq.astype(F)), s((m * q).astype(F)), s(_mask(c)), wgt.astype(np.float64)], 1).astype(F)
    acc = F(0)
    for r in records:
        acc = F(acc + F(r[4] * r[2]))
    return dpred, records, F(acc * F(1.0 / norm))
