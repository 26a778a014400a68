"""fp64 restatement of the LoRA merge and of the adapter gradients (diffute_amd/csrc/lora.hip), written from the formulas:

    W'[n][k]   = W0[n][k] + sum_j s_j sum_p B_j[n][p] A_j[p][k]
    dA_j[p][k] = s_j sum_n B_j[n][p] dW[n][k]
    dB_j[n][p] = s_j sum_k dW[n][k] A_j[p][k]

together with the per-element error bounds an fp32 evaluation in ANY summation order satisfies (u = 2^-24):

    merge  |got - exact| <= (R + 3) u (|W0| + sum_j |s_j| sum_p |B_j||A_j|)      R = total number of rank terms
    dA     |got - exact| <= (N + 3) u |s| sum_n |B||dW|
    dB     |got - exact| <= (K + 3) u |s| sum_k |dW||A|

and honest fp32 evaluations in several orders (numpy float32, every operation rounded), used by the host test to show that fp32 stays inside
the bounds and that the injected faults leave them.  Inputs are float32 arrays; adapters are (A [r,K], B [N,r], s)."""
import numpy as np

U = 2.0 ** -24

# (N, K): a tail-only tile, one full tile, the full-size attn2.to_k, the largest attention projection
SHAPES = [(33, 7), (320, 320), (320, 1024), (1280, 1280)]
RANKS = [1, 3, 16, 64]


def make_case(N, K, ranks, seed, scales=None):
    """-> (W0 [N,K], [(A, B, s)]) float32, no exact zeros and nothing small enough to hide a fault"""
    g = np.random.default_rng(seed)
    W0 = (g.standard_normal((N, K)) * 0.05).astype(np.float32)
    ads = []
    for j, r in enumerate(ranks):
        A = (g.standard_normal((r, K)) / np.sqrt(K)).astype(np.float32)
        B = (g.standard_normal((N, r)) * 0.1).astype(np.float32)
        s = np.float32(scales[j] if scales is not None else (0.5 + 0.75 * j) * 8.0 / r)
        ads.append((A, B, s))
    return W0, ads


def make_dw(N, K, seed):
    return (np.random.default_rng(seed).standard_normal((N, K)) * 0.02).astype(np.float32)


# ---------------------------------------------------------------------------------------------- fp64
def merge64(W0, ads):
    out = W0.astype(np.float64)
    for A, B, s in ads:
        out = out + float(s) * (B.astype(np.float64) @ A.astype(np.float64))
    return out


def merge_bound(W0, ads):
    R = sum(A.shape[0] for A, _, _ in ads)
    mag = np.abs(W0.astype(np.float64))
    for A, B, s in ads:
        mag = mag + abs(float(s)) * (np.abs(B.astype(np.float64)) @ np.abs(A.astype(np.float64)))
    return (R + 3) * U * mag


def grads64(dW, A, B, s):
    """-> (dA [r,K], dB [N,r])"""
    d = dW.astype(np.float64)
    return float(s) * (B.astype(np.float64).T @ d), float(s) * (d @ A.astype(np.float64).T)


def grads_bound(dW, A, B, s):
    N, K = dW.shape
    d = np.abs(dW.astype(np.float64))
    return ((N + 3) * U * abs(float(s)) * (np.abs(B.astype(np.float64)).T @ d),
            (K + 3) * U * abs(float(s)) * (d @ np.abs(A.astype(np.float64)).T))


# ---------------------------------------------------------------------------------------------- fp32, every operation rounded
def _dot32(x, y, order):
    """sum_i x[..., i] * y[..., i] in float32: 'fwd' ascending, 'rev' descending, 'pair' a halving tree"""
    p = (x.astype(np.float32) * y.astype(np.float32)).astype(np.float32)
    n = p.shape[-1]
    if order == "pair":
        while p.shape[-1] > 1:
            if p.shape[-1] % 2:
                p = np.concatenate([p, np.zeros(p.shape[:-1] + (1,), np.float32)], -1)
            p = (p[..., 0::2] + p[..., 1::2]).astype(np.float32)
        return p[..., 0]
    acc = np.zeros(p.shape[:-1], np.float32)
    for i in (range(n) if order == "fwd" else range(n - 1, -1, -1)):
        acc = (acc + p[..., i]).astype(np.float32)
    return acc


ORDERS = ("fwd", "rev", "pair")


def merge32(W0, ads, order="fwd"):
    out = W0.astype(np.float32)
    for A, B, s in (ads if order != "rev" else ads[::-1]):
        dot = _dot32(B[:, None, :], A.T[None, :, :], order)                 # [N, K]
        out = (out + (np.float32(s) * dot).astype(np.float32)).astype(np.float32)
    return out


def grads32(dW, A, B, s, order="fwd"):
    dA = (np.float32(s) * _dot32(B.T[:, None, :], dW.T[None, :, :], order)).astype(np.float32)     # [r, K] over n
    dB = (np.float32(s) * _dot32(dW[:, None, :], A[None, :, :], order)).astype(np.float32)         # [N, r] over k
    return dA, dB


# ---------------------------------------------------------------------------------------------- the injected faults
def fault_merge(W0, ads, fault):
    """a wrong merge in fp64; `fault` in MERGE_FAULTS"""
    out = W0.astype(np.float64)
    for A, B, s in ads:
        A64, B64, s = A.astype(np.float64), B.astype(np.float64), float(s)
        if fault == "s_twice":
            s = s * s
        elif fault == "alpha_over_r_inverted":
            s = 1.0 / s
        elif fault == "dropped_last_rank":
            A64, B64 = A64[:-1], B64[:, :-1]
        term = s * (B64 @ A64)
        if fault == "a_b_transposed":                                       # (square targets only: B^T-shaped A and A^T-shaped B)
            term = s * (A64.T @ B64.T) if A64.shape[1] == B64.shape[0] else term * 0
        if fault == "dropped_tail_row":
            term[-1] = 0
        out = out + term
    return out


MERGE_FAULTS = ("s_twice", "alpha_over_r_inverted", "a_b_transposed", "dropped_last_rank", "dropped_tail_row")


def fault_grads(dW, A, B, s, fault):
    """wrong gradients in fp64; `fault` in GRAD_FAULTS"""
    d, A64, B64, s = dW.astype(np.float64), A.astype(np.float64), B.astype(np.float64), float(s)
    if fault == "s_twice":
        s = s * s
    elif fault == "alpha_over_r_inverted":
        s = 1.0 / s
    dA, dB = s * (B64.T @ d), s * (d @ A64.T)
    if fault == "dA_from_A":                                                # A where B belongs (the roles of the two factors swapped)
        dA = s * (A64 @ d) if d.shape[0] == d.shape[1] else dA * 0          # (A [r,K] fits dW's rows on square targets only)
    elif fault == "dropped_last_rank":
        dA[-1] = 0; dB[:, -1] = 0
    elif fault == "dropped_tail_row":
        dA = s * (B64[:-1].T @ d[:-1]); dB[-1] = 0
    return dA, dB


GRAD_FAULTS = ("s_twice", "alpha_over_r_inverted", "dA_from_A", "dropped_last_rank", "dropped_tail_row")
