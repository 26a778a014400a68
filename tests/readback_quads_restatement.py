"""The quad read-back and the quad select-paste restated in numpy BY COMPOSITION of what the other restatements already state
(include/diffute_hip.h, "Verified edits for quads"): nothing here samples, rounds or resamples on its own.
  read-back   row (b, k) = pil_resample_restatement.pixel_values of rectify of paste_page with a ONE-quad list - candidate k of quad b
              pasted alone over the original page, the quad's strip taken from that page.  pm None: the similarity frame
              (quad_restatement), else the projective one (persp_restatement).
  select      choice by readback_restatement.select; the paste is paste_page over the quads that were NOT skipped, in table order - a
              skipped quad is transparent, which is what dropping it from the list means -, the union mask the OR of ALL quads."""
import numpy as np

import persp_restatement as PR
import pil_resample_restatement as R
import quad_restatement as QR
import readback_restatement as RR


def pasted_alone(page, q, vae, S, pm=None):
    """the page with the decoder output `vae` [3][S][S] of quad q pasted on it, nothing else"""
    return (QR.paste_page(page, [q], [vae], S) if pm is None else PR.paste_page(page, [q], [pm], [vae], S))["out"]


def rectify(page, q, pm=None):
    return QR.rectify(page, q) if pm is None else PR.rectify(page, q, pm)


def strip(page, q, vae, S, pm=None):
    """uint8 [rh][rw][3]: what the OCR model is shown of candidate `vae` of quad q, before the processor"""
    return rectify(pasted_alone(page, q, vae, S, pm), q, pm)


def readback(page, q, vae, S, size, resample, pm=None):
    """-> (resized uint8 [3][h][w], pixel_values fp32 [3][h][w]); size = (height, width)"""
    return R.pixel_values(np.ascontiguousarray(strip(page, q, vae, S, pm)), size, resample)


def select_paste(page, qs, vaes, scores, threshold, S, pms=None):
    """One page: its quads `qs` in table order, vaes [n][K][3][S][S], scores [n][K] -> dict(out, union, choice)"""
    choice = RR.select(scores, threshold)
    kept = [b for b in range(len(qs)) if choice[b] >= 0]
    rows = [vaes[b][choice[b]] for b in kept]
    if not kept:
        out = page.copy()
    elif pms is None:
        out = QR.paste_page(page, [qs[b] for b in kept], rows, S)["out"]
    else:
        out = PR.paste_page(page, [qs[b] for b in kept], [pms[b] for b in kept], rows, S)["out"]
    H, W, _ = page.shape
    Y, X = np.meshgrid(np.arange(H, dtype=np.int64), np.arange(W, dtype=np.int64), indexing="ij")
    union = np.zeros((H, W), np.uint8)
    for q in qs:
        union |= QR.inside(q, X, Y).astype(np.uint8)
    return dict(out=out, union=union, choice=choice)
