"""Test-local restatement of transformers' teacher-forced scoring, `VisionEncoderDecoderModel(encoder_outputs=..., labels=...)`
over the model of app.ipynb:548: the labels shifted right (`shift_tokens_right`: start token first, -100 -> pad), the decoder's
teacher-forced forward (tests/trocr_restatement.forward), and torch's CrossEntropyLoss over the flattened batch.  fp32 torch on the
CPU; pinned against transformers by scripts/pin_trocr_score_oracle.py."""
import torch
import torch.nn.functional as F

import trocr_restatement as R

IGNORE = -100


def shift_tokens_right(labels, pad, start):
    ids = labels.new_zeros(labels.shape)
    ids[:, 1:] = labels[:, :-1]
    ids[:, 0] = start
    return ids.masked_fill(ids == IGNORE, pad)


def score(P, cfg, labels, enc, start, pad):
    """(decoder input ids, logits [B, T, V], per-token log-probs [B, T] with 0 at ignored positions, loss)"""
    ids = shift_tokens_right(labels, pad, start)
    logits = R.forward(P, cfg, ids, enc)
    keep = labels != IGNORE
    lp = F.log_softmax(logits.float(), -1).gather(-1, labels.masked_fill(~keep, 0)[..., None])[..., 0]
    lp = torch.where(keep, lp, torch.zeros_like(lp))
    loss = F.cross_entropy(logits.reshape(-1, logits.shape[-1]), labels.reshape(-1), ignore_index=IGNORE)   # NaN when every label is ignored
    return ids, logits, lp, loss
