"""Test-local restatement of transformers' beam search (`GenerationMixin._beam_search`, the vectorised version of 5.x) for the
OCR read-back (app.ipynb:845 with a checkpoint's own num_beams / length_penalty / early_stopping), specialised to
do_sample=False, no logits processors, one eos id (or none) and a decoder prompt of one token.  fp32 torch on the CPU.

`beam_step` is one step's bookkeeping on given log-probs; `beam_search` runs it over trocr_restatement's forward.  Every
selection orders by (larger score first, equal scores -> lower flat index, NaN never first): the rule is spelled out with a
stable sort instead of relying on torch.topk's choice among ties."""
import torch
import torch.nn.functional as F

import trocr_restatement as R

NEG = -1.0e9


def topk_ordered(x, k):
    """values, indices of the k best along the last dim: descending, ties -> lower index, NaN last"""
    key = torch.where(torch.isnan(x), torch.full_like(x, float("-inf")), x)
    # NaN must lose against a real -inf too: sort NaN entries after everything else by a second stable pass
    idx = torch.sort(key, dim=-1, descending=True, stable=True).indices
    nan_sorted = torch.gather(torch.isnan(x), -1, idx)
    idx = torch.gather(idx, -1, torch.sort(nan_sorted.to(torch.int8), dim=-1, stable=True).indices)[..., :k]
    return torch.gather(x, -1, idx), idx


def init_state(B, nb, max_length, start, fill):
    seq = torch.full((B, nb, max_length), int(fill), dtype=torch.int64)
    seq[:, :, 0] = int(start)
    run_scores = torch.zeros(B, nb)
    run_scores[:, 1:] = NEG
    return dict(cur_len=1, run_seq=seq, run_scores=run_scores, fin_seq=seq.clone(), fin_scores=torch.full((B, nb), NEG),
                fin_flags=torch.zeros(B, nb, dtype=torch.bool), fin_len=torch.zeros(B, nb, dtype=torch.int64),
                improvable=torch.ones(B, dtype=torch.bool), go=True)


def beam_step(state, logp, max_length, eos, length_penalty, early_stopping):
    """one step on log-probs [B * nb, V] (fp32); returns the new state and, per item, the K = 2 nb candidates (score, parent,
    token, hit) and the parent / token of every new running row"""
    s = state
    B, nb = s["run_scores"].shape
    V = logp.shape[-1]
    K = 2 * nb
    cur = s["cur_len"]
    acc = (logp.view(B, nb, V) + s["run_scores"][:, :, None]).reshape(B, nb * V)          # one fp32 add
    cand, flat = topk_ordered(acc, K)
    parent, token = flat // V, flat % V
    hits = torch.full_like(token, cur + 1 >= max_length, dtype=torch.bool)
    if eos is not None:
        hits = hits | (token == int(eos))
    cand_seq = torch.gather(s["run_seq"], 1, parent[:, :, None].expand(B, K, s["run_seq"].shape[2])).clone()
    cand_seq[:, :, cur] = token
    # the next running beams
    pen = cand + hits.to(torch.float32) * NEG
    run_scores, sel = topk_ordered(pen, nb)
    run_seq = torch.gather(cand_seq, 1, sel[:, :, None].expand(B, nb, cand_seq.shape[2]))
    new_parent, new_token = torch.gather(parent, 1, sel), torch.gather(token, 1, sel)
    # the finished set
    did = hits & (torch.arange(K) < nb)[None]
    sc = cand / (cur ** length_penalty)
    sc = sc + (s["fin_flags"].all(-1, keepdim=True) & (early_stopping is True)).to(torch.float32) * NEG
    sc = sc + (~s["improvable"])[:, None].to(torch.float32) * NEG
    sc = sc + (~did).to(torch.float32) * NEG
    m_scores = torch.cat([s["fin_scores"], sc], 1)
    m_flags = torch.cat([s["fin_flags"], did], 1)
    m_seq = torch.cat([s["fin_seq"], cand_seq], 1)
    m_len = torch.cat([s["fin_len"], torch.full((B, K), cur, dtype=torch.int64)], 1)
    fin_scores, mi = topk_ordered(m_scores, nb)
    fin_flags, fin_len = torch.gather(m_flags, 1, mi), torch.gather(m_len, 1, mi)
    fin_seq = torch.gather(m_seq, 1, mi[:, :, None].expand(B, nb, m_seq.shape[2]))
    # advance: can the running beams still improve on the finished ones?
    cur2 = cur + 1
    h = max_length - 1 if (early_stopping == "never" and length_penalty > 0.0) else cur2 - 1
    best = run_scores[:, :1] / (h ** length_penalty)
    worst = torch.where(fin_flags, fin_scores.min(1, keepdim=True).values, torch.full_like(fin_scores, NEG))
    improvable = s["improvable"] & (best > worst).any(-1)
    go = bool(improvable.any()) and not (bool(fin_flags.all()) and early_stopping is True) and not bool(hits.all())
    new = dict(cur_len=cur2, run_seq=run_seq, run_scores=run_scores, fin_seq=fin_seq, fin_scores=fin_scores, fin_flags=fin_flags,
               fin_len=fin_len, improvable=improvable, go=go)
    info = dict(cand=cand, parent=parent, token=token, hits=hits, new_parent=new_parent, new_token=new_token, acc=acc)
    return new, info


def finalize(state, num_return_sequences):
    """sequences [B * nret, L] cropped to 1 + the longest generated length among the returned rows, and their scores"""
    B, nb = state["fin_scores"].shape
    n = num_return_sequences
    L = 1 + int(state["fin_len"][:, :n].max())
    return state["fin_seq"][:, :n, :L].reshape(B * n, L), state["fin_scores"][:, :n].reshape(B * n)


def gap(info, K):
    """smallest difference between adjacent candidates among each item's top K + 1 accumulated scores (dead beams' -1e9 apart)"""
    v = topk_ordered(info["acc"], K + 1)[0]
    d = v[:, :-1] - v[:, 1:]
    live = v[:, 1:] > 0.5 * NEG
    return float(d[live].min()) if bool(live.any()) else float("inf")


def beam_search(P, cfg, enc, max_length, start, eos, pad, num_beams, length_penalty=1.0, early_stopping=False, num_return_sequences=1):
    """(sequences, sequences_scores, per-step infos) of transformers' beam search over the restated decoder"""
    B, nb = enc.shape[0], num_beams
    fill = pad if pad is not None else (eos if eos is not None else 0)
    st = init_state(B, nb, max_length, start, fill)
    enc_rows = enc.repeat_interleave(nb, 0)
    infos = []
    while st["go"] and st["cur_len"] < max_length:
        ids = st["run_seq"].reshape(B * nb, -1)[:, :st["cur_len"]]
        logits = R.forward(P, cfg, ids, enc_rows)[:, -1]
        st, info = beam_step(st, F.log_softmax(logits.float(), -1), max_length, eos, length_penalty, early_stopping)
        info["gap"] = gap(info, 2 * nb)
        infos.append(info)
    seq, sc = finalize(st, num_return_sequences)
    return seq, sc, infos
