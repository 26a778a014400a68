"""Test-local restatement of transformers' TrOCRForCausalLM (the text decoder of app.ipynb:548) and of its greedy
`generate(num_beams=1, do_sample=False)` (app.ipynb:845): fp32 torch on the CPU, written out from the module structure
(BART-style post-LN layers, learned positions read at row p + 2, q scaled after its bias, LayerNorm eps 1e-5), with a
teacher-forced forward over the whole sequence (causal mask) and a KV-cache greedy loop.  `P` maps transformers' state-dict
keys to fp32 tensors; `cfg` is a dict of TrOCRConfig fields."""
import math

import torch
import torch.nn.functional as F

EPS = 1e-5


def _ln(x, P, k):
    return F.layer_norm(x, (x.shape[-1],), P[k + ".weight"], P[k + ".bias"], EPS)


def _lin(x, P, k, bias=True):
    return F.linear(x, P[k + ".weight"], P[k + ".bias"] if bias else None)


def _act(cfg, x):
    return F.gelu(x) if cfg["activation_function"] == "gelu" else F.relu(x)


def _heads(x, H):
    B, T, D = x.shape
    return x.view(B, T, H, D // H).transpose(1, 2)


def _attend(q, k, v, mask=None):
    s = q @ k.transpose(-1, -2)
    if mask is not None:
        s = s.masked_fill(mask, float("-inf"))
    o = torch.softmax(s, -1) @ v
    B, H, T, d = o.shape
    return o.transpose(1, 2).reshape(B, T, H * d)


def lm_weight(P, cfg):
    return P["model.decoder.embed_tokens.weight"] if cfg.get("tie_word_embeddings", True) else P["output_projection.weight"]


def embed(P, cfg, ids, pos0):
    D = cfg["d_model"]
    scale = math.sqrt(D) if cfg.get("scale_embedding") else 1.0
    pos = torch.arange(pos0, pos0 + ids.shape[1]) + 2
    x = P["model.decoder.embed_tokens.weight"][ids] * scale + P["model.decoder.embed_positions.weight"][pos][None]
    if cfg.get("layernorm_embedding", True):
        x = _ln(x, P, "model.decoder.layernorm_embedding")
    return x


def cross_kv(P, cfg, enc):
    H = cfg["decoder_attention_heads"]
    out = []
    for i in range(cfg["decoder_layers"]):
        p = f"model.decoder.layers.{i}.encoder_attn."
        out.append((_heads(_lin(enc, P, p + "k_proj"), H), _heads(_lin(enc, P, p + "v_proj"), H)))
    return out


def _layers(P, cfg, x, ckv, self_kv=None, mask=None):
    """the decoder layers over x [B, T, D]; self_kv (list of [K, V] per layer) is extended in place when given"""
    H = cfg["decoder_attention_heads"]
    scale = (cfg["d_model"] // H) ** -0.5
    for i in range(cfg["decoder_layers"]):
        p = f"model.decoder.layers.{i}."
        q = _heads(_lin(x, P, p + "self_attn.q_proj") * scale, H)
        k = _heads(_lin(x, P, p + "self_attn.k_proj"), H)
        v = _heads(_lin(x, P, p + "self_attn.v_proj"), H)
        if self_kv is not None:
            if self_kv[i] is not None:
                k = torch.cat([self_kv[i][0], k], 2); v = torch.cat([self_kv[i][1], v], 2)
            self_kv[i] = (k, v)
        x = _ln(x + _lin(_attend(q, k, v, mask), P, p + "self_attn.out_proj"), P, p + "self_attn_layer_norm")
        q = _heads(_lin(x, P, p + "encoder_attn.q_proj") * scale, H)
        x = _ln(x + _lin(_attend(q, ckv[i][0], ckv[i][1]), P, p + "encoder_attn.out_proj"), P, p + "encoder_attn_layer_norm")
        x = _ln(x + _lin(_act(cfg, _lin(x, P, p + "fc1")), P, p + "fc2"), P, p + "final_layer_norm")
    return x


def forward(P, cfg, input_ids, enc):
    """teacher-forced logits [B, T, V] of input_ids [B, T] over encoder states [B, S, D_enc]"""
    T = input_ids.shape[1]
    x = embed(P, cfg, input_ids, 0)
    mask = torch.triu(torch.ones(T, T, dtype=torch.bool), 1)
    return F.linear(_layers(P, cfg, x, cross_kv(P, cfg, enc), mask=mask), lm_weight(P, cfg))


def generate(P, cfg, enc, max_length, start, eos, pad):
    """greedy ids [B, L] (L <= max_length, counting the start token) and the fp32 logits [B, L - 1, V] of every step, as
    transformers' greedy search: argmax (lowest index on ties), finished rows emit pad, stop when all rows finished"""
    B = enc.shape[0]
    ckv = cross_kv(P, cfg, enc)
    kv = [None] * cfg["decoder_layers"]
    ids = torch.full((B, 1), int(start), dtype=torch.int64)
    unfinished = torch.ones(B, dtype=torch.bool)
    steps = []
    while ids.shape[1] < max_length:
        pos = ids.shape[1] - 1
        x = _layers(P, cfg, embed(P, cfg, ids[:, -1:], pos), ckv, self_kv=kv)
        logits = F.linear(x[:, -1], lm_weight(P, cfg))
        steps.append(logits)
        nxt = torch.argmax(logits, -1)
        if eos is not None:
            nxt = torch.where(unfinished, nxt, torch.full_like(nxt, int(pad)))
        ids = torch.cat([ids, nxt[:, None]], 1)
        if eos is not None:
            unfinished &= nxt != int(eos)
            if not unfinished.any():
                break
    return ids, torch.stack(steps, 1)


def margins(step_logits):
    """top-1 minus top-2 logit of every (row, step) [B, L - 1]"""
    t2 = torch.topk(step_logits, 2, -1).values
    return t2[..., 0] - t2[..., 1]
