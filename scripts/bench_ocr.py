"""OCR read-back benchmark (app.ipynb:845 `full_trocr_model_te.generate(pixel_values)`): the full-size TrOCR decoder (seeded
weights) generating 32 new tokens for B = 1, 8, 32 crops from encoder states [B, 577, 1024].  Prints one JSON line.

    python scripts/bench_ocr.py [--batches 1,8,32] [--new-tokens 32] [--iters 5]

Per batch size: ms per `generate` (cross K/V + 32 greedy steps, host poll included), us per step (32 replays of the captured step
graph, device events), launches per step, the bytes a step must read (weights + cross K/V of every image, from the shapes) over
the step time, as TB/s and as a share of the 8.0 TB/s peak and of the 6.3 TB/s measured copy rate; and a torch-eager baseline of the
same arithmetic (bf16 F.linear + scaled_dot_product_attention over a KV cache, argmax on fp32 logits) - transformers' own generate
when it is importable on the machine is not used: it would run fp32 weights, not the same arithmetic.
"""
import argparse
import json
import os
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import diffute_amd as D  # noqa: E402

PEAK, COPY = 8.0e12, 6.3e12


def step_bytes(cfg, B, S):
    d, f, L, V = cfg["d_model"], cfg["decoder_ffn_dim"], cfg["decoder_layers"], cfg["vocab_size"]
    weights = 2 * (L * (6 * d * d + 2 * d * f) + V * d)
    cross = 2 * B * S * L * 2 * d
    return weights, cross


class Eager:
    """torch-eager decode of the same model: bf16 weights, fp32 logits for the pick"""

    def __init__(self, m):
        P = {k: v.detach() for k, v in m.named_parameters()}
        self.c = m.config
        bf = lambda k: P[k].to(torch.bfloat16)  # noqa: E731
        self.emb, self.pos = bf("model.decoder.embed_tokens.weight"), P["model.decoder.embed_positions.weight"]
        self.le = (P["model.decoder.layernorm_embedding.weight"], P["model.decoder.layernorm_embedding.bias"])
        self.L = []
        for i in range(self.c.decoder_layers):
            p = f"model.decoder.layers.{i}."
            g = lambda n: (bf(p + n + ".weight"), P[p + n + ".bias"].to(torch.bfloat16))  # noqa: E731
            ln = lambda n: (P[p + n + ".weight"].to(torch.bfloat16), P[p + n + ".bias"].to(torch.bfloat16))  # noqa: E731
            qkv = (torch.cat([bf(p + f"self_attn.{x}_proj.weight") for x in "qkv"]), torch.cat([P[p + f"self_attn.{x}_proj.bias"] for x in "qkv"]).to(torch.bfloat16))
            ckv = (torch.cat([bf(p + f"encoder_attn.{x}_proj.weight") for x in "kv"]), torch.cat([P[p + f"encoder_attn.{x}_proj.bias"] for x in "kv"]).to(torch.bfloat16))
            self.L.append(dict(qkv=qkv, o=g("self_attn.out_proj"), ln1=ln("self_attn_layer_norm"), cq=g("encoder_attn.q_proj"), ckv=ckv,
                               co=g("encoder_attn.out_proj"), ln2=ln("encoder_attn_layer_norm"), fc1=g("fc1"), fc2=g("fc2"), ln3=ln("final_layer_norm")))

    @torch.no_grad()
    def generate(self, enc, max_length):
        c = self.c
        B, S, d = enc.shape[0], enc.shape[1], c.d_model
        H = c.decoder_attention_heads
        e = enc.to(torch.bfloat16)
        cross = [F.linear(e, W["ckv"][0], W["ckv"][1]).view(B, S, 2, H, 64).permute(2, 0, 3, 1, 4) for W in self.L]
        kc = torch.zeros(len(self.L), 2, B, H, max_length, 64, dtype=torch.bfloat16, device=enc.device)
        ids = torch.full((B, 1), c.decoder_start_token_id, dtype=torch.int64, device=enc.device)
        for pos in range(max_length - 1):
            x = self.emb[ids[:, -1]].float() + self.pos[pos + 2]
            x = F.layer_norm(x, (d,), *self.le, 1e-5).to(torch.bfloat16)[:, None]
            for li, W in enumerate(self.L):
                qkv = F.linear(x, *W["qkv"]).view(B, 1, 3, H, 64).permute(2, 0, 3, 1, 4)
                kc[li, :, :, :, pos] = qkv[1:, :, :, 0]
                a = F.scaled_dot_product_attention(qkv[0], kc[li, 0, :, :, :pos + 1], kc[li, 1, :, :, :pos + 1])
                x = F.layer_norm(x + F.linear(a.transpose(1, 2).reshape(B, 1, d), *W["o"]), (d,), *W["ln1"], 1e-5)
                q = F.linear(x, *W["cq"]).view(B, 1, H, 64).transpose(1, 2)
                a = F.scaled_dot_product_attention(q, cross[li][0], cross[li][1])
                x = F.layer_norm(x + F.linear(a.transpose(1, 2).reshape(B, 1, d), *W["co"]), (d,), *W["ln2"], 1e-5)
                h = F.gelu(F.linear(x, *W["fc1"]))
                x = F.layer_norm(x + F.linear(h, *W["fc2"]), (d,), *W["ln3"], 1e-5)
            nxt = torch.argmax(F.linear(x[:, 0], self.emb).float(), -1)
            ids = torch.cat([ids, nxt[:, None]], 1)
        return ids


def timed(fn, iters, samples=None):
    """best of `iters` timed runs after one warm-up (ms); every sample is appended to `samples`"""
    fn()
    torch.cuda.synchronize()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    best = float("inf")
    for _ in range(iters):
        s.record(); fn(); e.record(); e.synchronize()
        best = min(best, s.elapsed_time(e))
        if samples is not None:
            samples.append(round(s.elapsed_time(e), 3))
    return best


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="1,8,32")
    ap.add_argument("--new-tokens", type=int, default=32)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--no-eager", action="store_true")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    m = D.TrOCRForCausalLM(device=dev)
    cfg = m.config.to_dict()
    model = D.VisionEncoderDecoderModel(D.TrOCREncoder(hidden_size=1024, num_hidden_layers=1, intermediate_size=128, device=dev), m,
                                        dict(eos_token_id=None))
    eager = None if a.no_eager else Eager(m)
    T = a.new_tokens + 1
    S = 577
    out = dict(metric="trocr_decoder_generate", new_tokens=a.new_tokens, launches_per_step=m.launches_per_step,
               launches_per_layer=(m.launches_per_step - 2) / cfg["decoder_layers"], rows=[])
    for B in [int(b) for b in a.batches.split(",")]:
        enc = torch.randn(B, S, 1024, generator=torch.Generator().manual_seed(B)).to(dev)
        gen_samples, eager_samples = [], []
        ms_gen = timed(lambda: model.generate(encoder_hidden_states=enc, max_new_tokens=a.new_tokens), a.iters, gen_samples)
        r = m._runs[(B, S, T)]
        g = next(iter(r["graphs"].values()))

        def steps():
            m._begin(r, enc.float().contiguous(), T, 2)
            for _ in range(a.new_tokens):
                g.replay()
        ms_steps = timed(steps, a.iters)
        ms_kv = timed(lambda: m._begin(r, enc.float().contiguous(), T, 2), a.iters)
        us_step = (ms_steps - ms_kv) * 1e3 / a.new_tokens
        wb, cb = step_bytes(cfg, B, S)
        bw = (wb + cb) / (us_step * 1e-6)
        row = dict(B=B, ms_per_generate=round(ms_gen, 3), us_per_step=round(us_step, 2), ms_cross_kv=round(ms_kv, 3),
                   bytes_per_step=wb + cb, weight_bytes=wb, cross_kv_bytes=cb, tb_per_s=round(bw / 1e12, 3),
                   share_of_peak=round(bw / PEAK, 3), share_of_copy_rate=round(bw / COPY, 3))
        if eager is not None:
            ms_eager = timed(lambda: eager.generate(enc, T), a.iters, eager_samples)
            hip_ids = model.generate(encoder_hidden_states=enc, max_new_tokens=a.new_tokens)
            row.update(eager_ms_per_generate=round(ms_eager, 3), speedup_vs_eager=round(ms_eager / ms_gen, 2),
                       generate_samples_ms=gen_samples, eager_samples_ms=eager_samples,
                       eager_ids_equal=bool(torch.equal(eager.generate(enc, T), hip_ids)))
        out["rows"].append(row)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
