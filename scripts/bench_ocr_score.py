"""Teacher-forced OCR scoring benchmark: the full-size TrOCR decoder (seeded weights) scoring T = 32 known target ids for
B = 1, 8, 32 crops from encoder states [B, 577, 1024].  Prints one JSON line.

    python scripts/bench_ocr_score.py [--batches 1,8,32] [--tokens 32] [--iters 7]

Per batch size: ms per `TrOCRForCausalLM.score(labels, enc)` (cross K/V + one prefill + the fused LM loss) against the other route to
the same answer, `TrOCRForCausalLM.forward(decoder_input_ids, enc)` (the decode step run T times, [B, T, V] fp32 logits) followed by
torch `log_softmax` + `gather`.  Method of scripts/bench_ocr.py: one warm-up call, then `iters` calls timed with device events on
the current stream; median, minimum and maximum of the samples are reported, the ratio is taken between the medians.  The two routes
must agree: the largest difference of their per-token log-probs is printed with the timings.
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import diffute_amd as D  # noqa: E402


def timed(fn, iters):
    fn()
    torch.cuda.synchronize()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    samples = []
    for _ in range(iters):
        s.record(); fn(); e.record(); e.synchronize()
        samples.append(s.elapsed_time(e))
    return dict(median=round(statistics.median(samples), 3), min=round(min(samples), 3), max=round(max(samples), 3))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="1,8,32")
    ap.add_argument("--tokens", type=int, default=32)
    ap.add_argument("--iters", type=int, default=7)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    m = D.TrOCRForCausalLM(device=dev)
    c = m.config
    T, S, V = a.tokens, 577, c.vocab_size
    out = dict(metric="trocr_decoder_score", tokens=T, S=S, iters=a.iters, rows=[])
    for B in [int(b) for b in a.batches.split(",")]:
        g = torch.Generator().manual_seed(B)
        enc = torch.randn(B, S, c.d_model, generator=g).to(dev)
        labels = torch.randint(0, V, (B, T), generator=g).to(dev)
        ids = torch.cat([torch.full((B, 1), c.decoder_start_token_id, dtype=torch.int64, device=dev), labels[:, :-1]], 1)

        def steps():
            lg = m(ids, enc).logits
            return torch.log_softmax(lg, -1).gather(-1, labels[..., None])[..., 0]

        ms_score = timed(lambda: m.score(labels, enc), a.iters)
        ms_steps = timed(steps, a.iters)
        diff = float((m.score(labels, enc).token_logprobs - steps()).abs().max())
        out["rows"].append(dict(B=B, rows=B * T, score_ms=ms_score, step_path_ms=ms_steps, speedup=round(ms_steps["median"] / ms_score["median"], 2),
                                max_logprob_diff_between_routes=round(diff, 4)))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
