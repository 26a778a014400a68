"""Beam-search OCR read-back on the full-size decoder: ms per `beam_search` call and per step at 32 new tokens for
(B, num_beams) in {(1, 4), (4, 4), (16, 4)}, next to `greedy` at the same row count M = B * num_beams (the same weights are
streamed per step), so the line reports the beam step's excess over the greedy step and the launches behind it.  Step times are
the difference between a call of 33 tokens and a call of 2 tokens over the 31 steps between them, so the cross-K/V GEMM (B x S
rows for beams, M x S rows for greedy), the reset, the gather and the final synchronisation drop out; the whole-call times and
the set-up cost (the 2-token call less one step) are reported beside them.

    python scripts/bench_ocr_beam.py [--reps 5] > profiles/ocr_beam_line.json

Prints one JSON line."""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import diffute_amd as D  # noqa: E402

NEW_TOKENS, S = 32, 577


def timed(fn, reps):
    fn(); fn()
    torch.cuda.synchronize()
    best = float("inf")
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        best = min(best, time.perf_counter() - t0)
    return best * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_ocr_beam: no GPU visible")
    dev = torch.device("cuda:0")
    m = D.TrOCRForCausalLM(device=dev)
    L = NEW_TOKENS + 1
    out = dict(bench="ocr_beam", new_tokens=NEW_TOKENS, S=S, launches_per_greedy_step=m.launches_per_step,
               launches_per_beam_step=m.beam_launches_per_step, cases=[])
    for B, nb in ((1, 4), (4, 4), (16, 4)):
        M = B * nb
        enc = torch.randn(M, S, 1024, generator=torch.Generator().manual_seed(B)).to(dev)
        beam = timed(lambda: m.beam_search(enc[:B], L, 2, None, 1, num_beams=nb), a.reps)          # no eos: all 32 steps run
        beam2 = timed(lambda: m.beam_search(enc[:B], 2, 2, None, 1, num_beams=nb), a.reps)         # set-up + one step
        greedy = timed(lambda: m.greedy(enc, L, 2, None, 1), a.reps)
        greedy2 = timed(lambda: m.greedy(enc, 2, 2, None, 1), a.reps)
        bstep, gstep = (beam - beam2) / (NEW_TOKENS - 1), (greedy - greedy2) / (NEW_TOKENS - 1)
        out["cases"].append(dict(B=B, num_beams=nb, rows=M, beam_ms=round(beam, 3), greedy_same_rows_ms=round(greedy, 3),
                                 beam_ms_per_step=round(bstep, 4), greedy_ms_per_step=round(gstep, 4), excess_ms_per_step=round(bstep - gstep, 4),
                                 beam_setup_ms=round(beam2 - bstep, 3), greedy_setup_ms=round(greedy2 - gstep, 3)))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
