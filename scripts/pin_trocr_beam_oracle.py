"""Pins tests/trocr_beam_restatement.py against the REAL dependency of a beam-search OCR read-back: transformers'
`VisionEncoderDecoderModel.generate(num_beams=...)` (app.ipynb:845 with a checkpoint's own generation settings).  Run from the repo
root where `transformers` (5.x) is installed, on the CPU:

    python scripts/pin_trocr_beam_oracle.py

For each case a tiny VisionEncoderDecoderModel is built around the decoder configs of tests/golden/trocr_transformers.npz with
counter-PRNG weights (diffute_amd.init.init_param, transformers' key names); transformers runs
`generate(encoder_outputs=BaseModelOutput(last_hidden_state=enc), num_beams=..., length_penalty=..., early_stopping=...,
num_return_sequences=..., return_dict_in_generate=True, output_scores=True)` and the restatement must return the same
`sequences` exactly and `sequences_scores` to 1e-6.  A bf16 decoder must reproduce the path, so at every step the top K + 1
accumulated scores of every item have to lie well apart.  Random encoder states never do (the best of 1500 seeds per case had
gaps of 0.008 ... 0.044 against a bf16 log-prob error near 0.03), so the encoder states are SEARCHED: starting from a seeded
normal draw (a short seed scan picks the start), Adam moves them through the differentiable restatement until every such gap
exceeds TARGET, the values kept within +-4.  Where a case has an eos id it is a token some beam emits at a middle step of the
searched path and no beam emits before, after which the search continues with that id.  The searched fixtures are fit but plain:
many returned hypotheses repeat one token, and none fills every finished slot under early_stopping=True before max_length (that
path is covered by the selection-op test and the early-stop test on the GPU).  Writes
tests/golden/trocr_beam_transformers.npz: settings, encoder states, ids, scores, per-step gaps - no weights.
"""
import ast
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from diffute_amd.init import init_param  # noqa: E402
import trocr_beam_restatement as BR  # noqa: E402

SRC = os.path.join(ROOT, "tests", "golden", "trocr_transformers.npz")
OUT = os.path.join(ROOT, "tests", "golden", "trocr_beam_transformers.npz")
S, MAX_LEN, SEEDS = 45, 6, 12
TARGET, ITERS, LR, CLAMP = 0.25, 400, 0.03, 4.0
CASES = {
    "nb4_lp2_early_eos": dict(model="tied_gelu", num_beams=4, length_penalty=2.0, early_stopping=True, num_return_sequences=2, eos=True),
    "nb3_lp1_noeos": dict(model="untied_relu_scaled", num_beams=3, length_penalty=1.0, early_stopping=False, num_return_sequences=1, eos=False),
    "nb2_lp0_never_eos": dict(model="tied_gelu", num_beams=2, length_penalty=0.0, early_stopping="never", num_return_sequences=2, eos=True),
    "nb4_lp1_never_eos": dict(model="untied_relu_scaled", num_beams=4, length_penalty=1.0, early_stopping="never", num_return_sequences=1, eos=True),
}


def hf_model(cfg, meta):
    from transformers import TrOCRConfig, VisionEncoderDecoderConfig, VisionEncoderDecoderModel, ViTConfig
    dc = TrOCRConfig(**cfg, decoder_start_token_id=meta["start"], pad_token_id=meta["pad"], eos_token_id=2, bos_token_id=0,
                     dropout=0.0, attention_dropout=0.0, activation_dropout=0.0)
    ec = ViTConfig(image_size=32, patch_size=16, hidden_size=cfg["d_model"], num_hidden_layers=1, num_attention_heads=4, intermediate_size=64)
    m = VisionEncoderDecoderModel(VisionEncoderDecoderConfig.from_encoder_decoder_configs(ec, dc)).eval()
    P = {}
    for k, v in m.decoder.state_dict().items():
        if k == "output_projection.weight" and cfg["tie_word_embeddings"]:
            continue
        P[k] = init_param(k, tuple(v.shape), seed=meta["seed"])
    missing, unexpected = m.decoder.load_state_dict(P, strict=False)
    assert not unexpected and set(missing) <= {"output_projection.weight"}, (missing, unexpected)
    return m, P


def search(P, cfg, meta, enc, c, eos):
    return BR.beam_search(P, cfg, enc, MAX_LEN, meta["start"], eos, meta["pad"], c["num_beams"], c["length_penalty"], c["early_stopping"],
                          c["num_return_sequences"])


def pick_eos(infos, start):
    """a token some running beam takes at a middle step (2 or 3) that no running beam took before"""
    for t in (2, 3):
        if len(infos) <= t + 1:
            break
        early = torch.cat([i["new_token"].reshape(-1) for i in infos[:t]])
        for tok in infos[t]["new_token"][0].tolist():
            if tok != start and not bool((early == tok).any()):
                return tok
    return None


def gap_loss(P, cfg, meta, enc, c, eos):
    """(sum of the shortfalls of every top K + 1 gap below TARGET, smallest gap), differentiable in enc along the current path"""
    import torch.nn.functional as F
    import trocr_restatement as R
    B, nb = enc.shape[0], c["num_beams"]
    K = 2 * nb
    fill = meta["pad"]
    st = BR.init_state(B, nb, MAX_LEN, meta["start"], fill)
    rs = st["run_scores"].clone()
    rows = enc.repeat_interleave(nb, 0)
    gaps = []
    while st["go"] and st["cur_len"] < MAX_LEN:
        ids = st["run_seq"].reshape(B * nb, -1)[:, :st["cur_len"]]
        logp = F.log_softmax(R.forward(P, cfg, ids, rows)[:, -1].float(), -1)
        V = logp.shape[-1]
        acc = (logp.view(B, nb, V) + rs[:, :, None]).reshape(B, nb * V)
        with torch.no_grad():
            st, info = BR.beam_step(st, logp.detach(), MAX_LEN, eos, c["length_penalty"], c["early_stopping"])
            top = BR.topk_ordered(acc.detach(), K + 1)[1]
        v = torch.gather(acc, 1, top)
        d = v[:, :-1] - v[:, 1:]
        gaps.append(d[v[:, 1:].detach() > 0.5 * BR.NEG])
        pen = torch.gather(acc, 1, info["parent"] * V + info["token"]) + info["hits"].to(torch.float32) * BR.NEG
        rs = torch.gather(pen, 1, BR.topk_ordered(pen.detach(), nb)[1])
    g = torch.cat(gaps)
    return torch.relu(1.5 * TARGET - g).sum(), float(g.detach().min())


def widen(P, cfg, meta, enc, c, eos):
    """Adam on the encoder states until every gap exceeds TARGET"""
    enc = enc.clone().requires_grad_(True)
    opt = torch.optim.Adam([enc], lr=LR)
    best = (-1.0, enc.detach().clone())
    for it in range(ITERS):
        opt.zero_grad()
        loss, mg = gap_loss(P, cfg, meta, enc, c, eos)
        if mg > best[0]:
            best = (mg, enc.detach().clone())
        if mg > TARGET:
            break
        loss.backward()
        opt.step()
        with torch.no_grad():
            enc.clamp_(-CLAMP, CLAMP)
    return best[1], best[0]


def main():
    from transformers.modeling_outputs import BaseModelOutput
    z = np.load(SRC)
    meta = ast.literal_eval(str(z["meta"]))
    res = {}
    for ci, (name, c) in enumerate(CASES.items()):
        cfg = ast.literal_eval(str(z[c["model"] + "/config"]))
        m, P = hf_model(cfg, meta)
        for p_ in P.values():
            p_.requires_grad_(False)
        done = None
        for seed in range(SEEDS):                                 # starts: two items per case
            enc0 = torch.randn(2, S, cfg["d_model"], generator=torch.Generator().manual_seed(5000 + 100 * ci + seed))
            enc, mg = widen(P, cfg, meta, enc0, c, None)
            eos = None
            if c["eos"]:
                eos = pick_eos(search(P, cfg, meta, enc, c, None)[2], meta["start"])
                if eos is None:
                    continue
                enc, mg = widen(P, cfg, meta, enc, c, eos)
            seq, sc, infos = search(P, cfg, meta, enc, c, eos)
            emitted = eos is None or bool((seq[:, 1:-1] == eos).any())
            print(f"  {name}: start seed {5000 + 100 * ci + seed}: eos {eos}, min gap {mg:.4f}, eos in a returned hypothesis: {emitted}", flush=True)
            if mg > TARGET and (emitted or name != "nb2_lp0_never_eos"):
                done = (seed, enc, eos)
                break
        assert done is not None, f"{name}: no start among {SEEDS} reached gaps above {TARGET}"
        seed, enc, eos = done
        seq, sc, infos = search(P, cfg, meta, enc, c, eos)
        with torch.no_grad():
            out = m.generate(encoder_outputs=BaseModelOutput(last_hidden_state=enc), num_beams=c["num_beams"], length_penalty=c["length_penalty"],
                             early_stopping=c["early_stopping"], num_return_sequences=c["num_return_sequences"], max_length=MAX_LEN,
                             eos_token_id=eos, pad_token_id=meta["pad"], decoder_start_token_id=meta["start"], do_sample=False,
                             return_dict_in_generate=True, output_scores=True)
        assert torch.equal(out.sequences, seq), (name, out.sequences, seq)
        assert float((out.sequences_scores - sc).abs().max()) <= 1e-6 * max(1.0, float(sc.abs().max())), (name, out.sequences_scores, sc)
        gaps = np.array([i["gap"] for i in infos], dtype=np.float32)
        print(f"{name}: start seed {5000 + 100 * ci + seed}, eos {eos}, steps {len(infos)}, min gap {gaps.min():.4f}, |enc| max {float(enc.abs().max()):.2f}, "
              f"ids {seq.tolist()}, scores {sc.tolist()}", flush=True)
        pre = name + "/"
        res[pre + "settings"] = np.array(repr(dict(c, eos=eos, max_length=MAX_LEN)))
        res[pre + "enc"] = enc.numpy()
        res[pre + "ids"] = seq.numpy()
        res[pre + "scores"] = sc.numpy()
        res[pre + "gaps"] = gaps
    np.savez_compressed(OUT, **res)
    print("wrote", OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
