"""Pins tests/trocr_score_restatement.py against the REAL dependency of a teacher-forced OCR score: transformers'
`VisionEncoderDecoderModel(encoder_outputs=..., labels=...)` (`.loss`, `.logits`) over the model of app.ipynb:548.  Run from the repo
root where `transformers` (5.x) is installed, on the CPU:

    python scripts/pin_trocr_score_oracle.py

For both decoder configs of tests/golden/trocr_transformers.npz a tiny VisionEncoderDecoderModel is built with counter-PRNG weights
(diffute_amd.init.init_param, the seed of that file's `meta`, transformers' key names); transformers scores labels of ragged
lengths padded with -100, one row with a -100 in the middle, at T = 9 and T = 1; the restatement must give the same `loss` to 1e-6
and the same `logits` to 1e-5.  Writes tests/golden/trocr_score_transformers.npz: encoder states, labels, the decoder input ids as
transformers shifted them, loss, per-token log-probs, logits - no weights.
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
import trocr_score_restatement as SR  # noqa: E402

SRC = os.path.join(ROOT, "tests", "golden", "trocr_transformers.npz")
OUT = os.path.join(ROOT, "tests", "golden", "trocr_score_transformers.npz")
S = 45


def hf_model(cfg, meta):
    from transformers import TrOCRConfig, VisionEncoderDecoderConfig, VisionEncoderDecoderModel, ViTConfig
    dc = TrOCRConfig(**cfg, decoder_start_token_id=meta["start"], pad_token_id=meta["pad"], eos_token_id=2, bos_token_id=0,
                     dropout=0.0, attention_dropout=0.0, activation_dropout=0.0)
    ec = ViTConfig(image_size=32, patch_size=16, hidden_size=cfg["d_model"], num_hidden_layers=1, num_attention_heads=4, intermediate_size=64)
    vc = VisionEncoderDecoderConfig.from_encoder_decoder_configs(ec, dc)
    vc.decoder_start_token_id, vc.pad_token_id = meta["start"], meta["pad"]
    m = VisionEncoderDecoderModel(vc).eval()
    P = {}
    for k, v in m.decoder.state_dict().items():
        if k == "output_projection.weight" and cfg["tie_word_embeddings"]:
            continue
        P[k] = init_param(k, tuple(v.shape), seed=meta["seed"])
    missing, unexpected = m.decoder.load_state_dict(P, strict=False)
    assert not unexpected and set(missing) <= {"output_projection.weight"}, (missing, unexpected)
    return m, P


def make_labels(V, T, g):
    """three rows: full length, ragged (padded with -100), and one with a -100 in the middle; T = 1: one kept, one ignored, one kept"""
    lab = torch.randint(0, V, (3, T), generator=g)
    lab[0, 0], lab[0, -1] = 0, V - 1                              # the ends of the vocabulary
    if T == 1:
        lab[1, 0] = SR.IGNORE
        return lab
    lab[1, T - 4:] = SR.IGNORE
    lab[2, T // 2] = SR.IGNORE
    lab[2, T - 1:] = SR.IGNORE
    return lab


def main():
    from transformers.modeling_outputs import BaseModelOutput
    z = np.load(SRC)
    meta = ast.literal_eval(str(z["meta"]))
    res = {}
    for mi, name in enumerate(("tied_gelu", "untied_relu_scaled")):
        cfg = ast.literal_eval(str(z[name + "/config"]))
        m, P = hf_model(cfg, meta)
        for T in (9, 1):
            g = torch.Generator().manual_seed(7000 + 10 * mi + T)
            enc = torch.randn(3, S, cfg["d_model"], generator=g)
            labels = make_labels(cfg["vocab_size"], T, g)
            with torch.no_grad():
                out = m(encoder_outputs=BaseModelOutput(last_hidden_state=enc), labels=labels)
            from transformers.models.vision_encoder_decoder.modeling_vision_encoder_decoder import shift_tokens_right
            tf_ids = shift_tokens_right(labels, meta["pad"], meta["start"])
            ids, logits, lp, loss = SR.score(P, cfg, labels, enc, meta["start"], meta["pad"])
            assert torch.equal(ids, tf_ids), (name, T, ids, tf_ids)
            assert abs(float(loss) - float(out.loss)) <= 1e-6, (name, T, float(loss), float(out.loss))
            err = float((logits - out.logits).abs().max())
            assert err <= 1e-5, (name, T, err)
            tf_lp = torch.log_softmax(out.logits.double(), -1).gather(-1, labels.clamp(min=0)[..., None])[..., 0]
            tf_lp = torch.where(labels != SR.IGNORE, tf_lp, torch.zeros_like(tf_lp)).float()
            print(f"{name} T={T}: loss {float(out.loss):.6f} (restatement {float(loss):.6f}), logits max |diff| {err:.2e}, labels {labels.tolist()}", flush=True)
            pre = f"{name}/T{T}/"
            res[pre + "enc"] = enc.numpy()
            res[pre + "labels"] = labels.numpy()
            res[pre + "decoder_input_ids"] = tf_ids.numpy()
            res[pre + "loss"] = np.float32(float(out.loss))
            res[pre + "token_logprobs"] = tf_lp.numpy()
            res[pre + "logits"] = out.logits.numpy()
    np.savez_compressed(OUT, **res)
    print("wrote", OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
