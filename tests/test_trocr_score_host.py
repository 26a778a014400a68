"""Teacher-forced OCR scoring, host side: the new C-ABI entries, the argument checks of `score` / `forward` on CPU tensors (every
refusal comes before anything touches a device), and the restatement against transformers' fixture."""
import ast
import os
import re

import numpy as np
import pytest
import torch

import diffute_amd as D
from diffute_amd import _cabi
import trocr_score_restatement as SR

HERE = os.path.dirname(__file__)
GOLDEN = os.path.join(HERE, "golden", "trocr_score_transformers.npz")
TINY_GOLDEN = os.path.join(HERE, "golden", "trocr_transformers.npz")
NEW = {"dmx_trocr_dec_prefill_workspace_bytes", "dmx_trocr_dec_score", "dmx_trocr_dec_prefill_embed", "dmx_trocr_dec_prefill_attn",
       "dmx_trocr_dec_prefill_lm_loss_workspace_bytes", "dmx_trocr_dec_prefill_lm_loss"}
TINY = dict(d_model=256, decoder_layers=1, decoder_attention_heads=4, decoder_ffn_dim=512, vocab_size=300, max_position_embeddings=64)


def test_score_entries_are_declared_exported_and_bound():
    hdr = open(os.path.join(os.path.dirname(HERE), "include", "diffute_hip.h")).read()
    declared = set(re.findall(r"\b(dmx_trocr_dec_(?:prefill_|score)[a-z0-9_]*)\s*\(", hdr))
    assert declared == NEW
    assert NEW <= set(_cabi.exported_symbols())
    assert not any(s.startswith("dmx_trocr_dec_beam_") for s in NEW)
    for elem in ("bf16", "fp16"):
        lib = _cabi.lib(elem)
        assert all(hasattr(lib, s) for s in NEW), elem
    lib = _cabi.lib()
    assert lib.dmx_trocr_dec_prefill_lm_loss_workspace_bytes(64, 50265) > 0
    assert lib.dmx_trocr_dec_prefill_lm_loss_workspace_bytes(0, 50265) == 0 and lib.dmx_trocr_dec_prefill_lm_loss_workspace_bytes(4097, 50265) == 0
    dec = D.TrOCRForCausalLM(**TINY)
    h = dec._h
    assert lib.dmx_trocr_dec_prefill_workspace_bytes(h, 3, 45, 9) > 0
    for B, T in ((0, 9), (65, 9), (3, 0), (3, 65), (64, 65)):
        assert lib.dmx_trocr_dec_prefill_workspace_bytes(h, B, 45, T) == 0, (B, T)
    # the entry refuses bad arguments with the project's error code, nothing launched (null pointers never reach a kernel)
    assert lib.dmx_trocr_dec_score(h, None, 3, 45, None, None, 9, 2, 1, -100, None, None, None, 0, None, 0, None) == -1
    assert lib.dmx_trocr_dec_prefill_attn(None, 8, None, 8, None, 8, None, 8, 1, 1, 4, 0.125, None) == -1
    assert lib.dmx_trocr_dec_prefill_lm_loss(None, 1, 128, None, 10, None, -100, None, None, None, 0, None, 0, None) == -1


@pytest.fixture(scope="module")
def dec():
    return D.TrOCRForCausalLM(**TINY)


def _enc(B, S=5):
    return torch.zeros(B, S, 256)


def _lab(B, T):
    return torch.zeros(B, T, dtype=torch.int64)


@pytest.mark.parametrize("B,T", [(0, 4), (65, 4), (2, 0), (2, 65)])
def test_decoder_score_refuses_bad_batch_and_length(dec, B, T):
    with pytest.raises(ValueError):
        dec.score(_lab(B, T), _enc(B))


def test_decoder_score_refuses_too_many_rows():
    big = D.TrOCRForCausalLM(**dict(TINY, max_position_embeddings=512))
    with pytest.raises(ValueError, match="4096"):
        big.score(_lab(64, 65), _enc(64))
    with pytest.raises(RuntimeError, match="GPU"):                 # 64 * 64 rows pass the checks; CPU tensors stop at the device gate
        big.score(_lab(64, 64), _enc(64))


def test_decoder_score_refuses_bad_labels(dec):
    for bad in (torch.zeros(2, 4, dtype=torch.int32), torch.zeros(2, 4), torch.zeros(8, dtype=torch.int64), torch.zeros(3, 4, dtype=torch.int64),
                torch.zeros(2, 4, 1, dtype=torch.int64), [[0, 1, 2, 3]] * 2):
        with pytest.raises(ValueError):
            dec.score(bad, _enc(2))
    for v in (300, -1, -99, 10 ** 6):
        lab = _lab(2, 4); lab[1, 2] = v
        with pytest.raises(ValueError, match="ignore_index"):
            dec.score(lab, _enc(2))
    lab = _lab(2, 4); lab[1, 2] = -100
    with pytest.raises(ValueError, match="ignore_index"):          # -100 is out of range once another ignore_index is chosen
        dec.score(lab, _enc(2), ignore_index=-1)
    with pytest.raises(RuntimeError, match="GPU"):                 # valid arguments: the first thing that fails is the device gate
        dec.score(lab, _enc(2))
    with pytest.raises(ValueError):
        dec.score(None, _enc(2))
    with pytest.raises(ValueError):
        dec.score(_lab(2, 4), _enc(2), decoder_input_ids=_lab(2, 5))
    with pytest.raises(ValueError):
        dec.score(None, _enc(2), decoder_input_ids=torch.full((2, 4), 300, dtype=torch.int64))
    with pytest.raises(ValueError):
        dec.score(_lab(2, 4), torch.zeros(2, 5, 128))


def test_model_score_and_forward_call_checks(dec):
    model = D.VisionEncoderDecoderModel(D.TrOCREncoder(image_size=32, patch_size=16, hidden_size=256, num_hidden_layers=1, num_attention_heads=4,
                                                       intermediate_size=64), dec)
    px, enc, lab = torch.zeros(2, 3, 32, 32), _enc(2), _lab(2, 4)
    with pytest.raises(ValueError, match="exactly one"):
        model.score(px, encoder_hidden_states=enc, labels=lab)
    with pytest.raises(ValueError, match="exactly one"):
        model.score(labels=lab)
    with pytest.raises(ValueError, match="labels or decoder_input_ids"):
        model.score(px)
    with pytest.raises(ValueError, match="exactly one"):
        model(labels=lab)
    with pytest.raises(ValueError, match="exactly one"):
        model(pixel_values=px, labels=lab, encoder_outputs=(enc,))
    with pytest.raises(ValueError, match="labels or decoder_input_ids"):
        model(pixel_values=px)
    with pytest.raises(ValueError, match="labels or decoder_input_ids"):
        model(encoder_outputs=(enc,))
    with pytest.raises(ValueError):                                # checked on the pixel batch, before the encoder runs
        model.score(px, labels=_lab(3, 4))
    with pytest.raises(ValueError):
        model(pixel_values=px, labels=_lab(2, 65))
    with pytest.raises(ValueError):
        model.score(torch.zeros(65, 3, 32, 32), labels=_lab(65, 4))
    bad = lab.clone(); bad[0, 0] = 300
    with pytest.raises(ValueError, match="ignore_index"):
        model(encoder_outputs=(enc,), labels=bad)
    with pytest.raises(RuntimeError, match="GPU"):
        model.score(encoder_hidden_states=enc, labels=lab)
    with pytest.raises(RuntimeError, match="GPU"):
        model(encoder_outputs=(enc,), decoder_input_ids=lab)


@pytest.mark.parametrize("name", ["tied_gelu", "untied_relu_scaled"])
@pytest.mark.parametrize("T", [9, 1])
def test_restatement_reproduces_the_transformers_fixture(name, T):
    z, zg = np.load(GOLDEN), np.load(TINY_GOLDEN)
    cfg = ast.literal_eval(str(zg[name + "/config"]))
    meta = ast.literal_eval(str(zg["meta"]))
    m = D.TrOCRForCausalLM(seed=meta["seed"], **cfg)
    P = {k: v.detach().float() for k, v in m.named_parameters()}
    pre = f"{name}/T{T}/"
    labels = torch.from_numpy(z[pre + "labels"])
    ids, logits, lp, loss = SR.score(P, cfg, labels, torch.from_numpy(z[pre + "enc"]), meta["start"], meta["pad"])
    assert torch.equal(ids, torch.from_numpy(z[pre + "decoder_input_ids"]))
    assert abs(float(loss) - float(z[pre + "loss"])) <= 1e-6
    assert abs(float(-lp.sum() / (labels != SR.IGNORE).sum()) - float(loss)) <= 1e-5, "loss = -sum(token log-probs) / number of tokens"
    assert float((logits - torch.from_numpy(z[pre + "logits"])).abs().max()) <= 1e-5
    assert float((lp - torch.from_numpy(z[pre + "token_logprobs"])).abs().max()) <= 1e-5
    assert bool((lp[labels == SR.IGNORE] == 0).all())


def test_fixture_covers_the_cases_and_is_small():
    z = np.load(GOLDEN)
    assert os.path.getsize(GOLDEN) < 1 << 20
    assert not any("weight" in k for k in z.files)
    for name in ("tied_gelu", "untied_relu_scaled"):
        lab = z[f"{name}/T9/labels"]
        n = (lab != -100).sum(1)
        assert lab.shape == (3, 9) and len(set(n.tolist())) == 3, "ragged lengths"
        assert any((row[:-1] == -100).any() and (row[np.argmax(row == -100) + 1:] != -100).any() for row in lab), "a -100 in the middle of a row"
        assert z[f"{name}/T1/labels"].shape == (3, 1) and (z[f"{name}/T1/labels"] == -100).sum() == 1
