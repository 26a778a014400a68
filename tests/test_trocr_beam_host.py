"""Beam-search OCR read-back, host side: the restatement against transformers' fixture, beam_step on constructed log-probs, the
argument checks of both beam_search methods on CPU tensors, and the C-ABI entries."""
import ast
import math
import os
import re

import numpy as np
import pytest
import torch

import diffute_amd as D
from diffute_amd import _cabi
import trocr_beam_restatement as BR

HERE = os.path.dirname(__file__)
GOLDEN = os.path.join(HERE, "golden", "trocr_beam_transformers.npz")
GREEDY_GOLDEN = os.path.join(HERE, "golden", "trocr_transformers.npz")
NAMES = ["nb4_lp2_early_eos", "nb3_lp1_noeos", "nb2_lp0_never_eos", "nb4_lp1_never_eos"]
NEG = -1.0e9


@pytest.mark.parametrize("name", NAMES)
def test_restatement_reproduces_the_transformers_fixture(name):
    z, zg = np.load(GOLDEN), np.load(GREEDY_GOLDEN)
    s = ast.literal_eval(str(z[name + "/settings"]))
    cfg = ast.literal_eval(str(zg[s["model"] + "/config"]))
    meta = ast.literal_eval(str(zg["meta"]))
    m = D.TrOCRForCausalLM(seed=meta["seed"], **cfg)
    P = {k: v.detach().float() for k, v in m.named_parameters()}
    seq, sc, infos = BR.beam_search(P, cfg, torch.from_numpy(z[name + "/enc"]), s["max_length"], meta["start"], s["eos"], meta["pad"], s["num_beams"],
                                    s["length_penalty"], s["early_stopping"], s["num_return_sequences"])
    assert torch.equal(seq, torch.from_numpy(z[name + "/ids"]))
    assert float((sc - torch.from_numpy(z[name + "/scores"])).abs().max()) <= 1e-6
    assert np.allclose(np.array([i["gap"] for i in infos], dtype=np.float32), z[name + "/gaps"], atol=1e-5)


def test_fixture_covers_the_settings_and_is_small():
    z = np.load(GOLDEN)
    ss = [ast.literal_eval(str(z[n + "/settings"])) for n in NAMES]
    assert {s["early_stopping"] for s in ss} == {False, True, "never"} and {s["length_penalty"] for s in ss} == {0.0, 1.0, 2.0}
    assert {s["num_beams"] for s in ss} == {2, 3, 4} and {s["num_return_sequences"] for s in ss} == {1, 2}
    assert any(s["eos"] is None for s in ss)
    # in at least one case a returned hypothesis ends with the eos id before max_length (the finished-merge path with pad after it)
    assert any(s["eos"] is not None and (z[n + "/ids"][:, 1:-1] == s["eos"]).any() for n, s in zip(NAMES, ss))
    assert os.path.getsize(GOLDEN) < 1 << 20


def _logp(rows, V=12):
    """log-probs [len(rows), V] with the given {token: value} entries and -30 elsewhere (not normalised: beam_step only adds)"""
    x = torch.full((len(rows), V), -30.0)
    for r, d in enumerate(rows):
        for t, v in d.items():
            x[r, t] = v
    return x


def test_first_step_only_beam_zero_is_alive():
    st = BR.init_state(1, 3, 6, 2, 1)
    row = {4: -0.1, 5: -0.2, 6: -0.3, 7: -0.4, 8: -0.5, 9: -0.6}
    st, info = BR.beam_step(st, _logp([row, {0: 0.0}, {1: 0.0}]), 6, None, 1.0, False)
    assert info["parent"].tolist() == [[0] * 6] and info["token"].tolist() == [[4, 5, 6, 7, 8, 9]]     # -1e9 + logp never enters
    assert st["run_seq"][0, :, :2].tolist() == [[2, 4], [2, 5], [2, 6]] and not st["fin_flags"].any() and st["go"]
    assert float(np.float32(-1e9) + np.float32(-0.1)) == -1e9                                           # the dead beams tie en masse


def test_eos_finishes_only_within_the_first_num_beams_ranks():
    st = BR.init_state(1, 2, 8, 2, 1)
    st["run_scores"] = torch.tensor([[-0.5, -0.6]])
    # ranks: (b0, 3) -0.6, (b0, eos) -0.7, (b1, 4) -0.9, (b1, eos) -1.0: the first eos has rank 1 < nb and finishes, the second not
    st2, info = BR.beam_step(st, _logp([{3: -0.1, 9: -0.2}, {4: -0.3, 9: -0.4}]), 8, 9, 1.0, False)
    assert info["token"].tolist() == [[3, 9, 4, 9]] and info["hits"].tolist() == [[False, True, False, True]]
    assert st2["fin_flags"].tolist() == [[True, False]] and st2["fin_len"][0, 0] == 1 and st2["fin_seq"][0, 0, :2].tolist() == [2, 9]
    assert math.isclose(float(st2["fin_scores"][0, 0]), -0.7, rel_tol=1e-6) and float(st2["fin_scores"][0, 1]) == NEG
    assert st2["run_seq"][0, :, 1].tolist() == [3, 4] and torch.allclose(st2["run_scores"], torch.tensor([[-0.6, -0.9]]))


def test_full_finished_set_with_early_stopping_true_takes_nothing_more_and_ends():
    st = BR.init_state(1, 2, 8, 2, 1)
    st.update(run_scores=torch.tensor([[-0.1, -0.2]]), fin_scores=torch.tensor([[-5.0, -6.0]]), fin_flags=torch.tensor([[True, True]]),
              fin_len=torch.tensor([[1, 1]]), cur_len=2)
    lp = _logp([{9: -0.01, 3: -0.5}, {9: -0.02, 4: -0.6}])
    a, _ = BR.beam_step(dict(st), lp, 8, 9, 1.0, True)
    assert a["fin_scores"].tolist() == [[-5.0, -6.0]] and not a["go"]
    b, _ = BR.beam_step(dict(st), lp, 8, 9, 1.0, False)                                       # without it the better ones replace them
    assert b["fin_scores"][0, 0] > -1.0 and b["fin_len"].tolist() == [[2, 2]]


@pytest.mark.parametrize("lp,improvable", [(2.0, True), (0.0, False)])
def test_never_uses_max_length_only_with_a_positive_length_penalty(lp, improvable):
    st = BR.init_state(1, 2, 10, 2, 1)
    st.update(run_scores=torch.tensor([[-4.0, -4.5]]), fin_scores=torch.tensor([[-1.0, -1.5]]), fin_flags=torch.tensor([[True, True]]),
              fin_len=torch.tensor([[1, 1]]), cur_len=2)
    new, _ = BR.beam_step(st, _logp([{3: -0.1, 5: -3.0}, {4: -0.1, 6: -3.0}]), 10, 9, lp, "never")
    # best running score -4.1: / 9 ** 2 beats the worst finished -1.5; / h ** 0 = -4.1 does not
    assert bool(new["improvable"][0]) == improvable and new["go"] == improvable


def test_last_step_everything_hits():
    st = BR.init_state(2, 2, 3, 2, 1)
    st.update(run_scores=torch.tensor([[-0.1, -0.2], [-0.3, -0.4]]), cur_len=2, run_seq=torch.tensor([[[2, 5, 1], [2, 6, 1]], [[2, 7, 1], [2, 8, 1]]]))
    new, info = BR.beam_step(st, _logp([{3: -0.1, 4: -0.2}] * 4), 3, None, 1.0, False)
    assert bool(info["hits"].all()) and not new["go"] and bool(new["fin_flags"].all()) and new["fin_len"].tolist() == [[2, 2], [2, 2]]
    seq, sc = BR.finalize(new, 1)
    assert seq.tolist() == [[2, 5, 3], [2, 7, 3]] and torch.allclose(sc, torch.tensor([-0.2 / 2, -0.4 / 2]))


def test_order_rule_lower_index_first_and_nan_last():
    v, i = BR.topk_ordered(torch.tensor([[1.0, float("nan"), 3.0, 3.0, float("-inf"), 1.0]]), 6)
    assert i.tolist() == [[2, 3, 0, 5, 4, 1]]


def _tiny_ved(**gen):
    enc = D.TrOCREncoder(image_size=32, patch_size=16, hidden_size=256, num_hidden_layers=1, num_attention_heads=4, intermediate_size=256)
    dec = D.TrOCRForCausalLM(d_model=256, decoder_layers=1, decoder_attention_heads=4, decoder_ffn_dim=512, vocab_size=300, max_position_embeddings=64)
    return D.VisionEncoderDecoderModel(enc, dec, gen or None)


ENC = torch.zeros(1, 5, 256)


@pytest.mark.parametrize("kw", [dict(num_beams=4, do_sample=True), dict(num_beams=4, num_beam_groups=2), dict(num_beams=4, no_repeat_ngram_size=3),
                                dict(num_beams=4, repetition_penalty=1.2), dict(num_beams=4, min_length=5), dict(num_beams=4, forced_eos_token_id=2),
                                dict(num_beams=4, suppress_tokens=[3]), dict(num_beams=4, eos_token_id=[2, 3])])
def test_model_beam_search_refuses_what_generate_refuses(kw):
    with pytest.raises(NotImplementedError):
        _tiny_ved().beam_search(encoder_hidden_states=ENC, **kw)


@pytest.mark.parametrize("kw", [dict(), dict(num_beams=1), dict(num_beams=17), dict(num_beams=4, num_return_sequences=5),
                                dict(num_beams=4, early_stopping="sometimes"), dict(num_beams=4, max_length=65), dict(num_beams=4, max_length=0)])
def test_model_beam_search_value_errors(kw):
    with pytest.raises(ValueError):
        _tiny_ved().beam_search(encoder_hidden_states=ENC, **kw)


def test_model_beam_search_shape_and_call_checks():
    m = _tiny_ved()
    with pytest.raises(ValueError, match="64 rows"):
        m.beam_search(encoder_hidden_states=torch.zeros(17, 5, 256), num_beams=4)
    with pytest.raises(ValueError):
        m.beam_search(encoder_hidden_states=torch.zeros(1, 5, 128), num_beams=4)
    with pytest.raises(ValueError):
        m.beam_search(num_beams=4)
    with pytest.raises(TypeError):
        m.beam_search(encoder_hidden_states=ENC, num_beams=4, output_scores=True)
    small = D.VisionEncoderDecoderModel(D.TrOCREncoder(image_size=32, patch_size=16, hidden_size=256, num_hidden_layers=1, num_attention_heads=4, intermediate_size=256),
                                        D.TrOCRForCausalLM(d_model=256, decoder_layers=1, decoder_attention_heads=4, decoder_ffn_dim=512, vocab_size=20))
    with pytest.raises(ValueError, match="vocab_size"):
        small.beam_search(encoder_hidden_states=ENC, num_beams=16)
    # settings come from the generation config; all checks pass, then the CPU tensor is refused at the device's door
    cfgd = _tiny_ved(num_beams=4, early_stopping=True, length_penalty=2.0)
    with pytest.raises(RuntimeError, match="GPU"):
        cfgd.beam_search(encoder_hidden_states=ENC)
    with pytest.raises(NotImplementedError, match="beam_search"):             # generate() still refuses, and names the new method
        cfgd.generate(encoder_hidden_states=ENC)


def test_decoder_beam_search_argument_checks():
    dec = _tiny_ved().decoder
    for kw in (dict(num_beams=1), dict(num_beams=17), dict(num_beams=2.0), dict(num_beams=4, num_return_sequences=0),
               dict(num_beams=4, early_stopping=1), dict(num_beams=4, early_stopping="always")):
        with pytest.raises(ValueError):
            dec.beam_search(ENC, 10, 2, 2, 1, **kw)
    with pytest.raises(ValueError):
        dec.beam_search(ENC, 65, 2, 2, 1, num_beams=4)
    with pytest.raises(ValueError):
        dec.beam_search(torch.zeros(33, 5, 256), 10, 2, 2, 1, num_beams=2)
    with pytest.raises(ValueError):
        dec.beam_search(torch.zeros(5, 256), 10, 2, 2, 1, num_beams=2)


def test_beam_entries_are_declared_and_exported():
    hdr = open(os.path.join(os.path.dirname(HERE), "include", "diffute_hip.h")).read()
    want = {"dmx_trocr_dec_beam_cache_bytes", "dmx_trocr_dec_beam_workspace_bytes", "dmx_trocr_dec_beam_begin", "dmx_trocr_dec_beam_step",
            "dmx_trocr_dec_beam_finalize", "dmx_trocr_dec_beam_launches_per_step", "dmx_trocr_dec_beam_select", "dmx_trocr_dec_beam_attn"}
    declared = set(re.findall(r"\b(dmx_trocr_dec_beam_[a-z0-9_]+)\s*\(", hdr))
    assert want <= declared and declared <= set(_cabi.exported_symbols())
    lib = _cabi.lib()
    assert all(hasattr(lib, s) for s in declared)
    for name, val in (("RUN_SCORE", _cabi.BEAM_RUN_SCORE), ("FIN_SCORE", _cabi.BEAM_FIN_SCORE), ("FIN_FLAG", _cabi.BEAM_FIN_FLAG),
                      ("FIN_LEN", _cabi.BEAM_FIN_LEN), ("IMPROVABLE", _cabi.BEAM_IMPROVABLE), ("PARENT", _cabi.BEAM_PARENT),
                      ("STEPS", _cabi.BEAM_STEPS), ("WORDS", _cabi.BEAM_WORDS)):
        assert int(re.search(rf"#define DMX_TROCR_BEAM_{name} (\d+)", hdr).group(1)) == val
    dec = D.TrOCRForCausalLM()
    assert dec.beam_launches_per_step == dec.launches_per_step + 1 <= dec.launches_per_step + 2
    assert lib.dmx_trocr_dec_beam_state_bytes(512) == (640 + 160 * 512) * 4
    assert lib.dmx_trocr_dec_beam_select_workspace_bytes(4, 16, 50265) > 0 and lib.dmx_trocr_dec_beam_select_workspace_bytes(4, 17, 50265) == 0
