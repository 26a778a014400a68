"""OCR read-back, host side (app.ipynb:548/845): the CPU restatement against transformers' fixture (and transformers itself when
importable), the decoder's parameter table against TrOCRForCausalLM, VisionEncoderDecoderModel.from_pretrained on a directory
written by transformers, and the generation-argument checks."""
import ast
import os

import numpy as np
import pytest
import torch

import diffute_amd as D
from diffute_amd.init import init_param
import trocr_restatement as R

GOLDEN = os.path.join(os.path.dirname(__file__), "golden", "trocr_transformers.npz")
NAMES = ["tied_gelu", "untied_relu_scaled"]


def _fixture(name):
    z = np.load(GOLDEN)
    pre = name + "/"
    return (ast.literal_eval(str(z[pre + "config"])), ast.literal_eval(str(z["meta"])),
            {k[len(pre):]: torch.from_numpy(z[k]) for k in z.files if k.startswith(pre) and k != pre + "config"})


def _params(cfg, seed):
    m = D.TrOCRForCausalLM(seed=seed, **cfg)
    return {k: v.detach().float() for k, v in m.named_parameters()}


@pytest.mark.parametrize("name", NAMES)
def test_restatement_matches_transformers_fixture(name):
    cfg, meta, f = _fixture(name)
    P = _params(cfg, meta["seed"])
    tf = R.forward(P, cfg, f["tf_ids"], f["enc"])
    assert float((tf - f["tf_logits"]).abs().max()) <= 1e-5 * max(1.0, float(tf.abs().max()))
    eos = int(f["eos"])
    ids, lg = R.generate(P, cfg, f["enc"], meta["max_length"], meta["start"], None if eos < 0 else eos, meta["pad"])
    assert torch.equal(ids, f["ids"])
    assert torch.allclose(R.margins(lg), f["margins"], atol=1e-5)
    if eos >= 0:                                   # the fixture exercises the finished -> pad rule on one row
        assert (f["ids"] == eos).any() and (f["ids"][:, -1] == meta["pad"]).any() and ids.shape[1] == meta["max_length"]


def test_fixture_is_small():
    assert os.path.getsize(GOLDEN) < 1 << 20


@pytest.mark.parametrize("name", NAMES)
def test_restatement_matches_live_transformers(name):
    pytest.importorskip("transformers")
    from transformers import TrOCRConfig, TrOCRForCausalLM
    cfg, meta, f = _fixture(name)
    m = TrOCRForCausalLM(TrOCRConfig(**cfg, dropout=0.0, attention_dropout=0.0, activation_dropout=0.0)).eval()
    P = {k: init_param(k, tuple(v.shape), seed=meta["seed"]) for k, v in m.state_dict().items()
         if not (k == "output_projection.weight" and cfg["tie_word_embeddings"])}
    m.load_state_dict(P, strict=False)
    with torch.no_grad():
        hf = m(input_ids=f["tf_ids"], encoder_hidden_states=f["enc"], use_cache=False).logits
    tf = R.forward(P, cfg, f["tf_ids"], f["enc"])
    assert float((hf - tf).abs().max()) <= 1e-5 * max(1.0, float(tf.abs().max()))


def test_parameter_table_matches_transformers():
    pytest.importorskip("transformers")
    from transformers import TrOCRConfig, TrOCRForCausalLM
    with torch.device("meta"):
        ref = TrOCRForCausalLM(TrOCRConfig())
    sd = ref.state_dict()
    m = D.TrOCRForCausalLM()
    mine = dict(m.named_parameters())
    assert set(mine) == set(sd) - {"output_projection.weight"}         # tied (the class default): no separate LM head
    assert all(tuple(mine[k].shape) == tuple(sd[k].shape) for k in mine)
    n = sum(p.numel() for p in m.parameters())
    assert n == sum(p.numel() for p in ref.parameters()) == 253_559_808
    assert m.launches_per_step == 2 + 8 * 12
    untied = D.TrOCRForCausalLM(tie_word_embeddings=False, decoder_layers=1, d_model=256, decoder_attention_heads=4, decoder_ffn_dim=512, vocab_size=300)
    assert "output_projection.weight" in dict(untied.named_parameters())


def test_pinned_parameter_count_without_transformers():
    assert sum(p.numel() for p in D.TrOCRForCausalLM().parameters()) == 253_559_808


def test_unsupported_configs_raise():
    with pytest.raises(NotImplementedError):
        D.TrOCRForCausalLM(use_learned_position_embeddings=False)
    with pytest.raises(NotImplementedError):
        D.TrOCRForCausalLM(activation_function="silu")
    enc = D.TrOCREncoder(image_size=32, patch_size=16, hidden_size=128, num_hidden_layers=1, num_attention_heads=2, intermediate_size=256)
    dec = D.TrOCRForCausalLM(d_model=256, decoder_layers=1, decoder_attention_heads=4, decoder_ffn_dim=512, vocab_size=300)
    with pytest.raises(NotImplementedError, match="enc_to_dec_proj"):
        D.VisionEncoderDecoderModel(enc, dec)


def _tiny_ved():
    enc = D.TrOCREncoder(image_size=32, patch_size=16, hidden_size=256, num_hidden_layers=1, num_attention_heads=4, intermediate_size=256)
    dec = D.TrOCRForCausalLM(d_model=256, decoder_layers=1, decoder_attention_heads=4, decoder_ffn_dim=512, vocab_size=300,
                             max_position_embeddings=64)
    return D.VisionEncoderDecoderModel(enc, dec)


@pytest.mark.parametrize("kw", [dict(num_beams=4), dict(do_sample=True), dict(no_repeat_ngram_size=3), dict(repetition_penalty=1.2),
                                dict(min_length=5), dict(forced_eos_token_id=2), dict(num_beams=4, length_penalty=2.0)])
def test_generation_arguments_raise(kw):
    m = _tiny_ved()
    with pytest.raises(NotImplementedError):
        m.generate(encoder_hidden_states=torch.zeros(1, 5, 256), **kw)


def test_beam_only_settings_are_inert_under_greedy_search():
    from diffute_amd.ocr import _check_generation
    _check_generation(dict(num_beams=1, length_penalty=2.0, early_stopping=True), explicit_beams=False)
    _check_generation(dict(num_beams=4, length_penalty=2.0, early_stopping=True), explicit_beams=True)
    with pytest.raises(NotImplementedError, match="remove it"):
        _check_generation(dict(num_beams=1, no_repeat_ngram_size=3), explicit_beams=True)


def test_generation_length_checks():
    m = _tiny_ved()
    with pytest.raises(ValueError):
        m.generate(encoder_hidden_states=torch.zeros(1, 5, 256), max_length=65)
    big = D.VisionEncoderDecoderModel(D.TrOCREncoder(num_hidden_layers=1, intermediate_size=128), D.TrOCRForCausalLM(decoder_layers=1))
    with pytest.raises(ValueError, match="512"):
        big.generate(encoder_hidden_states=torch.zeros(1, 5, 1024), max_length=513)
    with pytest.raises(ValueError):
        m.generate()
    with pytest.raises(TypeError):
        m.generate(encoder_hidden_states=torch.zeros(1, 5, 256), output_scores=True)


def _save_tiny(tmp_path, gen_extra=None, tie=True):
    pytest.importorskip("transformers")
    from transformers import TrOCRConfig, VisionEncoderDecoderConfig, VisionEncoderDecoderModel, ViTConfig
    ec = ViTConfig(image_size=32, patch_size=16, hidden_size=256, num_hidden_layers=1, num_attention_heads=4, intermediate_size=256)
    dc = TrOCRConfig(vocab_size=300, d_model=256, decoder_layers=1, decoder_attention_heads=4, decoder_ffn_dim=512, activation_function="relu",
                     scale_embedding=True, tie_word_embeddings=tie, max_position_embeddings=64)
    hf = VisionEncoderDecoderModel(VisionEncoderDecoderConfig.from_encoder_decoder_configs(ec, dc))
    if gen_extra:
        for k, v in gen_extra.items():
            setattr(hf.generation_config, k, v)
    hf.save_pretrained(str(tmp_path))
    return hf


@pytest.mark.parametrize("tie", [True, False])
def test_from_pretrained_transformers_directory(tmp_path, tie):
    hf = _save_tiny(tmp_path, tie=tie)
    m = D.VisionEncoderDecoderModel.from_pretrained(str(tmp_path))
    assert isinstance(m.encoder, D.TrOCREncoder) and isinstance(m.decoder, D.TrOCRForCausalLM)
    c = m.decoder.config
    assert c.activation_function == "relu" and c.scale_embedding and bool(c.tie_word_embeddings) == tie and c.vocab_size == 300
    ref = hf.decoder.state_dict()
    mine = dict(m.decoder.named_parameters())
    for k, v in mine.items():
        assert torch.equal(v.detach(), ref[k].float()), k
    assert ("output_projection.weight" in mine) == (not tie)
    assert sum(p.numel() for p in m.encoder.parameters()) == sum(p.numel() for k, p in hf.encoder.named_parameters() if not k.startswith("pooler."))
    g = m.generation_config
    assert (g.decoder_start_token_id, g.eos_token_id, g.pad_token_id) == (2, 2, 1)


def test_from_pretrained_refuses_beam_generation_config(tmp_path):
    _save_tiny(tmp_path, gen_extra=dict(num_beams=4, early_stopping=True))
    m = D.VisionEncoderDecoderModel.from_pretrained(str(tmp_path))
    with pytest.raises(NotImplementedError, match="num_beams"):
        m.generate(encoder_hidden_states=torch.zeros(1, 5, 256))
