"""Teacher-forced OCR scoring on the GPU: the prefill kernels on their own (causal attention, fused LM head + loss), the tiny
decoders against transformers' fixtures, the full-size decoder against the CPU restatement, independence and reproducibility.
Tile sizes the shapes straddle: the causal attention takes 16 queries per block and walks 32-key tiles; the LM head takes 64 rows
x 64 vocabulary entries per block (16 entries per wave) and merges the tiles of a row 64 at a time."""
import ast
import os

import numpy as np
import pytest
import torch

import diffute_amd as D
from diffute_amd import _cabi
from util import rel_l2
import trocr_restatement as R

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(__file__)
TINY_GOLDEN = os.path.join(HERE, "golden", "trocr_transformers.npz")
SCORE_GOLDEN = os.path.join(HERE, "golden", "trocr_score_transformers.npz")
DEV = torch.device("cuda:0")
IGNORE = -100
# the step path's bounds (tests/test_trocr_gpu.py): they hold for the prefill too
FULL_REL = 2e-2
TINY_TF_REL, TINY_TF_ABS = 1e-2, 6e-2
SENTINEL = 777.0


def _ptr(t):
    return None if t is None else _cabi.ptr(t)


# ---------------------------------------------------------------------------- causal attention
def _attn(fused, out, col, B, H, T, D):
    """q | k | v = column slices [0, D), [D, 2D), [2D, 3D) of `fused`; the output goes to columns [col, col + D) of `out`"""
    lib = _cabi.lib()
    es = fused.element_size()
    _cabi.check(lib.dmx_trocr_dec_prefill_attn(fused.data_ptr(), fused.shape[1], fused.data_ptr() + D * es, fused.shape[1],
                                               fused.data_ptr() + 2 * D * es, fused.shape[1], out.data_ptr() + col * es, out.shape[1],
                                               B, H, T, 0.125, _cabi.current_stream()), "trocr_dec_prefill_attn")
    torch.cuda.synchronize()


# T: 1 and 2 (the smallest), 15 / 16 / 17 (the 16-query tile), 33 (the 32-key tile), 65 (two key tiles and one key), 130 (nine query tiles)
@pytest.mark.parametrize("T", [1, 2, 15, 16, 17, 33, 65, 130])
@pytest.mark.parametrize("B,H", [(1, 1), (3, 4)])
def test_prefill_attention(T, B, H):
    Dm = H * 64
    g = torch.Generator().manual_seed(T * 31 + B)
    fused = torch.randn(B * T, 3 * Dm + 8, generator=g).to(torch.bfloat16).to(DEV)       # (8 spare columns: never read)
    col, ldo, guard = 8, Dm + 24, 2
    full = torch.full((B * T + 2 * guard, ldo), SENTINEL, dtype=torch.bfloat16, device=DEV)
    out = full[guard:guard + B * T]
    _attn(fused, out, col, B, H, T, Dm)
    f = fused.double().cpu()
    q, k, v = (f[:, i * Dm:(i + 1) * Dm].view(B, T, H, 64).transpose(1, 2) for i in range(3))
    s = (q @ k.transpose(-1, -2)) * 0.125
    s = s.masked_fill(torch.triu(torch.ones(T, T, dtype=torch.bool), 1), float("-inf"))
    ref = (torch.softmax(s, -1) @ v).transpose(1, 2).reshape(B * T, Dm)                   # fp64 on the rounded operands
    got = out[:, col:col + Dm].double().cpu()
    assert bool((full[:guard] == SENTINEL).all()) and bool((full[guard + B * T:] == SENTINEL).all()), "guard rows overwritten"
    assert bool((out[:, :col] == SENTINEL).all()) and bool((out[:, col + Dm:] == SENTINEL).all()), "guard columns overwritten"
    assert bool((out[:, col:col + Dm] != SENTINEL).all()), "an output element was never written"
    e = float((got - ref).norm() / ref.norm())
    assert e <= 4e-3, f"T={T}: rel-L2 {e:.3e}"
    assert bool(((got - ref).abs() <= ref.abs() * 2.0 ** -7 + 1e-5 + 1e-4).all()), f"T={T}: element beyond one bf16 step + 1e-4"
    if T > 1:                                                      # causality: keys / values behind position t0 do not reach rows <= t0
        t0 = T // 2 - 1 if T > 2 else 0
        f2 = fused.clone().view(B, T, -1)
        f2[:, t0 + 1:, Dm:3 * Dm] = (torch.randn(B, T - t0 - 1, 2 * Dm, generator=g) * 3).to(torch.bfloat16).to(DEV)
        full2 = torch.full_like(full, SENTINEL)
        out2 = full2[guard:guard + B * T]
        _attn(f2.view(B * T, -1), out2, col, B, H, T, Dm)
        a = out.view(B, T, ldo)[:, :t0 + 1, col:col + Dm].contiguous().view(torch.int16)
        b = out2.view(B, T, ldo)[:, :t0 + 1, col:col + Dm].contiguous().view(torch.int16)
        assert torch.equal(a, b), f"T={T}: rows <= {t0} changed with the keys / values behind them"
        assert not torch.equal(out.view(B, T, ldo)[:, t0 + 1:], out2.view(B, T, ldo)[:, t0 + 1:])


# ---------------------------------------------------------------------------- fused LM head + loss
def _lm(x, w, labels, want_logits, ld=None):
    lib = _cabi.lib()
    M, K = x.shape
    V = w.shape[0]
    ws = torch.empty(lib.dmx_trocr_dec_prefill_lm_loss_workspace_bytes(M, V), dtype=torch.uint8, device=DEV)
    ld = ld or V
    logits = torch.full((M, ld), SENTINEL, dtype=torch.float32, device=DEV) if want_logits else None
    logp = torch.empty(M, dtype=torch.float32, device=DEV) if labels is not None else None
    amax = torch.empty(M, dtype=torch.int32, device=DEV)
    _cabi.check(lib.dmx_trocr_dec_prefill_lm_loss(_ptr(x), M, K, _ptr(w), V, _ptr(labels), IGNORE, _ptr(logp), _ptr(amax), _ptr(logits), ld,
                                                  _ptr(ws), ws.numel(), _cabi.current_stream()), "trocr_dec_prefill_lm_loss")
    torch.cuda.synchronize()
    return logp, amax, logits


def _labels(M, V, g):
    lab = torch.randint(0, V, (M,), generator=g)
    for i, v in enumerate((0, V - 1, V - 1 - (V - 1) % 64 + ((V - 1) % 64) // 2, IGNORE)):   # first, last, inside the ragged last tile, ignored
        if i < M:
            lab[(i * 5) % M if M > 3 else i] = v
    return lab.to(DEV)


def _check_lm(x, w, lab, name):
    M, V = x.shape[0], w.shape[0]
    ref = x.double() @ w.double().T                                # fp64 on the same bf16 operands
    logp, amax, logits = _lm(x, w, lab, True, ld=V + 3)
    assert bool((logits[:, V:] == SENTINEL).all()), f"{name}: logits written beyond the vocabulary"
    lg = logits[:, :V].double()
    scale = float(ref.abs().max())
    e = float((lg - ref).norm() / ref.norm())
    worst = float((lg - ref).abs().max())
    assert e <= 1e-3 and worst <= 2e-3 * scale, f"{name}: logits rel-L2 {e:.3e}, max |diff| {worst:.3e} (bound {2e-3 * scale:.3e})"
    keep = lab != IGNORE
    lp_ref = torch.log_softmax(ref, -1).gather(-1, lab.clamp(min=0)[:, None])[:, 0]
    lp_ref = torch.where(keep, lp_ref, torch.zeros_like(lp_ref))
    assert bool(torch.isfinite(logp).all())
    lw = float((logp.double() - lp_ref).abs().max())
    assert lw <= 2 * 2e-3 * scale, f"{name}: token_logprob max |diff| {lw:.3e} (bound {4e-3 * scale:.3e})"
    assert bool((logp[~keep] == 0).all()), f"{name}: ignored positions must score 0"
    assert torch.equal(amax.long(), torch.argmax(logits[:, :V], -1)), f"{name}: arg-max differs from torch.argmax of the kernel's own logits"
    logp2, amax2, _ = _lm(x, w, lab, False)                        # no logits buffer: the same bits
    assert torch.equal(logp.view(torch.int32), logp2.view(torch.int32)) and torch.equal(amax, amax2), f"{name}: results depend on the logits buffer"
    return logits[:, :V]


# M: 1, 3 (inside one 16-row MFMA tile), 17 (two), 64 (one full block), 130 (three blocks, the last ragged)
# V: 997 / 1000 (16 tiles, the last ragged: 37 / 40 entries), 50265 (786 tiles: the 64-at-a-time merge runs 13 rounds; last tile 25 entries)
@pytest.mark.parametrize("M", [1, 3, 17, 64, 130])
@pytest.mark.parametrize("V,K", [(997, 256), (1000, 256), (50265, 1024)])
def test_prefill_lm_loss(M, V, K):
    g = torch.Generator().manual_seed(M * 7 + V + K)
    x = torch.randn(M, K, generator=g).to(torch.bfloat16).to(DEV)
    w = (torch.randn(V, K, generator=g) * K ** -0.5).to(torch.bfloat16).to(DEV)
    lab = _labels(M, V, g)
    _check_lm(x, w, lab, f"M={M} V={V}")
    # ties: rows equal to row 7 - 23 (same block, another wave), 60 (another lane group), 65 (the next block), V // 2 + 3 (far away: another
    # lane of the merge, another round at V = 50265) and V - 1 (the ragged last tile); every input row is that row, so all of them share the maximum
    w2 = w.clone()
    dup = (23, 60, 65, V // 2 + 3, V - 1)
    for j in dup:
        w2[j] = w2[7]
    xt = w2[7:8].repeat(M, 1).contiguous()
    logits = _check_lm(xt, w2, lab, f"ties M={M} V={V}")
    mx = logits.max(-1).values
    assert bool(((logits == mx[:, None]).sum(-1) >= 6).all()), "ties were not constructed"
    _, amax, _ = _lm(xt, w2, None, False)
    assert bool((amax == 7).all()), f"ties must go to the lowest index: {amax.tolist()}"
    w3 = w2.clone(); w3[7] = w[7] * 0.5                            # without row 7 the lowest duplicate is 23, and so on up to the last tile
    for drop, want in ((7, 23), (23, 60), (60, 65), (65, V // 2 + 3), (V // 2 + 3, V - 1)):
        w3[drop] = w[7] * 0.5
        _, amax, _ = _lm(xt, w3, None, False)
        assert bool((amax == want).all()), f"lowest index after dropping {drop}: {amax.tolist()} != {want}"


def test_prefill_lm_loss_large_logits():
    """logits near +-60: exp() of them overflows fp16 and, unshifted, loses everything in fp32 sums; the log-probs stay finite and in bound"""
    g = torch.Generator().manual_seed(99)
    M, V, K = 17, 1000, 256
    x = (torch.randn(M, K, generator=g) * 14).to(torch.bfloat16).to(DEV)
    w = (torch.randn(V, K, generator=g) * K ** -0.5).to(torch.bfloat16).to(DEV)
    logits = _check_lm(x, w, _labels(M, V, g), "large logits")
    assert 45 < float(logits.abs().max()) < 90


# ---------------------------------------------------------------------------- decoders
def _fixture(name):
    z = np.load(TINY_GOLDEN)
    pre = name + "/"
    cfg = ast.literal_eval(str(z[pre + "config"]))
    meta = ast.literal_eval(str(z["meta"]))
    return cfg, meta, {k[len(pre):]: torch.from_numpy(z[k]) for k in z.files if k.startswith(pre) and k != pre + "config"}


_TINY = {}


def _tiny(name):
    if name not in _TINY:
        cfg, meta, _ = _fixture(name)
        _TINY[name] = D.TrOCRForCausalLM(seed=meta["seed"], device=DEV, decoder_start_token_id=meta["start"], pad_token_id=meta["pad"], **cfg)
    return _TINY[name]


def _held(lp, pred, ref_logits, labels, err, name):
    """log-probs within 2 x the measured logit error (log-sum-exp is 1-Lipschitz in the max norm); the arg-max wherever the reference's
    top-1 - top-2 margin exceeds 2 x that error; returns the decided share"""
    keep = labels != IGNORE
    ref_lp = torch.log_softmax(ref_logits.double(), -1).gather(-1, labels.clamp(min=0)[..., None])[..., 0]
    ref_lp = torch.where(keep, ref_lp, torch.zeros_like(ref_lp))
    lw = float((lp.double().cpu() - ref_lp).abs().max())
    assert lw <= 2 * err, f"{name}: token_logprobs max |diff| {lw:.3e} > 2 x logit error {err:.3e}"
    assert bool((lp.cpu()[~keep] == 0).all())
    decided = R.margins(ref_logits) > 2 * err
    assert torch.equal(pred.cpu()[decided], torch.argmax(ref_logits, -1)[decided]), f"{name}: prediction differs where the margin decides it"
    return float(decided.float().mean())


@pytest.mark.parametrize("name", ["tied_gelu", "untied_relu_scaled"])
def test_tiny_decoder_score_vs_transformers_fixture(name):
    cfg, meta, f = _fixture(name)
    m = _tiny(name)
    tf_ids, ref = f["tf_ids"], f["tf_logits"]
    labels = torch.cat([tf_ids[:, 1:], torch.full((tf_ids.shape[0], 1), 5, dtype=torch.int64)], 1)      # shifted right they are tf_ids
    out = m.score(labels.to(DEV), f["enc"].to(DEV), return_logits=True)
    e, err = rel_l2(out.logits, ref), float((out.logits.cpu() - ref).abs().max())
    print(f"{name}: prefill logits rel-L2 {e:.3e}, max |diff| {err:.3e}")
    assert e <= TINY_TF_REL and err <= TINY_TF_ABS, f"{name}: rel-L2 {e:.3e} / max |diff| {err:.3e}"
    share = _held(out.token_logprobs, out.predictions, ref, labels, err, name)
    print(f"{name}: {share:.2f} of the positions decided by the margin rule")
    assert share > 0.5
    out2 = m.score(None, f["enc"].to(DEV), decoder_input_ids=tf_ids.to(DEV), return_logits=True)           # the same inputs, unshifted
    assert out2.loss is None and out2.token_logprobs is None
    assert torch.equal(out2.logits.view(torch.int32), out.logits.view(torch.int32)) and torch.equal(out2.predictions, out.predictions)


@pytest.mark.parametrize("name", ["tied_gelu", "untied_relu_scaled"])
@pytest.mark.parametrize("T", [9, 1])
def test_score_fixture_through_every_entry(name, T):
    """ragged rows, a -100 in the middle of a row, T = 1: TrOCRForCausalLM.score, VisionEncoderDecoderModel.score and .forward"""
    z = np.load(SCORE_GOLDEN)
    pre = f"{name}/T{T}/"
    cfg, meta, _ = _fixture(name)
    dec = _tiny(name)
    enc = torch.from_numpy(z[pre + "enc"]).to(DEV)
    labels = torch.from_numpy(z[pre + "labels"])
    ref = torch.from_numpy(z[pre + "logits"])
    out = dec.score(labels.to(DEV), enc, return_logits=True)
    err = float((out.logits.cpu() - ref).abs().max())
    print(f"{name} T={T}: logits rel-L2 {rel_l2(out.logits, ref):.3e}, max |diff| {err:.3e}, loss {float(out.loss):.5f} vs {float(z[pre + 'loss']):.5f}")
    assert rel_l2(out.logits, ref) <= TINY_TF_REL and err <= TINY_TF_ABS
    keep = labels != IGNORE
    assert float((out.token_logprobs.cpu() - torch.from_numpy(z[pre + "token_logprobs"])).abs().max()) <= 2 * err
    assert bool((out.token_logprobs.cpu()[~keep] == 0).all()), "ignored positions must score 0"
    assert torch.equal(out.num_tokens.cpu(), keep.sum(1))
    assert torch.equal(out.sequence_logprobs, out.token_logprobs.sum(1))
    assert abs(float(out.loss) - float(z[pre + "loss"])) <= 2 * err
    assert out.predictions.dtype == torch.int64 and out.predictions.shape == labels.shape
    lean = dec.score(labels.to(DEV), enc)
    assert lean.logits is None and torch.equal(lean.token_logprobs.view(torch.int32), out.token_logprobs.view(torch.int32))
    model = D.VisionEncoderDecoderModel(D.TrOCREncoder(device=DEV, image_size=32, patch_size=16, hidden_size=cfg["d_model"], num_hidden_layers=1,
                                                       num_attention_heads=4, intermediate_size=64), dec,
                                        dict(decoder_start_token_id=meta["start"], pad_token_id=meta["pad"]))
    s2 = model.score(encoder_hidden_states=enc, labels=labels.to(DEV))
    assert s2.logits is None and torch.equal(s2.token_logprobs.view(torch.int32), out.token_logprobs.view(torch.int32))
    assert torch.equal(s2.loss.view(torch.int32), out.loss.view(torch.int32)) and s2.loss.ndim == 0
    for eo in ((enc,), type("BaseModelOutput", (), {"last_hidden_state": enc})()):
        fw = model(encoder_outputs=eo, labels=labels.to(DEV))
        assert torch.equal(fw.loss.view(torch.int32), out.loss.view(torch.int32)) and torch.equal(fw.logits.view(torch.int32), out.logits.view(torch.int32))
        assert fw.encoder_last_hidden_state is enc
    fi = model(encoder_outputs=(enc,), decoder_input_ids=torch.from_numpy(z[pre + "decoder_input_ids"]).to(DEV))
    assert fi.loss is None and torch.equal(fi.logits.view(torch.int32), out.logits.view(torch.int32))
    tup = model(encoder_outputs=(enc,), labels=labels.to(DEV), return_dict=False)
    assert torch.equal(tup[0], fw.loss) and torch.equal(tup[1], fw.logits)
    # pixel_values: the encoder's states, then the same decoder pass
    px = torch.randn(3, 3, 32, 32, generator=torch.Generator().manual_seed(3)).to(DEV)
    sp = model.score(px, labels=labels.to(DEV))
    se = model.score(encoder_hidden_states=model.encoder(px).last_hidden_state, labels=labels.to(DEV))
    assert torch.equal(sp.token_logprobs.view(torch.int32), se.token_logprobs.view(torch.int32)) and bool(torch.isfinite(sp.loss))
    allign = dec.score(torch.full_like(labels, IGNORE).to(DEV), enc)
    assert bool(torch.isnan(allign.loss)) and bool((allign.token_logprobs == 0).all()), "every label ignored: NaN, as torch's CrossEntropyLoss"


@pytest.fixture(scope="module")
def full():
    m = D.TrOCRForCausalLM(device=DEV)
    enc = torch.randn(3, 577, 1024, generator=torch.Generator().manual_seed(31)).to(DEV)
    return m, enc


def test_full_size_score_vs_restatement(full):
    m, enc = full
    cfg = dict(D.TROCR_LARGE_DECODER_CONFIG)
    g = torch.Generator().manual_seed(17)
    labels = torch.randint(0, cfg["vocab_size"], (2, 17), generator=g)
    labels[1, 11:] = IGNORE
    out = m.score(labels.to(DEV), enc[:2], return_logits=True)
    P = {k: v.detach().float().cpu() for k, v in m.named_parameters()}
    ids = labels.new_full(labels.shape, 1)
    ids[:, 1:] = labels[:, :-1]; ids[:, 0] = 2
    ids[ids == IGNORE] = 1
    ref = R.forward(P, cfg, ids, enc[:2].cpu())
    e, err = rel_l2(out.logits, ref), float((out.logits.cpu() - ref).abs().max())
    print(f"full size: prefill logits rel-L2 {e:.3e}, max |diff| {err:.3e}")
    assert e <= FULL_REL, f"full-size logits rel-L2 {e:.3e}"
    share = _held(out.token_logprobs, out.predictions, ref, labels, err, "full size")
    print(f"full size: {share:.2f} of the positions decided by the margin rule")


def _bits(t):
    return t.contiguous().view(torch.int32)


def test_independence_and_reproducibility(full):
    """labels[:, t0:] feed the inputs of positions t0 + 1 ...: the logits and predictions of positions <= t0 keep their bits, and so do
    the log-probs up to t0 - 1 whatever label t0 becomes (token_logprobs[t0] gathers label t0 itself) and up to t0 when label t0 is kept"""
    m, enc = full
    V = m.config.vocab_size
    g = torch.Generator().manual_seed(5)
    labels = torch.randint(0, V, (3, 9), generator=g).to(DEV)
    ids0, lg0 = m.greedy(enc[:2], 6, 2, None, 1, keep_logits=True)
    a = m.score(labels, enc, return_logits=True)
    b = m.score(labels, enc)
    assert torch.equal(_bits(a.token_logprobs), _bits(b.token_logprobs)) and torch.equal(a.predictions, b.predictions), "two runs differ"
    # position t0's input is labels[t0 - 1]: changing labels[:, t0:] moves only later inputs
    t0 = 4
    lab2 = labels.clone(); lab2[:, t0:] = torch.randint(0, V, (3, 9 - t0), generator=g).to(DEV)
    c = m.score(lab2, enc, return_logits=True)
    assert torch.equal(_bits(a.logits[:, :t0 + 1]), _bits(c.logits[:, :t0 + 1])), "a later label reached the logits of an earlier position"
    assert torch.equal(a.predictions[:, :t0 + 1], c.predictions[:, :t0 + 1]), "a later label reached an earlier prediction"
    assert torch.equal(_bits(a.token_logprobs[:, :t0]), _bits(c.token_logprobs[:, :t0])), "a later label reached an earlier log-prob"
    same = lab2.clone(); same[:, t0] = labels[:, t0]               # with the label at t0 kept, position t0 scores the same too
    c2 = m.score(same, enc)
    assert torch.equal(_bits(a.token_logprobs[:, :t0 + 1]), _bits(c2.token_logprobs[:, :t0 + 1]))
    for i in range(3):                                             # a row alone = the row inside the batch
        one = m.score(labels[i:i + 1], enc[i:i + 1])
        assert torch.equal(_bits(one.token_logprobs[0]), _bits(a.token_logprobs[i])) and torch.equal(one.predictions[0], a.predictions[i]), f"row {i}"
    # greedy() before and after: shared run buffers and caches
    ids1, lg1 = m.greedy(enc[:2], 6, 2, None, 1, keep_logits=True)
    assert torch.equal(ids0, ids1) and torch.equal(_bits(lg0), _bits(lg1)), "greedy() changed after score()"
    d = m.score(labels, enc)
    assert torch.equal(_bits(a.token_logprobs), _bits(d.token_logprobs)), "score() changed after greedy()"
