"""Beam-search OCR read-back on the GPU (app.ipynb:845 with a checkpoint's own beam settings): the selection kernel against the
restatement on supplied logits, the decode attention with the ancestry table and the row -> item mapping, the tiny decoders
against transformers' fixture, the full-size decoder, bit-reproducibility, the early stop and VisionEncoderDecoderModel.beam_search.

The fixtures' encoder states are searched (scripts/pin_trocr_beam_oracle.py) so that every step's top K + 1 candidates lie at
least 0.25 apart: random encoder states leave gaps of 0.008 ... 0.044, below twice the bf16 log-prob error (measured on the MI355X:
max |diff| 2.4e-2 ... 3.0e-2 on random states), and such a fixture cannot decide the comparison with transformers.
Each test prints the figures it measures."""
import ast
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import diffute_amd as D
from diffute_amd import _cabi, ocr
from util import assert_close
import trocr_restatement as R
import trocr_beam_restatement as BR
from test_trocr_gpu import FULL_REL, TINY_TF_ABS, _bf16_elem, _full_params

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(__file__), "golden", "trocr_beam_transformers.npz")
GREEDY_GOLDEN = os.path.join(os.path.dirname(__file__), "golden", "trocr_transformers.npz")
DEV = torch.device("cuda:0")
ES = {False: 0, True: 1, "never": 2}
W = _cabi.BEAM_WORDS


def _ptr(t):
    return None if t is None else _cabi.ptr(t)


class Select:
    """the selection op on supplied logits, its state in guarded buffers (sentinel bands around every output)"""
    GUARD = 64

    def __init__(self, B, nb, V, max_len):
        self.B, self.nb, self.V, self.max_len, self.M = B, nb, V, max_len, B * nb
        lib = _cabi.lib()
        g = self.GUARD
        self.nstate = lib.dmx_trocr_dec_beam_state_bytes(max_len) // 4
        self.state_buf = torch.full((256 + 2 * g,), -77, dtype=torch.int32, device=DEV)
        self.bs_buf = torch.full((self.nstate + 2 * g,), -77, dtype=torch.int32, device=DEV)
        self.logp_buf = torch.full((self.M * V + 2 * g,), -7.0, dtype=torch.float32, device=DEV)
        self.state, self.bs, self.logp = self.state_buf[g:-g], self.bs_buf[g:-g], self.logp_buf[g:-g].view(self.M, V)
        self.ws = torch.empty(lib.dmx_trocr_dec_beam_select_workspace_bytes(B, nb, V), dtype=torch.uint8, device=DEV)

    def step(self, logits, eos, lp, es, reset, start=2):
        _cabi.check(_cabi.lib().dmx_trocr_dec_beam_select(_ptr(logits), self.B, self.nb, self.V, self.max_len, -1 if eos is None else eos, float(lp),
                                                          ES[es], int(reset), start, _ptr(self.state), _ptr(self.bs), _ptr(self.logp),
                                                          _ptr(self.ws), self.ws.numel(), _cabi.current_stream()), "trocr_dec_beam_select")
        torch.cuda.synchronize()
        g = self.GUARD
        for name, buf, fill in (("state", self.state_buf, -77), ("beam state", self.bs_buf, -77), ("logp", self.logp_buf, -7.0)):
            assert bool((buf[:g] == fill).all()) and bool((buf[-g:] == fill).all()), f"{name}: guard band overwritten"

    def read(self):
        B, nb, M, L = self.B, self.nb, self.M, self.max_len
        bs = self.bs.cpu()
        f = bs.view(torch.float32)
        fin_ids = bs[W + 64 * L:W + 128 * L].view(64, L)[:M].view(B, nb, L).long()
        return dict(pos=int(self.state[0]), done=int(self.state[1]), stop=int(self.state[2]), tok=self.state[16:16 + M].cpu().long().view(B, nb),
                    run=f[_cabi.BEAM_RUN_SCORE:][:M].view(B, nb), fsc=f[_cabi.BEAM_FIN_SCORE:][:M].view(B, nb),
                    ffl=bs[_cabi.BEAM_FIN_FLAG:][:M].view(B, nb) != 0, fln=bs[_cabi.BEAM_FIN_LEN:][:M].view(B, nb).long(),
                    impr=bs[_cabi.BEAM_IMPROVABLE:][:B] != 0, parent=bs[_cabi.BEAM_PARENT:][:M].view(B, nb).long() % nb, fin_ids=fin_ids)


def _check_step(sel, st, logits, eos, lp, es, first, tag):
    """one device step against the restatement's beam_step on the device's own log-probs; returns the new restatement state"""
    sel.step(logits, eos, lp, es, reset=first)
    logp = sel.logp.cpu()
    ref = F.log_softmax(logits.cpu(), -1)
    ok = torch.isfinite(ref)
    assert float((logp - ref)[ok].abs().max()) <= 4e-6 * max(1.0, float(ref[ok].abs().max())), f"{tag}: log-probs"   # a few fp32 ulp of the lse
    new, info = BR.beam_step(st, logp, sel.max_len, eos, lp, es)
    d = sel.read()
    assert torch.equal(d["parent"], info["new_parent"]) and torch.equal(d["tok"], info["new_token"]), \
        f"{tag}: parents / tokens {d['parent'].tolist()} {d['tok'].tolist()} vs {info['new_parent'].tolist()} {info['new_token'].tolist()}"
    assert torch.equal(d["run"].view(torch.int32), new["run_scores"].view(torch.int32)), f"{tag}: running scores are one fp32 add: bit-equal"
    assert torch.equal(d["ffl"], new["fin_flags"]) and torch.equal(d["fln"], new["fin_len"]), f"{tag}: finished flags / lengths"
    assert torch.allclose(d["fsc"], new["fin_scores"], rtol=1e-6, atol=0), f"{tag}: finished scores {d['fsc']} vs {new['fin_scores']}"
    assert torch.equal(d["impr"], new["improvable"]) and d["done"] == int(not new["go"]) and d["pos"] == new["cur_len"] - 1, f"{tag}: loop state"
    for b in range(sel.B):
        for k in range(sel.nb):
            n = int(new["fin_len"][b, k]) + 1
            assert torch.equal(d["fin_ids"][b, k, :n], new["fin_seq"][b, k, :n]), f"{tag}: finished ids of slot {b},{k}"
    return new


@pytest.mark.parametrize("V", [997, 50265])
@pytest.mark.parametrize("B,nb", [(1, 2), (1, 3), (3, 4), (16, 4), (4, 16)])
def test_beam_select_vs_restatement(V, B, nb):
    M, max_len = B * nb, 6
    g = torch.Generator().manual_seed(V + 31 * B + nb)
    sel = Select(B, nb, V, max_len)
    st = BR.init_state(B, nb, max_len, 2, 1)
    eos = 5
    for t in range(max_len - 1):
        logits = (torch.randn(M, V, generator=g) * 3.0)
        if t == 0:
            logits[:, V - 3] = 40.0                                # a row maximum in the ragged last 64-tile
        if t == 1:
            logits[0::2, eos] = 25.0                               # eos leads in some rows: rank < nb finishes, rank >= nb does not
        if t == 2:
            logits[:, eos] = 30.0
        st = _check_step(sel, st, logits.to(DEV), eos, 2.0 if nb != 3 else 0.0, (True if nb == 4 else "never" if nb == 3 else False), t == 0,
                         f"V={V} B={B} nb={nb} step {t}")
        if not st["go"]:
            break


@pytest.mark.parametrize("V", [997, 50265])
def test_beam_select_ties_pick_the_lowest_flat_index(V):
    """equal candidates within a 64-tile, across tiles, across selection chunks and across beams"""
    B, nb, max_len = 2, 3, 5
    sel = Select(B, nb, V, max_len)
    st = BR.init_state(B, nb, max_len, 2, 1)
    g = torch.Generator().manual_seed(V)
    base = torch.randn(1, V, generator=g)
    # step 1: all rows share one logits row (only beam 0 is alive), with five tokens tied at the top
    ties = [7, 23, 65, V // 2 + 3, V - 1]
    base[0, ties] = 9.0
    logits = base.repeat(B * nb, 1).contiguous()
    st = _check_step(sel, st, logits.to(DEV), None, 1.0, False, True, f"V={V} ties step 0")
    assert st["run_seq"][0, :, 1].tolist() == ties[:nb]
    # step 2: make the beams' running scores equal by hand, then identical rows tie across beams as well
    f = sel.bs.view(torch.float32)
    f[_cabi.BEAM_RUN_SCORE:_cabi.BEAM_RUN_SCORE + B * nb] = -1.5
    st["run_scores"] = torch.full((B, nb), -1.5)
    st = _check_step(sel, st, logits.to(DEV), None, 1.0, False, False, f"V={V} ties step 1")
    assert st["run_seq"][0, :, 1].tolist() == [ties[0]] * nb and st["run_seq"][0, :, 2].tolist() == ties[:nb], st["run_seq"][0]


@pytest.mark.parametrize("L", [1, 7, 64, 65, 511])
def test_dec_attention_with_ancestry_table(L):
    lib = _cabi.lib()
    M, H, Dm, P = 5, 16, 1024, 8                                   # P physical rows; rows 5 .. 7 are NaN and never named
    g = torch.Generator().manual_seed(L)
    q = (torch.randn(M, Dm, generator=g) * 0.125).to(DEV)
    kv = torch.randn(P, L + 2, 2 * Dm, generator=g).to(torch.bfloat16)
    kv[M:] = float("nan")
    kv = kv.to(DEV)
    table = torch.randint(0, M, (M, max(L - 1, 1)), generator=g, dtype=torch.uint8).to(DEV)
    ws = torch.empty(lib.dmx_trocr_dec_attn_workspace_bytes(M, H, L), dtype=torch.uint8, device=DEV)
    out = torch.empty(M, Dm, dtype=torch.bfloat16, device=DEV)
    _cabi.check(lib.dmx_trocr_dec_beam_attn(_ptr(q), M, H, _ptr(kv), (L + 2) * 2 * Dm, 2 * Dm, L, _ptr(table), table.shape[1], 0, _ptr(out),
                                            _ptr(ws), ws.numel(), _cabi.current_stream()), "trocr_dec_beam_attn")
    torch.cuda.synchronize()
    rows = torch.cat([table[:, :L - 1].long(), torch.arange(M, device=DEV)[:, None]], 1)            # [M][L]
    sel = kv[rows, torch.arange(L, device=DEV)[None, :]].float()                                   # [M][L][2 Dm]
    k = sel[..., :Dm].view(M, L, H, 64).transpose(1, 2); v = sel[..., Dm:].view(M, L, H, 64).transpose(1, 2)
    ref = (torch.softmax(q.view(M, H, 1, 64) @ k.transpose(-1, -2), -1) @ v).view(M, H * 64)
    assert_close(out, ref, 4e-3, f"table attn L={L}")
    assert bool(((out.float() - ref).abs().cpu() <= _bf16_elem(ref) + 1e-4).all()), f"table attn L={L}: element beyond one bf16 step"
    # a null table is the existing entry, bit for bit
    kv2 = torch.randn(M, L + 2, 2 * Dm, generator=g).to(torch.bfloat16).to(DEV)
    a = torch.empty(M, Dm, dtype=torch.bfloat16, device=DEV); b = torch.empty_like(a)
    _cabi.check(lib.dmx_trocr_dec_beam_attn(_ptr(q), M, H, _ptr(kv2), (L + 2) * 2 * Dm, 2 * Dm, L, None, 0, 0, _ptr(a), _ptr(ws), ws.numel(),
                                            _cabi.current_stream()), "trocr_dec_beam_attn")
    _cabi.check(lib.dmx_trocr_dec_attn(_ptr(q), M, H, _ptr(kv2), (L + 2) * 2 * Dm, 2 * Dm, L, _ptr(b), _ptr(ws), ws.numel(), _cabi.current_stream()),
                "trocr_dec_attn")
    torch.cuda.synchronize()
    assert torch.equal(a.view(torch.int16), b.view(torch.int16))


@pytest.mark.parametrize("S", [45, 577])
def test_cross_attention_row_to_item(S):
    lib = _cabi.lib()
    nb, B, H, Dm = 3, 2, 16, 1024
    M = B * nb
    g = torch.Generator().manual_seed(S)
    q = (torch.randn(M, Dm, generator=g) * 0.125).to(DEV)
    kv = torch.randn(B, S, 2 * Dm, generator=g).to(torch.bfloat16).to(DEV)
    ws = torch.empty(lib.dmx_trocr_dec_attn_workspace_bytes(M, H, S), dtype=torch.uint8, device=DEV)
    out = torch.empty(M, Dm, dtype=torch.bfloat16, device=DEV)
    _cabi.check(lib.dmx_trocr_dec_beam_attn(_ptr(q), M, H, _ptr(kv), S * 2 * Dm, 2 * Dm, S, None, 0, nb, _ptr(out), _ptr(ws), ws.numel(),
                                            _cabi.current_stream()), "trocr_dec_beam_attn")
    torch.cuda.synchronize()
    kvr = kv.float().repeat_interleave(nb, 0)
    k = kvr[..., :Dm].view(M, S, H, 64).transpose(1, 2); v = kvr[..., Dm:].view(M, S, H, 64).transpose(1, 2)
    ref = (torch.softmax(q.view(M, H, 1, 64) @ k.transpose(-1, -2), -1) @ v).view(M, H * 64)
    assert_close(out, ref, 4e-3, f"cross attn S={S}")
    assert bool(((out.float() - ref).abs().cpu() <= _bf16_elem(ref) + 1e-4).all())


# ---- end to end
def _cases():
    z = np.load(GOLDEN)
    return sorted({k.split("/")[0] for k in z.files})


def _case(name):
    z, zg = np.load(GOLDEN), np.load(GREEDY_GOLDEN)
    s = ast.literal_eval(str(z[name + "/settings"]))
    cfg = ast.literal_eval(str(zg[s["model"] + "/config"]))
    meta = ast.literal_eval(str(zg["meta"]))
    return s, cfg, meta, {k: torch.from_numpy(z[f"{name}/{k}"]) for k in ("enc", "ids", "scores", "gaps")}


def _replay(trace, B, nb, max_len, start, pad, eos, lp, es, nret):
    """the restatement's beam_step over the device's own traced log-probs: every step's state must match; returns its output"""
    st = BR.init_state(B, nb, max_len, start, pad)
    for t, tr in enumerate(trace):
        assert torch.equal(tr["running_scores"].cpu().view(B, nb).view(torch.int32), st["run_scores"].view(torch.int32)), f"step {t}: running scores"
        assert torch.equal(tr["input_tokens"].cpu().long().view(B, nb), st["run_seq"][:, :, t]), f"step {t}: input tokens"
        st, info = BR.beam_step(st, tr["logp"].cpu(), max_len, eos, lp, es)
        assert torch.equal(tr["parent"].cpu().long().view(B, nb), info["new_parent"]) and torch.equal(tr["token"].cpu().long().view(B, nb), info["new_token"]), f"step {t}"
        assert torch.equal(tr["sequences"].cpu().view(B, nb, -1), st["run_seq"][:, :, :t + 2]), f"step {t}: running sequences from the table"
    assert not st["go"] or st["cur_len"] == max_len, "the device stopped although the restatement's loop condition holds"
    return BR.finalize(st, nret)


def _teacher_forced_error(P, cfg, trace, enc_rows):
    """max |traced log-prob - restatement log-prob| with the restatement teacher-forced on the device's own running sequences"""
    worst = 0.0
    for t, tr in enumerate(trace):
        ids = trace[t - 1]["sequences"].cpu() if t else tr["input_tokens"].cpu().long()[:, None]
        ref = F.log_softmax(R.forward(P, cfg, ids, enc_rows)[:, -1].float(), -1)
        worst = max(worst, float((tr["logp"].cpu() - ref).abs().max()))
    return worst


def _assert_normalised(trace, tag):
    """every traced row is a log-softmax: logsumexp = 0.  The log-sum-exp comes from the LM head's per-block partials (ragged last
    tile included); an fp32 lse of magnitude ~10 carries a few ulp, ~1e-6, so 1e-5 holds with room and a dropped tile does not"""
    worst = max(float(torch.logsumexp(tr["logp"].double(), -1).abs().max()) for tr in trace)
    print(f"{tag}: max |logsumexp(traced log-probs)| over {len(trace)} steps {worst:.3e}")
    assert worst <= 1e-5, f"{tag}: traced log-probs are not normalised: {worst:.3e}"


@pytest.mark.parametrize("name", _cases() if os.path.exists(GOLDEN) else ["missing-golden"])
def test_tiny_beam_search_vs_transformers_fixture(name):
    s, cfg, meta, f = _case(name)
    m = D.TrOCRForCausalLM(seed=meta["seed"], device=DEV, decoder_start_token_id=meta["start"], pad_token_id=meta["pad"], **cfg)
    enc = f["enc"].to(DEV)
    B, nb, nret = enc.shape[0], s["num_beams"], s["num_return_sequences"]
    ids, scores, trace = m.beam_search(enc, s["max_length"], meta["start"], s["eos"], meta["pad"], num_beams=nb, length_penalty=s["length_penalty"],
                                       early_stopping=s["early_stopping"], num_return_sequences=nret, keep_trace=True)
    assert m.beam_launches_per_step <= m.launches_per_step + 2
    # (a) the traced log-probs against the teacher-forced restatement on the device's own sequences (a wrong cache reorder shows here)
    P = _full_params(m)
    err = _teacher_forced_error(P, cfg, trace, f["enc"].repeat_interleave(nb, 0))
    print(f"{name}: traced log-probs max |diff| {err:.3e} (bound {2 * TINY_TF_ABS:.1e}), fixture min gap {float(f['gaps'].min()):.3e}")
    assert err <= 2 * TINY_TF_ABS, f"{name}: log-prob max |diff| {err:.3e}"
    _assert_normalised(trace, name)
    # (b) the bookkeeping, exactly, on the device's own log-probs
    r_ids, r_scores = _replay(trace, B, nb, s["max_length"], meta["start"], meta["pad"], s["eos"], s["length_penalty"], s["early_stopping"], nret)
    assert torch.equal(ids.cpu(), r_ids), f"{name}: {ids.tolist()} vs replay {r_ids.tolist()}"
    assert torch.allclose(scores.cpu(), r_scores, rtol=1e-6, atol=0)
    # (c) transformers' output, decided by gaps wider than twice the measured log-prob error (or the fixture is unfit)
    assert float(f["gaps"].min()) > 2 * err, f"{name}: fixture gap {float(f['gaps'].min()):.3e} does not exceed twice the log-prob error {err:.3e}"
    assert torch.equal(ids.cpu(), f["ids"]), f"{name}: {ids.tolist()} vs transformers {f['ids'].tolist()}"
    assert float((scores.cpu() - f["scores"]).abs().max()) <= 2 * err


@pytest.fixture(scope="module")
def full():
    m = D.TrOCRForCausalLM(device=DEV)
    enc = torch.randn(2, 577, 1024, generator=torch.Generator().manual_seed(31)).to(DEV)
    return m, enc


def test_full_size_beam_search(full):
    """(a) against the CPU restatement at three of the eleven steps (the fp32 forward of the full model is slow), the row
    normalisation and (b) the exact replay at every step"""
    m, enc = full
    cfg = dict(D.TROCR_LARGE_DECODER_CONFIG)
    ids, scores, trace = m.beam_search(enc, 12, 2, None, 1, num_beams=4, length_penalty=2.0, keep_trace=True)
    assert ids.shape == (2, 12) and len(trace) == 11
    P = _full_params(m)
    enc_rows = enc.cpu().repeat_interleave(4, 0)
    worst = 0.0
    for t in (0, 5, 10):                                          # (a) at three steps: the CPU forward of the full model is slow
        tr = trace[t]
        seq = trace[t - 1]["sequences"].cpu() if t else tr["input_tokens"].cpu().long()[:, None]
        ref = R.forward(P, cfg, seq, enc_rows)[:, -1].float()
        lref = F.log_softmax(ref, -1)
        e = float((tr["logp"].cpu() - lref).norm() / lref.norm())
        worst = max(worst, e)
    print(f"full size: traced log-probs rel-L2 {worst:.3e}")
    assert worst <= FULL_REL
    _assert_normalised(trace, "full size")
    r_ids, r_scores = _replay(trace, 2, 4, 12, 2, 1, None, 2.0, False, 1)
    assert torch.equal(ids.cpu(), r_ids) and torch.allclose(scores.cpu(), r_scores, rtol=1e-6, atol=0)


def test_beam_search_is_bit_reproducible(full):
    m, enc = full
    kw = dict(num_beams=3, length_penalty=1.0, keep_trace=True)
    a = m.beam_search(enc[:1], 7, 2, None, 1, **kw)
    b = m.beam_search(enc[:1], 7, 2, None, 1, **kw)
    c = m.beam_search(enc[:1], 7, 2, None, 1, use_graph=False, **kw)
    for o in (b, c):
        assert torch.equal(a[0], o[0]) and torch.equal(a[1].view(torch.int32), o[1].view(torch.int32))
        assert all(torch.equal(x["logp"].view(torch.int32), y["logp"].view(torch.int32)) for x, y in zip(a[2], o[2]))


def test_beam_search_stops_early_on_the_device():
    s, cfg, meta, f = _case(_cases()[0])
    m = D.TrOCRForCausalLM(seed=meta["seed"], device=DEV, decoder_start_token_id=meta["start"], pad_token_id=meta["pad"], **cfg)
    enc = f["enc"][:1].to(DEV)
    # an eos id with which both finished slots fill early: found with the CPU restatement among the first steps' candidates
    P = _full_params(m)
    first = BR.beam_search(P, cfg, f["enc"][:1], 4, meta["start"], None, meta["pad"], 2, 1.0, True, 1)[2]
    eos = None
    for tok in dict.fromkeys(int(t) for i in first for t in i["token"][0]):
        if len(BR.beam_search(P, cfg, f["enc"][:1], 40, meta["start"], tok, meta["pad"], 2, 1.0, True, 1)[2]) <= 8:
            eos = tok
            break
    assert eos is not None, "no candidate token of the first steps ends the search early"
    ids, scores, trace = m.beam_search(enc, 40, meta["start"], eos, meta["pad"], num_beams=2, early_stopping=True, keep_trace=True)
    r = m._runs[("beam", 1, 2, enc.shape[1], 40)]
    stop, steps = int(r["cache"][:16].view(torch.int32)[2]), int(r["words"][_cabi.BEAM_STEPS])
    assert int(r["cache"][:16].view(torch.int32)[1]) == 1 and stop < 40, "the search did not end on the device"
    assert steps <= stop - 1 + 2 * ocr.POLL_EVERY, f"{steps} steps ran for a search that stopped at length {stop}"
    assert len(trace) == stop - 1 and ids.shape[1] <= stop
    r_ids, _ = _replay(trace, 1, 2, 40, meta["start"], meta["pad"], eos, 1.0, True, 1)
    assert torch.equal(ids.cpu(), r_ids)


def test_vision_encoder_decoder_beam_search(tmp_path):
    import transformers  # noqa: F401  (a missing library fails this test: it is the only model-level beam_search run)
    from test_trocr_host import _save_tiny
    _save_tiny(tmp_path, gen_extra=dict(num_beams=4, early_stopping=True))
    model = D.VisionEncoderDecoderModel.from_pretrained(str(tmp_path)).to(DEV)
    g = model.generation_config
    assert g.num_beams == 4 and g.early_stopping is True
    px = torch.randn(2, 3, 32, 32, generator=torch.Generator().manual_seed(3)).to(DEV)
    ids, sc = model.beam_search(px, return_scores=True)
    assert ids.dtype == torch.int64 and ids.device.type == "cuda" and ids.shape[0] == 2 and sc.shape == (2,)
    enc = model.encoder(px).last_hidden_state
    ids2, sc2 = model.beam_search(encoder_hidden_states=enc, return_scores=True)
    assert torch.equal(ids, ids2) and torch.equal(sc, sc2)
    d_ids, d_sc, _ = model.decoder.beam_search(enc, 20, g.decoder_start_token_id, g.eos_token_id, g.pad_token_id, num_beams=4, early_stopping=True)
    assert torch.equal(ids, d_ids)
    with pytest.raises(NotImplementedError, match="num_beams"):
        model.generate(px)
