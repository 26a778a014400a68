"""OCR read-back on the GPU (app.ipynb:548/845): the decoder kernels against fp32 torch, the tiny decoders against transformers'
fixture, the full-size decoder against the CPU restatement, bit-reproducibility, and VisionEncoderDecoderModel.generate."""
import ast
import os

import numpy as np
import pytest
import torch

import diffute_amd as D
from diffute_amd import _cabi
from util import assert_close, rel_l2
import trocr_restatement as R

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(__file__), "golden", "trocr_transformers.npz")
DEV = torch.device("cuda:0")
EPI_STORE, EPI_QKV, EPI_LN, EPI_PICK = 0, 1, 2, 3
# measured on the MI355X (bf16 weights and activations, fp32 accumulation): teacher-forced logits of the tiny decoders
# rel-L2 5.3e-3 / 6.2e-3, max |diff| 2.3e-2 / 2.6e-2 (tied_gelu / untied_relu_scaled); set with headroom.  Full size: 9.7e-3.
FULL_REL = 2e-2
TINY_TF_REL, TINY_TF_ABS = 1e-2, 6e-2


def _ptr(t):
    return None if t is None else _cabi.ptr(t)


def _linear(epi, x, w, bias, act=0, oscale=1.0, yf=None, yb=None, res=None, gamma=None, beta=None, kv=None, max_len=1, state=None,
            ids=None, eos=-1, pad=0, kchunk=0, ld_yf=None):
    lib = _cabi.lib()
    M, K = x.shape
    N = w.shape[0]
    ws = torch.empty(lib.dmx_trocr_dec_linear_workspace_bytes(M, N, K), dtype=torch.uint8, device=DEV)
    _cabi.check(lib.dmx_trocr_dec_linear(epi, act, _ptr(x), M, K, _ptr(w), N, _ptr(bias), oscale, _ptr(yf), ld_yf or N, _ptr(yb),
                                         _ptr(res), _ptr(gamma), _ptr(beta), _ptr(kv), max_len, _ptr(state), _ptr(ids), eos, pad, kchunk,
                                         _ptr(ws), ws.numel(), _cabi.current_stream()), "trocr_dec_linear")
    torch.cuda.synchronize()


def _close(hip, ref, name, rel=1e-3, elem=None):
    """rel-L2 <= rel and every element within `elem` (default: 2e-3 of the largest |ref|)"""
    e = assert_close(hip, ref, rel, name)
    h, r = hip.detach().float().cpu(), ref.detach().float().cpu()
    bound = elem if elem is not None else 2e-3 * float(r.abs().max())
    worst = float((h - r).abs().max())
    assert worst <= bound, f"{name}: max |diff| {worst:.3e} > {bound:.3e}"
    return e


def _bf16_elem(ref):
    """per-element bound of a bf16-rounded output: one bf16 step of the value, plus fp32 summation noise"""
    return (ref.abs() * 2.0 ** -7 + 1e-5).cpu()


LIN_SHAPES = [(3072, 1024), (1024, 1024), (4096, 1024), (1024, 4096), (50265, 1024)]


@pytest.mark.parametrize("M", [1, 3, 8, 32, 64])
@pytest.mark.parametrize("N,K", LIN_SHAPES)
def test_dec_linear_epilogues(M, N, K):
    g = torch.Generator().manual_seed(M * 7 + N + K)
    x = (torch.randn(M, K, generator=g)).to(torch.bfloat16).to(DEV)
    w = (torch.randn(N, K, generator=g) * K ** -0.5).to(torch.bfloat16).to(DEV)
    bias = (torch.randn(N, generator=g) * 0.1).to(DEV)
    y0 = x.float() @ w.float().T                                   # fp32 torch on the same bf16 operands
    for kchunk in (0, K):                                          # the planned split-K, and one block per feature tile
        if N == 50265:
            if kchunk:
                continue
            # LM head: logits + greedy pick; constructed ties resolve to the lowest index
            w2 = w.clone()
            # rows equal to row 7: 23 (same block, another wave) and 60 (same block, another lane group) for the in-block merges,
            # 65, 40000 and N-1 (the ragged last tile) for the cross-block merge
            for j in (23, 60, 65, 40000, N - 1):
                w2[j] = w2[7]
            xs = x.clone()
            y = x.float() @ w2.float().T
            xs_ids = torch.zeros(M, 4, dtype=torch.int64, device=DEV)
            state = torch.zeros(256, dtype=torch.int32, device=DEV)
            logits = torch.empty(M, N, dtype=torch.float32, device=DEV)
            _linear(EPI_PICK, xs, w2, None, yf=logits, max_len=4, state=state, ids=xs_ids, eos=-1, pad=0)
            _close(logits, y, f"lm head M={M}")
            ref_tok = torch.argmax(logits, -1)                     # torch.argmax: lowest index among equal maxima
            assert torch.equal(xs_ids[:, 1].cpu(), ref_tok.cpu()), f"pick M={M}: {xs_ids[:, 1].tolist()} vs {ref_tok.tolist()}"
            assert torch.equal(state[16:16 + M].cpu(), ref_tok.int().cpu()) and int(state[0]) == 1
            # forced ties: a row whose maximum is shared by rows 7, 23, 60, 65, 40000 and N-1 picks 7
            xt = w2[7:8].repeat(M, 1).contiguous()
            ids_t = torch.zeros(M, 4, dtype=torch.int64, device=DEV)
            state.zero_()
            lt = torch.empty(M, N, dtype=torch.float32, device=DEV)
            _linear(EPI_PICK, xt, w2, None, yf=lt, max_len=4, state=state, ids=ids_t, eos=-1, pad=0)
            mx = lt.max(-1).values
            tie = (lt == mx[:, None]).sum(-1)
            assert bool((tie >= 6).all()), f"ties were not constructed: {tie.tolist()}"
            assert torch.equal(ids_t[:, 1].cpu(), torch.argmax(lt, -1).cpu()) and bool((ids_t[:, 1] == 7).all())
            # finished rows emit pad; a row that emits eos finishes
            state.zero_(); state[80] = 1                           # row 0 finished already
            ids_f = torch.zeros(M, 4, dtype=torch.int64, device=DEV)
            _linear(EPI_PICK, xt, w2, None, max_len=4, state=state, ids=ids_f, eos=7, pad=1)
            assert int(ids_f[0, 1]) == 1 and bool((ids_f[1:, 1] == 7).all()) and bool((state[80:80 + M] == 1).all())
            assert int(state[1]) == 1 and int(state[2]) == 2, "all rows finished at length 2"
            continue
        # bias (+ scale), both outputs
        yf = torch.empty(M, N, dtype=torch.float32, device=DEV); yb = torch.empty(M, N, dtype=torch.bfloat16, device=DEV)
        _linear(EPI_STORE, x, w, bias, oscale=0.5, yf=yf, yb=yb, kchunk=kchunk)
        ref = (y0 + bias) * 0.5
        _close(yf, ref, f"bias M={M} N={N} K={K} kchunk={kchunk}")
        assert bool(((yb.float() - ref).abs().cpu() <= _bf16_elem(ref)).all()), "bf16 output beyond one rounding step"
        for act, fn in ((1, torch.nn.functional.gelu), (2, torch.relu)):
            yb = torch.empty(M, N, dtype=torch.bfloat16, device=DEV)
            _linear(EPI_STORE, x, w, bias, act=act, yb=yb, kchunk=kchunk)
            ref = fn(y0 + bias)
            assert_close(yb, ref, 4e-3, f"act {act} M={M} N={N}")
            assert bool(((yb.float() - ref).abs().cpu() <= _bf16_elem(ref) + 1e-6).all()), f"act {act}: element beyond one bf16 step"
        if N == 3072:                                              # q | k | v: q scaled to yf, k | v into the cache row `pos`
            Dm = N // 3
            max_len, pos = 6, 4
            kv = torch.zeros(M, max_len, 2 * Dm, dtype=torch.bfloat16, device=DEV)
            q = torch.empty(M, Dm, dtype=torch.float32, device=DEV)
            state = torch.zeros(256, dtype=torch.int32, device=DEV); state[0] = pos
            _linear(EPI_QKV, x, w, bias, oscale=0.125, yf=q, kv=kv, max_len=max_len, state=state, kchunk=kchunk)
            ref = y0 + bias
            _close(q, ref[:, :Dm] * 0.125, f"qkv q M={M}")
            kvr = ref[:, Dm:]
            assert bool(((kv[:, pos].float() - kvr).abs().cpu() <= _bf16_elem(kvr)).all()), "k|v cache row"
            assert bool((kv[:, :pos] == 0).all()) and bool((kv[:, pos + 1:] == 0).all()), "k|v written outside row pos"
        if N == 1024:                                              # + residual, LayerNorm (eps 1e-5)
            res = torch.randn(M, N, generator=g).to(DEV)
            gamma = (1 + 0.1 * torch.randn(N, generator=g)).to(DEV); beta = (0.1 * torch.randn(N, generator=g)).to(DEV)
            yf = res.clone(); yb = torch.empty(M, N, dtype=torch.bfloat16, device=DEV)
            _linear(EPI_LN, x, w, bias, yf=yf, yb=yb, res=yf, gamma=gamma, beta=beta, kchunk=kchunk)   # in place, as the decoder runs it
            ref = torch.nn.functional.layer_norm(y0 + bias + res, (N,), gamma, beta, 1e-5)
            _close(yf, ref, f"ln M={M} K={K}", elem=2e-3 * float(ref.abs().max()))
            assert bool(((yb.float() - ref).abs().cpu() <= _bf16_elem(ref) + 1e-4).all())


@pytest.mark.parametrize("L", [1, 7, 64, 511, 577])
@pytest.mark.parametrize("M", [1, 5])
def test_dec_attention(L, M):
    lib = _cabi.lib()
    H, Dm = 16, 1024
    g = torch.Generator().manual_seed(L * 13 + M)
    q = (torch.randn(M, Dm, generator=g) * 0.125).to(DEV)
    kv = (torch.randn(M, L + 3, 2 * Dm, generator=g)).to(torch.bfloat16).to(DEV)   # (3 spare rows: never read)
    out = torch.empty(M, Dm, dtype=torch.bfloat16, device=DEV)
    ws = torch.empty(lib.dmx_trocr_dec_attn_workspace_bytes(M, H, L), dtype=torch.uint8, device=DEV)
    _cabi.check(lib.dmx_trocr_dec_attn(_ptr(q), M, H, _ptr(kv), (L + 3) * 2 * Dm, 2 * Dm, L, _ptr(out), _ptr(ws), ws.numel(),
                                       _cabi.current_stream()), "trocr_dec_attn")
    torch.cuda.synchronize()
    k = kv[:, :L, :Dm].float().view(M, L, H, 64).transpose(1, 2)
    v = kv[:, :L, Dm:].float().view(M, L, H, 64).transpose(1, 2)
    p = torch.softmax(q.view(M, H, 1, 64) @ k.transpose(-1, -2), -1)
    ref = (p @ v).view(M, H * 64)
    assert_close(out, ref, 4e-3, f"attn L={L}")
    assert bool(((out.float() - ref).abs().cpu() <= _bf16_elem(ref) + 1e-4).all()), f"attn L={L}: element beyond one bf16 step"


def _fixture(name):
    z = np.load(GOLDEN)
    pre = name + "/"
    cfg = ast.literal_eval(str(z[pre + "config"]))
    meta = ast.literal_eval(str(z["meta"]))
    return cfg, meta, {k[len(pre):]: torch.from_numpy(z[k]) for k in z.files if k.startswith(pre) and k != pre + "config"}


def _tiny(cfg, meta):
    return D.TrOCRForCausalLM(seed=meta["seed"], device=DEV, decoder_start_token_id=meta["start"], pad_token_id=meta["pad"], **cfg)


@pytest.mark.parametrize("name", ["tied_gelu", "untied_relu_scaled"])
def test_tiny_decoder_vs_transformers_fixture(name):
    cfg, meta, f = _fixture(name)
    m = _tiny(cfg, meta)
    enc = f["enc"].to(DEV)
    lg = m(f["tf_ids"].to(DEV), enc).logits
    ref = f["tf_logits"]
    err_abs = float((lg.cpu() - ref).abs().max())
    e = rel_l2(lg, ref)
    print(f"{name}: teacher-forced logits rel-L2 {e:.3e}, max |diff| {err_abs:.3e}")
    assert e <= TINY_TF_REL and err_abs <= TINY_TF_ABS, f"{name}: rel-L2 {e:.3e} / max |diff| {err_abs:.3e}"
    # the greedy path must be decided by margins wider than twice the measured logit error, or the fixture is unfit
    ids_ref = f["ids"]
    live = torch.ones_like(f["margins"], dtype=torch.bool)
    eos = int(f["eos"])
    if eos >= 0:                                                   # steps after a row finished emit pad whatever the logits say
        for b in range(ids_ref.shape[0]):
            hit = (ids_ref[b, 1:] == eos).nonzero()
            if len(hit):
                live[b, int(hit[0]) + 1:] = False
    assert float(f["margins"][live].min()) > 2 * err_abs, "fixture margin does not exceed twice the measured logit error"
    ids, _ = m.greedy(enc, meta["max_length"], meta["start"], None if eos < 0 else eos, meta["pad"])
    assert torch.equal(ids.cpu(), ids_ref), f"{name}: {ids.tolist()} vs transformers {ids_ref.tolist()}"


def _full_params(m):
    return {k: v.detach().float().cpu() for k, v in m.named_parameters()}


@pytest.fixture(scope="module")
def full():
    m = D.TrOCRForCausalLM(device=DEV)
    enc = (torch.randn(4, 577, 1024, generator=torch.Generator().manual_seed(31))).to(DEV)
    return m, enc


def test_full_size_decoder_vs_restatement(full):
    m, enc = full
    cfg = dict(D.TROCR_LARGE_DECODER_CONFIG)
    assert m.launches_per_step <= 2 + 8 * cfg["decoder_layers"]
    ids, lg = m.greedy(enc, 25, 2, None, 1, keep_logits=True)
    assert ids.shape == (4, 25)
    P = _full_params(m)
    ref = R.forward(P, cfg, ids[:, :-1].cpu(), enc.cpu())       # teacher-forced on the GPU's own path
    e = rel_l2(lg, ref)
    err = float((lg.cpu() - ref).abs().max())
    print(f"full size: logits rel-L2 {e:.3e}, max |diff| {err:.3e}")
    assert e <= FULL_REL, f"full-size logits rel-L2 {e:.3e}"
    mg = R.margins(ref)
    decided = mg > 2 * err
    pick = torch.argmax(ref, -1)
    assert torch.equal(ids[:, 1:].cpu()[decided], pick[decided]), "greedy id differs where the margin decides it"
    assert float(decided.float().mean()) > 0.5, "too few steps decided by the margin rule to check anything"


def test_bit_reproducible(full):
    m, enc = full
    a_ids, a_lg = m.greedy(enc[:2], 9, 2, None, 1, keep_logits=True)
    b_ids, b_lg = m.greedy(enc[:2], 9, 2, None, 1, keep_logits=True)
    c_ids, c_lg = m.greedy(enc[:2], 9, 2, None, 1, keep_logits=True, use_graph=False)
    assert torch.equal(a_ids, b_ids) and torch.equal(a_ids, c_ids)
    assert torch.equal(a_lg.view(torch.int32), b_lg.view(torch.int32)), "two graph-replayed generate calls differ in logit bits"
    assert torch.equal(a_lg.view(torch.int32), c_lg.view(torch.int32)), "graph replay and the uncaptured run differ in logit bits"


def test_vision_encoder_decoder_generate():
    """generate(pixel_values) = the HIP encoder's states -> the CPU restatement's greedy search, on pixel inputs (seed scan) whose
    greedy path is decided at every step by a margin wider than twice the measured logit error"""
    _, meta, _ = _fixture("tied_gelu")
    cfg, _, _ = _fixture("untied_relu_scaled")
    enc_cfg = dict(image_size=64, patch_size=16, num_channels=3, hidden_size=256, num_hidden_layers=2, num_attention_heads=4,
                   intermediate_size=512, qkv_bias=True)
    model = D.VisionEncoderDecoderModel(D.TrOCREncoder(device=DEV, **enc_cfg), _tiny(cfg, meta),
                                        dict(decoder_start_token_id=meta["start"], pad_token_id=meta["pad"], eos_token_id=None, max_length=8))
    P = _full_params(model.decoder)
    chosen = None
    for seed in range(40):
        px = torch.randn(2, 3, 64, 64, generator=torch.Generator().manual_seed(seed)).to(DEV)
        enc = model.encoder(px).last_hidden_state
        ref_ids, ref_lg = R.generate(P, cfg, enc.cpu(), 8, meta["start"], None, meta["pad"])
        _, lg = model.decoder.greedy(enc, 8, meta["start"], None, meta["pad"], keep_logits=True)
        err = float((lg.cpu() - ref_lg).abs().max())
        if float(R.margins(ref_lg).min()) > 2 * err:
            chosen = (px, enc, ref_ids)
            break
    assert chosen is not None, "no pixel input among 40 seeds whose greedy margins exceed twice the logit error"
    px, enc, ref_ids = chosen
    ids = model.generate(px)
    assert ids.dtype == torch.int64 and ids.device.type == "cuda" and ids.shape == (2, 8)
    assert torch.equal(ids.cpu(), ref_ids), f"{ids.tolist()} vs restatement {ref_ids.tolist()}"
    assert torch.equal(model.generate(encoder_hidden_states=enc), ids)


def test_generate_stops_early_on_the_device():
    """a batch whose rows have all emitted eos stops: the returned length is the device's stop length, and the host enqueued at
    most 2 * POLL_EVERY steps past it"""
    from diffute_amd import ocr
    cfg, meta, f = _fixture("untied_relu_scaled")
    m = _tiny(cfg, meta)
    enc = f["enc"][:1].to(DEV)
    ids_full, _ = m.greedy(enc, 40, meta["start"], None, meta["pad"])
    eos = int(ids_full[0, 3])                                    # the token emitted at step 3
    stop = int((ids_full[0, 1:] == eos).nonzero()[0]) + 2        # length including the start token
    ids, _ = m.greedy(enc, 40, meta["start"], eos, meta["pad"])
    assert torch.equal(ids, ids_full[:, :stop])
    steps_run = int(m._runs[(1, enc.shape[1], 40)]["cache"][:4].view(torch.int32)[0])
    assert steps_run <= stop - 1 + 2 * ocr.POLL_EVERY, f"{steps_run} steps ran for a sequence that stopped at length {stop}"


def test_decode_loop_graph_and_eager_agree_and_graphs_are_cached_per_key():
    """what greedy and beam search share in the decode loop: the captured step graph and the uncaptured step give the same ids
    (and beam scores) on a batch where one row finishes early and another never does, and a run keeps one graph per key - a
    second eos id captures a second graph and leaves the first alone"""
    cfg, meta, _ = _fixture("tied_gelu")
    m = _tiny(cfg, meta)
    B, S, L, start, pad = 3, 5, 12, meta["start"], meta["pad"]
    enc = torch.randn(B, S, cfg["d_model"], generator=torch.Generator().manual_seed(3))
    # the eos id comes from the CPU restatement's free-running greedy path on the same weights: the first token of row 0
    free, free_lg = R.generate(_full_params(m), cfg, enc, L, start, None, pad)
    eos, eos2 = int(free[0, 1]), int(free[1, 1])
    early = (free[:, 1:-1] == eos).any(1)
    assert bool(early.any()) and not bool((free[:, 1:] == eos).any(1).all()) and eos2 != eos, f"unfit inputs: {free.tolist()}"
    # the GPU takes the same path: every pick on it is decided by more than four times the 2.3e-2 logit error measured above
    assert float(R.margins(free_lg).min()) > 4 * 2.3e-2
    enc = enc.to(DEV)
    ids_g, _ = m.greedy(enc, L, start, eos, pad, use_graph=True)
    ids_e, _ = m.greedy(enc, L, start, eos, pad, use_graph=False)
    assert torch.equal(ids_g, ids_e), f"greedy: graph {ids_g.tolist()} vs uncaptured {ids_e.tolist()}"
    hit = (ids_g[:, 1:-1] == eos).any(1).cpu()
    assert ids_g.shape == (B, L) and bool(hit.any()) and not bool(hit.all()), f"one row should stop early, one not: {ids_g.tolist()}"
    beam_g = m.beam_search(enc, L, start, eos, pad, num_beams=2, use_graph=True)
    beam_e = m.beam_search(enc, L, start, eos, pad, num_beams=2, use_graph=False)
    assert torch.equal(beam_g[0], beam_e[0]) and torch.equal(beam_g[1].view(torch.int32), beam_e[1].view(torch.int32)), "beam: graph vs uncaptured"
    for key, again in (((B, S, L), lambda: m.greedy(enc, L, start, eos2, pad)),
                       (("beam", B, 2, S, L), lambda: m.beam_search(enc, L, start, eos2, pad, num_beams=2))):
        graphs = m._runs[key]["graphs"]
        assert len(graphs) == 1, f"{key}: {list(graphs)}"
        (k0, g0), = graphs.items()
        again()
        assert m._runs[key]["graphs"] is graphs and len(graphs) == 2 and graphs[k0] is g0, f"{key}: {list(graphs)}"
