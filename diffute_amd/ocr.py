"""OCR read-back: TrOCR's text decoder and the encoder-decoder wrapper the reference loads as `full_trocr_model`.

app.ipynb:547-548 builds two models from `trocr-large-printed`: `.encoder` (the glyph encoder, `TrOCREncoder`) and the full
`VisionEncoderDecoderModel`, whose `generate(pixel_values)` reads an edited box back as token ids (app.ipynb:842-847; the
tokenizer's `batch_decode` stays with the caller).  `from diffute_amd import VisionEncoderDecoderModel` serves both.
Greedy generation follows transformers' `generate(num_beams=1, do_sample=False)`; every FLOP runs in the gfx950 library.
The host side of the decoder is shared: `_cached_run` keys the buffers of a run, `_decode_loop` drives greedy and beam search alike
(step graph, replay, the device's all-finished flag), `_check_enc_shape` checks encoder states for every entry.
"""
import ctypes
import json
import os

import torch
from torch import nn

from . import _cabi
from .models import TROCR_LARGE_VIT_CONFIG, TrOCREncoder, _Config, _HipModel, load_weights_file

# transformers' TrOCRConfig defaults = the trocr-large decoder
TROCR_LARGE_DECODER_CONFIG = dict(
    vocab_size=50265, d_model=1024, decoder_layers=12, decoder_attention_heads=16, decoder_ffn_dim=4096, activation_function="gelu",
    max_position_embeddings=512, scale_embedding=False, use_learned_position_embeddings=True, layernorm_embedding=True,
    tie_word_embeddings=True, cross_attention_hidden_size=None, decoder_start_token_id=2, eos_token_id=2, pad_token_id=1, bos_token_id=0)

# generation settings whose non-default values select search / processing this library does not implement
_GEN_UNSUPPORTED = dict(num_beams=1, do_sample=False, num_beam_groups=1, no_repeat_ngram_size=0, length_penalty=1.0, min_length=0,
                        min_new_tokens=None, forced_bos_token_id=None, forced_eos_token_id=None, repetition_penalty=1.0,
                        early_stopping=False, penalty_alpha=None, num_return_sequences=1, temperature=1.0, top_k=50, top_p=1.0,
                        bad_words_ids=None, suppress_tokens=None, begin_suppress_tokens=None, encoder_no_repeat_ngram_size=0)

# settings that only beam search reads: inert when greedy search runs (num_beams == 1)
_BEAM_ONLY = ("early_stopping", "length_penalty", "num_beam_groups")

# the settings beam_search() implements itself (every other non-default entry of _GEN_UNSUPPORTED stays refused there too)
_BEAM_SEARCH_OWN = ("num_beams", "length_penalty", "early_stopping", "num_return_sequences")

POLL_EVERY = 4          # a decode loop reads the device's all-finished flag (copied asynchronously) every POLL_EVERY steps


def _eos_pad(eos_token_id, pad_token_id):
    """the (eos, pad) ids a step takes: no eos = -1, pad defaults to eos, and to 0 without either"""
    eos = -1 if eos_token_id is None else int(eos_token_id)
    pad = eos if pad_token_id is None else int(pad_token_id)
    return eos, max(pad, 0)


def _state_words(r):
    """int32 view of a run's state words (include/diffute_hip.h DMX_TROCR_STATE_*) up to the finished flags"""
    return r["cache"][:4 * _cabi.STATE_FINISHED].view(torch.int32)


class CausalLMOutput:
    def __init__(self, logits):
        self.logits = logits


class ScoreOutput:
    """what `score()` returns: per-token log-probs of the labels under teacher forcing, their sums and the batch loss"""

    def __init__(self, token_logprobs, sequence_logprobs, num_tokens, predictions, loss, logits=None):
        self.token_logprobs, self.sequence_logprobs, self.num_tokens = token_logprobs, sequence_logprobs, num_tokens
        self.predictions, self.loss, self.logits = predictions, loss, logits


class BaseModelOutput:
    def __init__(self, last_hidden_state=None):
        self.last_hidden_state = last_hidden_state

    def __getitem__(self, i):
        return (self.last_hidden_state,)[i]


class Seq2SeqLMOutput:
    def __init__(self, loss=None, logits=None, encoder_last_hidden_state=None):
        self.loss, self.logits, self.encoder_last_hidden_state = loss, logits, encoder_last_hidden_state

    def to_tuple(self):
        return tuple(v for v in (self.loss, self.logits, self.encoder_last_hidden_state) if v is not None)

    def __getitem__(self, i):
        return self.to_tuple()[i]


MAX_SCORE_ROWS = 4096   # B * T rows of one score() call (include/diffute_hip.h dmx_trocr_dec_score)


class TrOCRForCausalLM(_HipModel):
    """TrOCR's text decoder (transformers `TrOCRForCausalLM`; the `.decoder` of app.ipynb:548's `full_trocr_model`).  Parameters
    carry transformers' state-dict keys; `output_projection.weight` exists only when the config unties it from `embed_tokens`.
    Forward-only."""
    _kind = "trocr_dec"

    def __init__(self, seed=555, device="cpu", **config):
        super().__init__()
        cfg = dict(TROCR_LARGE_DECODER_CONFIG)
        cfg.update({k: v for k, v in config.items() if k in TROCR_LARGE_DECODER_CONFIG})
        if not cfg["use_learned_position_embeddings"]:
            raise NotImplementedError("TrOCRForCausalLM: sinusoidal position embeddings are not implemented (use_learned_position_embeddings=False)")
        if cfg["activation_function"] not in ("gelu", "relu"):
            raise NotImplementedError(f"TrOCRForCausalLM: activation_function={cfg['activation_function']!r} is not implemented (gelu, relu)")
        if cfg["max_position_embeddings"] > 512:
            raise NotImplementedError("TrOCRForCausalLM: more than 512 positions are not implemented")
        self.config = _Config(**cfg)
        c = _cabi.TrOCRDecConfig()
        c.vocab_size = cfg["vocab_size"]; c.d_model = cfg["d_model"]; c.num_layers = cfg["decoder_layers"]
        c.num_heads = cfg["decoder_attention_heads"]; c.ffn_dim = cfg["decoder_ffn_dim"]; c.max_position_embeddings = cfg["max_position_embeddings"]
        c.cross_hidden_size = int(cfg["cross_attention_hidden_size"] or 0)
        c.activation = 1 if cfg["activation_function"] == "relu" else 0
        c.scale_embedding = int(bool(cfg["scale_embedding"])); c.layernorm_embedding = int(bool(cfg["layernorm_embedding"]))
        c.tie_word_embeddings = int(bool(cfg["tie_word_embeddings"]))
        self._cstruct = c
        h = self._create_handle("bf16")
        self._setup(h, seed, device)
        self.requires_grad_(False)
        self._runs, self._runs_epoch = {}, self._epoch

    def _switch_build(self, elem):
        if elem != "bf16":
            raise NotImplementedError("TrOCRForCausalLM: the decoder runs on the bf16 build")

    @property
    def launches_per_step(self):
        return int(self._lib.dmx_trocr_dec_launches_per_step(self._h))

    def _cached_run(self, key, make):
        """the buffers of one run, made once per key and set of weights"""
        if self._runs_epoch != self._epoch:      # runs (and their captured graphs) of earlier weights
            self._runs, self._runs_epoch = {}, self._epoch
        r = self._runs.get(key)
        if r is None:
            r = self._runs[key] = make()
        return r

    # ---- buffers of one (B, S, max_len): cache (state words, self / cross K/V), workspace, output ids, optional logits row
    def _run(self, B, S, max_len):
        def make():
            lib, dev = self._lib, self.device
            return dict(cache=torch.empty(lib.dmx_trocr_dec_cache_bytes(self._h, B, S, max_len), dtype=torch.uint8, device=dev),
                        ws=torch.empty(lib.dmx_trocr_dec_workspace_bytes(self._h, B, S, max_len), dtype=torch.uint8, device=dev),
                        ids=torch.zeros(B, max_len, dtype=torch.int64, device=dev),
                        logits=torch.empty(B, self.config.vocab_size, dtype=torch.float32, device=dev), graphs={})
        return self._cached_run((B, S, max_len), make)

    def _begin(self, r, enc, max_len, start):
        lib = self._lib
        B, S = enc.shape[0], enc.shape[1]
        st = _cabi.current_stream()
        _cabi.check(lib.dmx_trocr_dec_cross_kv(self._h, _cabi.ptr(enc), B, S, max_len, _cabi.ptr(r["cache"]), _cabi.ptr(r["ws"]),
                                               r["ws"].numel(), st), "trocr_dec_cross_kv")
        _cabi.check(lib.dmx_trocr_dec_reset(self._h, _cabi.ptr(r["cache"]), B, S, max_len, int(start), _cabi.ptr(r["ids"]), st), "trocr_dec_reset")

    def _step(self, r, B, S, max_len, eos, pad, logits, ld):
        _cabi.check(self._lib.dmx_trocr_dec_step(self._h, _cabi.ptr(r["cache"]), B, S, max_len, int(eos), int(pad), _cabi.ptr(r["ids"]),
                                                 None if logits is None else ctypes.c_void_p(logits), ld, _cabi.ptr(r["ws"]),
                                                 r["ws"].numel(), _cabi.current_stream()), "trocr_dec_step")

    def _check_enc_shape(self, enc_shape, rows_per_item=1):
        """encoder states (a tensor or its shape) must be [B, S, kdim] with B * rows_per_item of the decoder's 64 rows"""
        shape = tuple(getattr(enc_shape, "shape", enc_shape))
        kdim = self.config.cross_attention_hidden_size or self.config.d_model
        if len(shape) != 3 or shape[2] != kdim:
            raise ValueError(f"encoder_hidden_states must be [B, S, {kdim}], got {shape}")
        if not 1 <= shape[0] or shape[0] * rows_per_item > 64:
            raise ValueError(f"TrOCRForCausalLM: 1 <= batch <= 64 rows, got {shape[0]}" if rows_per_item == 1 else
                             f"beam_search: batch * num_beams = {shape[0]} * {rows_per_item} exceeds the decoder's 64 rows")
        return shape

    def _check_inputs(self, enc):
        if torch.is_grad_enabled() and any(p.requires_grad for p in self.parameters()):
            raise NotImplementedError("diffute_amd: the OCR decoder is forward-only")
        _cabi.require_cuda(enc)
        self._check_enc_shape(enc)
        self._ensure_packed()
        return enc.to(torch.float32).contiguous()

    @torch.no_grad()
    def forward(self, input_ids, encoder_hidden_states, return_dict=True, **unused):
        """teacher-forced logits [B, T, V] (fp32) of input_ids [B, T]: the decode step run T times over the KV cache"""
        enc = self._check_inputs(encoder_hidden_states)
        ids = input_ids.to(device=enc.device, dtype=torch.int64).contiguous()
        B, T = ids.shape
        if ids.shape[0] != enc.shape[0] or not 1 <= T <= self.config.max_position_embeddings:
            raise ValueError(f"input_ids must be [B, T] with B = {enc.shape[0]} and 1 <= T <= {self.config.max_position_embeddings}")
        V = self.config.vocab_size
        r = self._run(B, enc.shape[1], T)
        out = torch.empty(B, T, V, dtype=torch.float32, device=enc.device)
        self._begin(r, enc, T, 0)
        lib, st = self._lib, _cabi.current_stream()
        for t in range(T):
            col = ids[:, t].contiguous()
            _cabi.check(lib.dmx_trocr_dec_set_tokens(self._h, _cabi.ptr(r["cache"]), _cabi.ptr(col), B, st), "trocr_dec_set_tokens")
            self._step(r, B, enc.shape[1], T, -1, 0, out.data_ptr() + t * V * 4, T * V)
        return CausalLMOutput(out) if return_dict else (out,)

    def _check_score_args(self, enc_shape, labels, decoder_input_ids, ignore_index):
        """every shape / dtype / range check of score(), on the host side: nothing is launched before it passes"""
        B = self._check_enc_shape(enc_shape)[0]
        if enc_shape[1] < 1:
            raise ValueError("encoder_hidden_states has no rows")
        if labels is None and decoder_input_ids is None:
            raise ValueError("score: pass labels or decoder_input_ids")
        V, P = self.config.vocab_size, self.config.max_position_embeddings
        shape = None
        for name, t in (("labels", labels), ("decoder_input_ids", decoder_input_ids)):
            if t is None:
                continue
            if not torch.is_tensor(t) or t.dtype != torch.int64:
                raise ValueError(f"score: {name} must be an int64 tensor, got {getattr(t, 'dtype', type(t))}")
            if t.ndim != 2 or t.shape[0] != B:
                raise ValueError(f"score: {name} must be [B, T] with B = {B}, got {tuple(t.shape)}")
            if shape is not None and tuple(t.shape) != shape:
                raise ValueError(f"score: labels {shape} and decoder_input_ids {tuple(t.shape)} differ in shape")
            shape = tuple(t.shape)
        T = shape[1]
        if not 1 <= T <= P:
            raise ValueError(f"score: 1 <= T <= {P} positions, got T = {T}")
        if B * T > MAX_SCORE_ROWS:
            raise ValueError(f"score: B * T = {B} * {T} exceeds {MAX_SCORE_ROWS} rows")
        if not -2 ** 31 <= int(ignore_index) < 2 ** 31:
            raise ValueError(f"score: ignore_index {ignore_index} is not a 32-bit integer")
        if labels is not None:
            bad = ((labels < 0) | (labels >= V)) & (labels != int(ignore_index))
            if bool(bad.any()):
                raise ValueError(f"score: labels must lie in [0, {V}) or equal ignore_index = {ignore_index}")
        if decoder_input_ids is not None and bool(((decoder_input_ids < 0) | (decoder_input_ids >= V)).any()):
            raise ValueError(f"score: decoder_input_ids must lie in [0, {V})")
        return B, T

    @torch.no_grad()
    def score(self, labels, encoder_hidden_states, *, decoder_start_token_id=None, pad_token_id=None, ignore_index=-100,
              decoder_input_ids=None, return_logits=False):
        """Teacher-forced pass over known target ids in ONE prefill (transformers' `model(encoder_outputs=..., labels=...)`): the
        decoder inputs are the labels shifted right (start token first, ignore_index -> pad), or decoder_input_ids as they are.
        Returns a ScoreOutput: token_logprobs [B, T] fp32 (0 where the label is ignore_index), sequence_logprobs [B], num_tokens
        [B], predictions [B, T] int64 (the teacher-forced arg-max), loss = -sum(token_logprobs) / sum(num_tokens) (torch's
        CrossEntropyLoss over the flattened batch; NaN when every label is ignored) and logits [B, T, V] fp32 only with
        return_logits.  With labels=None (decoder_input_ids given) only predictions and logits are computed."""
        B, T = self._check_score_args(tuple(encoder_hidden_states.shape), labels, decoder_input_ids, ignore_index)
        start = self.config.decoder_start_token_id if decoder_start_token_id is None else decoder_start_token_id
        pad = self.config.pad_token_id if pad_token_id is None else pad_token_id
        if decoder_input_ids is None and (start is None or pad is None):
            raise ValueError("score: decoder_start_token_id and pad_token_id are needed to shift the labels")
        enc = self._check_inputs(encoder_hidden_states)
        dev, S, V = enc.device, enc.shape[1], self.config.vocab_size
        lab = None if labels is None else labels.to(dev).contiguous()
        dids = None if decoder_input_ids is None else decoder_input_ids.to(dev).contiguous()
        r = self._cached_run(("score", B, S, T), lambda: dict(
            ws=torch.empty(self._lib.dmx_trocr_dec_prefill_workspace_bytes(self._h, B, S, T), dtype=torch.uint8, device=dev)))
        logp = None if lab is None else torch.empty(B, T, dtype=torch.float32, device=dev)
        amax = torch.empty(B, T, dtype=torch.int32, device=dev)
        logits = torch.empty(B, T, V, dtype=torch.float32, device=dev) if return_logits else None
        _cabi.check(self._lib.dmx_trocr_dec_score(self._h, _cabi.ptr(enc), B, S, _cabi.ptr(lab), _cabi.ptr(dids), T, int(start or 0), int(pad or 0),
                                                  int(ignore_index), _cabi.ptr(logp), _cabi.ptr(amax), _cabi.ptr(logits), V, _cabi.ptr(r["ws"]),
                                                  r["ws"].numel(), _cabi.current_stream()), "trocr_dec_score")
        if lab is None:
            return ScoreOutput(None, None, None, amax.long(), None, logits)
        n = (lab != int(ignore_index)).sum(1)
        seq = logp.sum(1)
        return ScoreOutput(logp, seq, n, amax.long(), -logp.sum() / n.sum(), logits)

    def _decode_loop(self, r, gkey, step, n_steps, use_graph, after_step=None, finish=None):
        """Enqueue up to n_steps calls of `step()` on the run r, as replays of one graph captured under r["graphs"][gkey] with
        use_graph; after_step(i) follows step i = 1, 2, ... and finish() the last one.  Returns (steps enqueued, done, stop_len):
        the device's all-finished flag and stop length, read once after everything enqueued has run."""
        if use_graph and gkey not in r["graphs"]:
            # one linear chain of kernels, captured on a side stream; the tokens, the position, the scores and the counters live in
            # device memory, so the same graph replays every step
            main, side = torch.cuda.current_stream(), torch.cuda.Stream(device=r["cache"].device)
            side.wait_stream(main)
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g, stream=side, capture_error_mode="thread_local"):
                step()
            main.wait_stream(side)
            r["graphs"][gkey] = g
        run = r["graphs"][gkey].replay if use_graph else step
        flags = _state_words(r)[_cabi.STATE_DONE:_cabi.STATE_STOP_LEN + 1]
        # every POLL_EVERY steps the all-finished flag is copied to pinned memory behind an event; before more steps are enqueued
        # the host waits for the copy of POLL_EVERY steps back, so at most 2 * POLL_EVERY steps are in flight and a batch that
        # has finished stops within that many steps instead of running to max_length
        polls, steps = [], 0
        while steps < n_steps:
            run()
            steps += 1
            if after_step is not None:
                after_step(steps)
            if steps % POLL_EVERY == 0 and steps < n_steps:
                f = torch.empty(2, dtype=torch.int32, pin_memory=True)
                f.copy_(flags, non_blocking=True)
                ev = torch.cuda.Event(); ev.record()
                polls.append((ev, f))
                if len(polls) > 1:
                    ev0, f0 = polls.pop(0)
                    ev0.synchronize()
                    if int(f0[0]):
                        break
        if finish is not None:
            finish()
        flag = torch.empty(2, dtype=torch.int32)
        flag.copy_(flags)                        # (the one synchronisation at the end)
        return steps, int(flag[0]), int(flag[1])

    @torch.no_grad()
    def greedy(self, encoder_hidden_states, max_length, decoder_start_token_id, eos_token_id, pad_token_id, use_graph=True, keep_logits=False):
        """greedy ids [B, L] (L <= max_length, counting the start token), as transformers' greedy search; with keep_logits also the
        fp32 logits [B, L - 1, V] of every step"""
        enc = self._check_inputs(encoder_hidden_states)
        B, S = enc.shape[0], enc.shape[1]
        if not 1 <= max_length <= self.config.max_position_embeddings:
            raise ValueError(f"max_length={max_length}: the decoder has {self.config.max_position_embeddings} positions")
        eos, pad = _eos_pad(eos_token_id, pad_token_id)
        r = self._run(B, S, max_length)
        self._begin(r, enc, max_length, decoder_start_token_id)
        if max_length == 1:
            return r["ids"][:, :1].clone(), None
        lg = r["logits"] if keep_logits else None
        lg_ptr, kept = (None if lg is None else lg.data_ptr()), []
        steps, done, stop_len = self._decode_loop(
            r, (eos, pad, keep_logits), lambda: self._step(r, B, S, max_length, eos, pad, lg_ptr, self.config.vocab_size), max_length - 1,
            use_graph, after_step=(lambda i: kept.append(lg.clone())) if keep_logits else None)
        L = stop_len if done else steps + 1
        ids = r["ids"][:, :L].clone()
        return ids, (torch.stack(kept[:L - 1], 1) if keep_logits else None)

    # ---- beam search: rows = items x beams; the cache adds a beam state block (include/diffute_hip.h DMX_TROCR_BEAM_*)
    @property
    def beam_launches_per_step(self):
        return int(self._lib.dmx_trocr_dec_beam_launches_per_step(self._h))

    def _check_beam_args(self, enc_shape, max_length, num_beams, length_penalty, early_stopping, num_return_sequences):
        if isinstance(num_beams, bool) or not isinstance(num_beams, int) or not 2 <= num_beams <= 16:
            raise ValueError(f"beam_search: num_beams must be an integer in 2 ... 16, got {num_beams!r}")
        self._check_enc_shape(enc_shape, num_beams)
        if not 1 <= int(num_return_sequences) <= num_beams:
            raise ValueError(f"beam_search: num_return_sequences={num_return_sequences} must be in 1 ... num_beams")
        if self.config.vocab_size < 2 * num_beams:
            raise ValueError(f"beam_search: vocab_size {self.config.vocab_size} < 2 * num_beams")
        if not (early_stopping is True or early_stopping is False or early_stopping == "never"):
            raise ValueError(f"beam_search: early_stopping must be False, True or 'never', got {early_stopping!r}")
        if not 1 <= max_length <= self.config.max_position_embeddings:
            raise ValueError(f"max_length={max_length}: the decoder has {self.config.max_position_embeddings} positions")
        float(length_penalty)

    def _beam_run(self, B, nb, S, max_len):
        def make():
            lib, dev, h = self._lib, self.device, self._h
            nbytes = lib.dmx_trocr_dec_beam_cache_bytes(h, B, nb, S, max_len)
            if not nbytes:
                raise NotImplementedError(f"beam_search: vocab_size {self.config.vocab_size} is too large for {nb} beams")
            off = lib.dmx_trocr_dec_beam_state_offset(h, B, nb, S, max_len)
            cache = torch.empty(nbytes, dtype=torch.uint8, device=dev)
            bstate = cache[off:off + lib.dmx_trocr_dec_beam_state_bytes(max_len)]
            W = _cabi.BEAM_WORDS
            return dict(cache=cache, ws=torch.empty(lib.dmx_trocr_dec_beam_workspace_bytes(h, B, nb, S, max_len), dtype=torch.uint8, device=dev),
                        words=bstate[:W * 4].view(torch.int32), fwords=bstate[:W * 4].view(torch.float32),
                        hist=bstate[W * 4:(W + 64 * max_len) * 4].view(torch.int32).view(max_len, 64),
                        table=bstate[(W + 128 * max_len) * 4:(W + 160 * max_len) * 4].view(2, 64, max_len),
                        logp=torch.empty(B * nb, self.config.vocab_size, dtype=torch.float32, device=dev), graphs={})
        return self._cached_run(("beam", B, nb, S, max_len), make)

    def _beam_step(self, r, B, nb, S, max_len, eos, lp, es, logp):
        _cabi.check(self._lib.dmx_trocr_dec_beam_step(self._h, _cabi.ptr(r["cache"]), B, nb, S, max_len, int(eos), float(lp), int(es),
                                                      None if logp is None else _cabi.ptr(logp), _cabi.ptr(r["ws"]), r["ws"].numel(),
                                                      _cabi.current_stream()), "trocr_dec_beam_step")

    @torch.no_grad()
    def beam_search(self, encoder_hidden_states, max_length, decoder_start_token_id, eos_token_id, pad_token_id, *, num_beams,
                    length_penalty=1.0, early_stopping=False, num_return_sequences=1, use_graph=True, keep_trace=False):
        """transformers' beam search (do_sample=False, no logits processors, one eos id or none): (sequences int64
        [B * num_return_sequences, L], sequences_scores fp32 [B * num_return_sequences], trace).  With keep_trace the trace
        lists, per executed step, the fp32 log-probs [B * num_beams, V] the selection used, the input tokens, the running
        scores before the step, the chosen (parent, token) of every row and every row's running sequence after it."""
        self._check_beam_args(encoder_hidden_states, max_length, num_beams, length_penalty, early_stopping, num_return_sequences)
        enc = self._check_inputs(encoder_hidden_states)
        B, S, nb, nret = enc.shape[0], enc.shape[1], num_beams, int(num_return_sequences)
        eos, pad = _eos_pad(eos_token_id, pad_token_id)
        if max_length == 1:
            return (torch.full((B * nret, 1), int(decoder_start_token_id), dtype=torch.int64, device=enc.device),
                    torch.full((B * nret,), -1.0e9, dtype=torch.float32, device=enc.device), [] if keep_trace else None)
        es = 2 if early_stopping == "never" else int(bool(early_stopping))
        lib, M = self._lib, B * nb
        r = self._beam_run(B, nb, S, max_length)
        _cabi.check(lib.dmx_trocr_dec_beam_begin(self._h, _cabi.ptr(enc), B, nb, S, max_length, int(decoder_start_token_id), _cabi.ptr(r["cache"]),
                                                 _cabi.ptr(r["ws"]), r["ws"].numel(), _cabi.current_stream()), "trocr_dec_beam_begin")
        logp = r["logp"] if keep_trace else None
        words, fwords, trace = r["words"], r["fwords"], []
        tokens = _state_words(r)[_cabi.STATE_TOKENS:_cabi.STATE_TOKENS + M]
        RUN, PAR = _cabi.BEAM_RUN_SCORE, _cabi.BEAM_PARENT
        # what a step starts from is what the step before left: the trace entry of step i takes its "before" values from here
        before = dict(input_tokens=tokens.clone(), running_scores=fwords[RUN:RUN + M].clone()) if keep_trace else None

        def record(steps):
            rows = torch.arange(M, device=enc.device)
            tab = r["table"][steps & 1, :M, :steps].long()                           # physical row of positions 0 .. steps - 1
            seq = torch.cat([r["hist"][torch.arange(steps, device=enc.device)[None, :], tab].long(), r["hist"][steps, :M].long()[:, None]], 1)
            trace.append(dict(before, logp=logp.clone(), parent=words[PAR:PAR + M].clone() - (rows // nb * nb).int(), token=tokens.clone(),
                              sequences=seq))
            before.update(input_tokens=trace[-1]["token"], running_scores=fwords[RUN:RUN + M].clone())

        seqs = torch.empty(B * nret, max_length, dtype=torch.int64, device=enc.device)
        scores = torch.empty(B * nret, dtype=torch.float32, device=enc.device)
        lens = torch.empty(B * nret, dtype=torch.int32, device=enc.device)

        def gather():
            _cabi.check(lib.dmx_trocr_dec_beam_finalize(self._h, _cabi.ptr(r["cache"]), B, nb, S, max_length, nret, pad, _cabi.ptr(seqs), _cabi.ptr(scores),
                                                        _cabi.ptr(lens), _cabi.current_stream()), "trocr_dec_beam_finalize")

        steps, done, stop_len = self._decode_loop(
            r, (eos, float(length_penalty), es, keep_trace), lambda: self._beam_step(r, B, nb, S, max_length, eos, length_penalty, es, logp),
            max_length - 1, use_graph, after_step=record if keep_trace else None, finish=gather)
        L = 1 + int(lens.max())
        if keep_trace:
            trace = trace[:stop_len - 1 if done else steps]      # steps the device executed before the loop condition ended it
        return seqs[:, :L].contiguous(), scores, (trace if keep_trace else None)


def _check_unsupported(who, settings, own, hint):
    """refuse every non-default entry of _GEN_UNSUPPORTED but the settings in `own` (what the caller implements itself, or what
    is inert in its search); hint(k) ends the message"""
    for k, want in _GEN_UNSUPPORTED.items():
        v = settings.get(k)
        if k in own or v is None or v == want:
            continue
        if k in ("temperature", "top_k", "top_p") and not settings.get("do_sample"):
            continue                              # sampling knobs are inert without sampling
        raise NotImplementedError(f"VisionEncoderDecoderModel.{who}: {k}={v!r} is not implemented{hint(k)}")


def _check_generation(settings, explicit_beams):
    """generate(): greedy search only.  An explicit num_beams=1 overrides the configuration's; beam-search knobs are inert under it"""
    greedy = explicit_beams or int(settings.get("num_beams") or 1) == 1
    own = ("num_beams", *_BEAM_ONLY) if explicit_beams else _BEAM_ONLY if greedy else ()
    _check_unsupported("generate", settings, own, lambda k: "; pass num_beams=1 to run greedy search anyway, or call beam_search()"
                       if k in ("num_beams", *_BEAM_ONLY) else " (greedy search only: remove it from the call / generation_config)")


class VisionEncoderDecoderModel(nn.Module):
    """`full_trocr_model` of app.ipynb:548: `.encoder` is the glyph encoder (`TrOCREncoder`, app.ipynb:547), `.decoder` the text
    decoder (`TrOCRForCausalLM`); `generate(pixel_values)` (app.ipynb:845) is transformers' greedy search and refuses settings that ask
    for anything else; `beam_search(pixel_values)` is transformers' beam search with the checkpoint's own num_beams / length_penalty /
    early_stopping.  Not implemented (refused where a config asks for it): sampling, group / constrained beam search, logits
    processors (no_repeat_ngram_size, repetition_penalty, min_length, forced tokens, ...), several eos ids, an encoder wider than the
    decoder's cross-attention (`enc_to_dec_proj`)."""

    def __init__(self, encoder=None, decoder=None, generation_config=None):
        super().__init__()
        self.encoder = encoder if encoder is not None else TrOCREncoder()
        self.decoder = decoder if decoder is not None else TrOCRForCausalLM()
        kdim = self.decoder.config.cross_attention_hidden_size or self.decoder.config.d_model
        if self.encoder.config.hidden_size != kdim:
            raise NotImplementedError(f"VisionEncoderDecoderModel: encoder width {self.encoder.config.hidden_size} != cross-attention width {kdim} "
                                      "(enc_to_dec_proj) is not implemented")
        dc = self.decoder.config
        gen = dict(decoder_start_token_id=dc.decoder_start_token_id, eos_token_id=dc.eos_token_id, pad_token_id=dc.pad_token_id,
                   max_length=20, max_new_tokens=None)
        gen.update(generation_config or {})
        self.generation_config = _Config(**gen)

    def to(self, *args, **kwargs):
        self.encoder.to(*args, **kwargs)
        self.decoder.to(*args, **kwargs)
        return self

    def cuda(self, device=None):
        return self.to(torch.device("cuda" if device is None else device))

    def eval(self):
        return self

    @classmethod
    def from_pretrained(cls, pretrained_model_name_or_path, subfolder=None, revision=None, **kw):
        """transformers' VisionEncoderDecoder directory: config.json (`encoder` / `decoder` entries), generation_config.json if
        present, model.safetensors or pytorch_model.bin with `encoder.*` / `decoder.*` keys"""
        d = pretrained_model_name_or_path if subfolder is None else os.path.join(pretrained_model_name_or_path, subfolder)
        with open(os.path.join(d, "config.json")) as f:
            cfg = json.load(f)
        ecfg, dcfg = cfg.get("encoder"), cfg.get("decoder")
        if ecfg is None or dcfg is None:
            raise ValueError(f"{d}: config.json has no encoder / decoder entries (not a VisionEncoderDecoder checkpoint)")
        if ecfg.get("hidden_act", "gelu") != "gelu":
            raise NotImplementedError(f"VisionEncoderDecoderModel: encoder hidden_act={ecfg['hidden_act']!r}")
        encoder = TrOCREncoder(**{k: ecfg[k] for k in TROCR_LARGE_VIT_CONFIG if k in ecfg})
        decoder = TrOCRForCausalLM(**{k: dcfg[k] for k in TROCR_LARGE_DECODER_CONFIG if k in dcfg})
        gen = {k: cfg[k] for k in ("decoder_start_token_id", "eos_token_id", "pad_token_id", "max_length") if cfg.get(k) is not None}
        gp = os.path.join(d, "generation_config.json")
        if os.path.exists(gp):
            with open(gp) as f:
                g = json.load(f)
            gen.update({k: v for k, v in g.items() if not k.startswith("_") and k != "transformers_version"})
        for k in _GEN_UNSUPPORTED:                   # settings the config.json itself carries (transformers' legacy generation keys)
            if k not in gen and cfg.get(k) is not None:
                gen[k] = cfg[k]
        model = cls(encoder, decoder, gen)
        sd = load_weights_file(d, "model.safetensors", "pytorch_model.bin")
        if any(k.startswith("enc_to_dec_proj.") for k in sd):
            raise NotImplementedError("VisionEncoderDecoderModel: enc_to_dec_proj is not implemented")
        enc_sd = TrOCREncoder._convert_legacy_keys({k: v for k, v in sd.items() if k.startswith("encoder.")})
        dec_sd = {k[len("decoder."):]: v for k, v in sd.items() if k.startswith("decoder.")}
        if decoder.config.tie_word_embeddings:
            dec_sd.pop("output_projection.weight", None)
        encoder.load_state_dict(enc_sd)
        decoder.load_state_dict(dec_sd)
        return model

    def _call_args(self, who, check, pixel_values, encoder_hidden_states, max_new_tokens, max_length, kwargs, **named):
        """what generate() / beam_search() were called with -> (settings g: the generation config overridden by the call, total
        length L, the one eos id or None); check(g) refuses the settings `who` does not implement"""
        unknown = set(kwargs) - set(_GEN_UNSUPPORTED) - {"decoder_start_token_id", "eos_token_id", "pad_token_id"}
        if unknown:
            raise TypeError(f"{who}() got unexpected keyword arguments {sorted(unknown)}")
        g = self.generation_config.to_dict()
        g.update({k: v for k, v in dict(kwargs, **named).items() if v is not None})
        check(g)
        if (pixel_values is None) == (encoder_hidden_states is None):
            raise ValueError(f"{who}: pass exactly one of pixel_values / encoder_hidden_states")
        if max_new_tokens is not None:
            L = 1 + int(max_new_tokens)
        elif max_length is not None:
            L = int(max_length)
        elif g.get("max_new_tokens") is not None:
            L = 1 + int(g["max_new_tokens"])
        else:
            L = int(g.get("max_length") or 20)
        if L > self.decoder.config.max_position_embeddings:
            raise ValueError(f"{who}: max_length {L} exceeds the decoder's {self.decoder.config.max_position_embeddings} positions")
        if L < 1:
            raise ValueError(f"{who}: max_length must be >= 1")
        eos = g.get("eos_token_id")
        if isinstance(eos, (list, tuple)):
            if len(eos) != 1:
                raise NotImplementedError(f"{who}: several eos_token_id values are not implemented")
            eos = eos[0]
        return g, L, eos

    def _enc_shape(self, pixel_values, encoder_hidden_states):
        """the shape the decoder's argument checks take: the encoder states', or [B, 1, kdim] standing in for the encoder's output"""
        if encoder_hidden_states is not None:
            return tuple(encoder_hidden_states.shape)
        if pixel_values.ndim != 4:
            raise ValueError(f"pixel_values must be [B, C, H, W], got {tuple(pixel_values.shape)}")
        return (pixel_values.shape[0], 1, self.decoder.config.cross_attention_hidden_size or self.decoder.config.d_model)

    def _score_inputs(self, who, pixel_values, encoder_hidden_states, labels, decoder_input_ids, ignore_index):
        """the argument checks of forward() / score(), all before the encoder runs"""
        if (pixel_values is None) == (encoder_hidden_states is None):
            raise ValueError(f"{who}: pass exactly one of pixel_values / encoder_hidden_states")
        if labels is None and decoder_input_ids is None:
            raise ValueError(f"{who}: pass labels or decoder_input_ids")
        self.decoder._check_score_args(self._enc_shape(pixel_values, encoder_hidden_states), labels, decoder_input_ids, ignore_index)

    @torch.no_grad()
    def score(self, pixel_values=None, *, encoder_hidden_states=None, labels=None, decoder_input_ids=None, decoder_start_token_id=None,
              pad_token_id=None, ignore_index=-100, return_logits=False):
        """how well the boxes read as `labels` [B, T] (ids; -100 = ignored): `TrOCRForCausalLM.score` on the encoder's states, or on
        encoder_hidden_states computed earlier.  No logits unless asked: what a best-of-N loop calls."""
        self._score_inputs("score", pixel_values, encoder_hidden_states, labels, decoder_input_ids, ignore_index)
        g = self.generation_config
        start = g.decoder_start_token_id if decoder_start_token_id is None else decoder_start_token_id
        pad = g.pad_token_id if pad_token_id is None else pad_token_id
        if encoder_hidden_states is None:
            encoder_hidden_states = self.encoder(pixel_values).last_hidden_state
        return self.decoder.score(labels, encoder_hidden_states, decoder_start_token_id=start, pad_token_id=pad, ignore_index=ignore_index,
                                  decoder_input_ids=decoder_input_ids, return_logits=return_logits)

    @torch.no_grad()
    def forward(self, pixel_values=None, labels=None, decoder_input_ids=None, encoder_outputs=None, return_dict=True):
        """transformers' `VisionEncoderDecoderModel.forward`: Seq2SeqLMOutput(loss, logits, encoder_last_hidden_state).  `labels`
        [B, T] (-100 = ignored) give the loss and the logits of the labels shifted right; `decoder_input_ids` alone give logits with
        loss None; encoder_outputs (a BaseModelOutput or a tuple) stands in for pixel_values.  Forward-only."""
        enc = None
        if encoder_outputs is not None:
            enc = encoder_outputs.last_hidden_state if hasattr(encoder_outputs, "last_hidden_state") else encoder_outputs[0]
        self._score_inputs("forward", pixel_values, enc, labels, decoder_input_ids, -100)
        if enc is None:
            enc = self.encoder(pixel_values).last_hidden_state
        g = self.generation_config
        out = self.decoder.score(labels, enc, decoder_start_token_id=g.decoder_start_token_id, pad_token_id=g.pad_token_id,
                                 decoder_input_ids=decoder_input_ids, return_logits=True)
        res = Seq2SeqLMOutput(out.loss, out.logits, enc)
        return res if return_dict else res.to_tuple()

    @torch.no_grad()
    def generate(self, pixel_values=None, *, encoder_hidden_states=None, max_new_tokens=None, max_length=None, num_beams=None,
                 use_graph=True, **kwargs):
        """greedy ids [B, L] (int64, on the device), L counting the decoder start token - transformers' `generate` with
        num_beams=1, do_sample=False.  Rows that emitted eos_token_id continue with pad_token_id; generation stops when every
        row has finished or at max_length (default 20) / 1 + max_new_tokens."""
        g, L, eos = self._call_args("generate", lambda g: _check_generation(g, explicit_beams=num_beams == 1), pixel_values,
                                    encoder_hidden_states, max_new_tokens, max_length, kwargs, num_beams=num_beams)
        if encoder_hidden_states is None:
            encoder_hidden_states = self.encoder(pixel_values).last_hidden_state
        ids, _ = self.decoder.greedy(encoder_hidden_states, L, g["decoder_start_token_id"], eos, g.get("pad_token_id"),
                                     use_graph=use_graph)
        return ids

    @torch.no_grad()
    def beam_search(self, pixel_values=None, *, encoder_hidden_states=None, max_new_tokens=None, max_length=None, num_beams=None,
                    length_penalty=None, early_stopping=None, num_return_sequences=None, return_scores=False, use_graph=True, **kwargs):
        """beam-search ids [B * num_return_sequences, L] (int64, on the device) - transformers' `generate` with num_beams > 1,
        do_sample=False.  Settings not passed come from generation_config (what from_pretrained read; else length_penalty 1.0,
        early_stopping False, num_return_sequences 1, max_length 20).  With return_scores also `sequences_scores`."""
        def check(g):
            _check_unsupported("beam_search", g, _BEAM_SEARCH_OWN, lambda k: " (remove it from the call / generation_config)")
            nb = g.get("num_beams")
            if isinstance(nb, bool) or not isinstance(nb, int) or not 2 <= nb <= 16:
                raise ValueError(f"beam_search: num_beams must resolve to 2 ... 16, got {nb!r} (generate() runs greedy search)")

        g, L, eos = self._call_args("beam_search", check, pixel_values, encoder_hidden_states, max_new_tokens, max_length, kwargs, num_beams=num_beams,
                                    length_penalty=length_penalty, early_stopping=early_stopping, num_return_sequences=num_return_sequences)
        nb, lp, es, nret = g["num_beams"], g.get("length_penalty"), g.get("early_stopping"), g.get("num_return_sequences")
        lp, es, nret = (1.0 if lp is None else float(lp)), (False if es is None else es), (1 if nret is None else int(nret))
        # every argument check before anything touches the device
        self.decoder._check_beam_args(self._enc_shape(pixel_values, encoder_hidden_states), L, nb, lp, es, nret)
        if encoder_hidden_states is None:
            encoder_hidden_states = self.encoder(pixel_values).last_hidden_state
        ids, scores, _ = self.decoder.beam_search(encoder_hidden_states, L, g["decoder_start_token_id"], eos, g.get("pad_token_id"), num_beams=nb,
                                                  length_penalty=lp, early_stopping=es, num_return_sequences=nret, use_graph=use_graph)
        return (ids, scores) if return_scores else ids
