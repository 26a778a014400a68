"""In-flight batching of the denoise loop: every row of the UNet batch on its own schedule.

`denoise()` gives the whole batch one timestep per step, so requests batch only when they start together and run the same number of
steps.  `DenoiseEngine` keeps a batch of `capacity` rows running: a request (one or several rows sharing a step count) takes free rows
whenever they come up, runs ITS `num_inference_steps` ticks and leaves, while the other rows are mid-loop.  One tick is one UNet forward
over all rows (`dmx_unet_forward` with per-row timesteps: each row fetches its own row of the time-embedding table), one per-row
scheduler launch (`dmx_sched_step_rows`, over the records of `scheduler.plan()` - the ones `denoise()` runs one at a time) and one
`dmx_rows_advance`.  Which step a row is on lives in two device ints per row (`row_index`, `row_left`) at fixed addresses, so one captured
graph serves every tick; the host mirrors that arithmetic (`Planner`) and never reads it back.

A request with classifier-free guidance (`submit(..., guidance=Guidance(...))`) is a request of 2n rows to the planner: rows [s0, s0+n) run
on the glyph context, rows [s0+n, s0+2n) on the unconditional one - the layout `denoise(guidance=)` gives its 2B rows -, both halves with
the same (plan_base, T), so they advance and retire together.  Which half a row is, its partner and the pair's own scale and rescale live
in a per-row device table (`dmx_rows_guide` writes a request's entries at admission and returns them to PLAIN when it leaves); while a
guided request is running the tick's scheduler launch is `dmx_sched_step_rows_guided` (schedulers.launch_step_rows_guided), which does a
plain row's update, a pair's guided update (into both of its rows) and nothing for idle rows in the same single launch.

`Planner`, `plan_records` and the queue are plain Python (no device calls): tests/test_inflight_host.py drives them without a GPU.
"""
import ctypes
from collections import deque

import torch

from . import _cabi
from .schedulers import Guidance, launch_step_rows_guided


# ----------------------------------------------------------------------------------------------------------------- host planner
class Planner:
    """Slot assignment, the FIFO queue and the per-row counters of a DenoiseEngine, as the device sees them.

    A request of n rows and T steps waits until it is the head of the queue and n CONSECUTIVE rows are free (the lowest such run); nothing
    overtakes the head.  `row_index[b]` / `row_left[b]` mirror the device ints: admit sets (plan_base, T) on each of the n rows, advance()
    does index++, left-- on every active row and index = -1 at left == 0 (dmx_rows_admit / dmx_rows_advance)."""

    def __init__(self, capacity):
        if int(capacity) < 1:
            raise ValueError("capacity must be at least 1")
        self.capacity = int(capacity)
        self.row_index = [-1] * self.capacity
        self.row_left = [0] * self.capacity
        self.owner = [None] * self.capacity          # the ticket that holds each row
        self.queue = deque()                         # (ticket, n, T, plan_base)
        self.running = {}                            # ticket -> (slot0, n, T, plan_base)
        self.ticks = 0                               # ticks run so far (the index of the next one)
        self._next = 0

    def submit(self, n, steps, plan_base):
        n, steps = int(n), int(steps)
        if n < 1 or n > self.capacity:
            raise ValueError(f"a request of {n} rows does not fit an engine of capacity {self.capacity}")
        if steps < 1:
            raise ValueError("num_inference_steps must be at least 1")
        ticket = self._next
        self._next += 1
        self.queue.append((ticket, n, steps, int(plan_base)))
        return ticket

    def _free_run(self, n):
        run = 0
        for b in range(self.capacity):
            run = run + 1 if self.owner[b] is None else 0
            if run == n:
                return b - n + 1
        return None

    def admit(self):
        """-> [(ticket, slot0, n, T, plan_base)] admitted now, in queue order"""
        out = []
        while self.queue:
            ticket, n, T, base = self.queue[0]
            s0 = self._free_run(n)
            if s0 is None:
                break
            self.queue.popleft()
            for b in range(s0, s0 + n):
                self.owner[b], self.row_index[b], self.row_left[b] = ticket, base, T
            self.running[ticket] = (s0, n, T, base)
            out.append((ticket, s0, n, T, base))
        return out

    def active(self):
        return any(i >= 0 for i in self.row_index)

    def busy(self):
        return bool(self.queue) or self.active()

    def step_of(self, ticket):
        """the step (0-based) the running request `ticket` takes at the next tick"""
        s0, _, T, _ = self.running[ticket]
        return T - self.row_left[s0]

    def finishing(self):
        """[(ticket, slot0, n)] of the requests whose last step is the next tick"""
        return [(t, s0, n) for t, (s0, n, _, _) in self.running.items() if self.row_left[s0] == 1]

    def advance(self):
        """one tick: the device's advance rule on the mirror -> the tickets that finished, by slot"""
        done = []
        for b in range(self.capacity):
            if self.row_index[b] < 0:
                continue
            self.row_left[b] -= 1
            if self.row_left[b] > 0:
                self.row_index[b] += 1
            else:
                self.row_index[b] = -1
                t = self.owner[b]
                self.owner[b] = None
                if t not in done:
                    done.append(t)
        for t in done:
            del self.running[t]
        self.ticks += 1
        return done


def scheduler_kind(scheduler):
    kind = getattr(scheduler, "kind", None)
    if kind is None:
        raise TypeError(f"DenoiseEngine: no per-row step for {type(scheduler).__name__}")
    return kind


def plan_records(scheduler, num_inference_steps, eta=0.0):
    """The plan of one step count: scheduler.set_timesteps(num_inference_steps) (pass a PRIVATE scheduler: it is mutated), then
    scheduler.plan(eta) - the records denoise()'s loop reads, one per step.  -> (timesteps, records); DPM-Solver++ may return fewer steps
    than asked (its grid is deduplicated)."""
    scheduler_kind(scheduler)
    scheduler.set_timesteps(int(num_inference_steps))
    return [int(t) for t in scheduler.timesteps], scheduler.plan(eta)


# ----------------------------------------------------------------------------------------------------------------- the engine
class _Request:
    def __init__(self, lat, mask, mlat, ctx, variance_noise, guidance=None):
        self.lat, self.mask, self.mlat, self.ctx, self.variance_noise, self.guidance = lat, mask, mlat, ctx, variance_noise, guidance


class DenoiseEngine:
    """eng = DenoiseEngine(unet, scheduler, capacity=4, latent_shape=(4, 64, 64), ctx_len=577)
    ticket = eng.submit(latents, mask, masked_image_latents, encoder_hidden_states, num_inference_steps, guidance=None)
    finished = eng.tick()            # one UNet forward + one scheduler launch + one advance for all rows -> the tickets that finished
    latents = eng.result(ticket)     # fp32 [n,4,h,w]: a copy taken on the engine's stream at the finishing tick, before the rows are reused
    eng.run_until_idle()

    The arguments of submit() are those of denoise() for n >= 1 rows that share one step count; they wait in a FIFO queue until n
    consecutive rows are free and their glyph context is projected by ONE dmx_unet_set_context_rows call, so a request that fills the
    engine and starts alone computes denoise()'s result bit for bit.  DDIM (with `eta`), DDPM (device randn per tick, or the request's
    `variance_noise` [T,n,4,h,w]) and DPM-Solver++ are served; what denoise() refuses is refused with the same exception.  The
    caller's scheduler object is never mutated: plans come from a private `type(scheduler).from_config(scheduler.config)`.

    guidance: a Guidance, denoise()'s classifier-free guidance, per request: its own scale, rescale and unconditional context.  The
    request then holds 2n consecutive rows (n on the glyph context, then the same n on the unconditional one), so 2n must fit the capacity;
    its result is still [n,4,h,w] and variance_noise still [T,n,4,h,w].  Guided and plain requests share the engine, and a tick is one
    forward, one scheduler launch and one advance either way; a guided request that fills the engine and starts alone computes
    denoise(guidance=)'s result bit for bit.  None, or a Guidance with scale 1.0 and rescale 0, is the plain request (n rows).

    All buffers (x, mask, masked latents, eps, the DPM history ring, noise, row_index, row_left, timesteps) keep their addresses for the
    life of the engine and the loop runs on the engine's own stream, so one captured graph serves every tick.  Plans are cached per
    num_inference_steps: the first request with a new step count uploads its records, computes its time-embedding rows
    (dmx_unet_temb_table) and appends both to the engine's plan array and table - which moves them, so the forward's graph is captured
    once more.  Neither submit() nor tick() synchronises with the device.  Rows nobody holds are zero latents (over a zeroed context
    until their first use, afterwards over the context of the request that left); their eps is computed, finite and ignored.

    The engine owns one execution slot of the UNet (its workspace and K/V cache); close() releases it."""

    def __init__(self, unet, scheduler, capacity=4, latent_shape=(4, 64, 64), ctx_len=577, eta=0.0, use_graph=True):
        self.kind = scheduler_kind(scheduler)
        if self.kind == _cabi.SCHED_DPMPP and eta != 0:
            raise ValueError("DPMSolverMultistepScheduler is deterministic: no variance_noise, eta = 0")
        self.unet, self.eta, self.use_graph = unet, float(eta), bool(use_graph)
        self.capacity, self.ctx_len = int(capacity), int(ctx_len)
        self.latent_shape = tuple(int(v) for v in latent_shape)
        C, h, w = self.latent_shape
        cfg = unet.config
        if C != cfg.out_channels or h % 8 or w % 8 or h < 8 or w < 8:
            raise ValueError(f"latent_shape {self.latent_shape}: expected ({cfg.out_channels}, h, w) with h, w positive multiples of 8")
        self.planner = Planner(self.capacity)
        self._sched = type(scheduler).from_config(scheduler.config)
        self.vpred = int(self._sched.config.prediction_type == "v_prediction")
        self.n_hist = int(self._sched.config.solver_order) if self.kind == _cabi.SCHED_DPMPP else 0
        self.per = C * h * w
        dev = self.device = unet.device
        unet._ensure_packed()
        self.slot = ("inflight", id(self))
        self.stream = torch.cuda.Stream(device=dev)
        self.stream.wait_stream(torch.cuda.current_stream(dev))
        B = self.capacity
        with torch.cuda.stream(self.stream):
            f32 = dict(dtype=torch.float32, device=dev)
            self.x = torch.zeros(B, C, h, w, **f32)
            self.mask = torch.zeros(B, 1, h, w, **f32)
            self.mlat = torch.zeros(B, cfg.in_channels - C - 1, h, w, **f32)
            self.eps = torch.zeros_like(self.x)
            self.hist = torch.zeros(self.n_hist, B, C, h, w, **f32) if self.n_hist else None
            self.noise = torch.zeros_like(self.x) if self.kind != _cabi.SCHED_DPMPP else None
            self.row_index = torch.full((B,), -1, dtype=torch.int32, device=dev)
            self.row_left = torch.zeros(B, dtype=torch.int32, device=dev)
            self.guide = torch.zeros(B * ctypes.sizeof(_cabi.GuideRow), dtype=torch.uint8, device=dev)     # [B] dmx_guide_row, all PLAIN
            self.timesteps = torch.zeros(B, dtype=torch.int64, device=dev)
            unet.reserve_context(B, self.ctx_len, slot=self.slot)
        self.table = None                  # [rows of all plans][tproj] fp32
        self.plan_dev = None               # uint8: the records of all plans, the table's row numbering
        self.plan_host = []                # the same records on the host
        self._plans = {}                   # num_inference_steps -> (plan_base, T)
        self._pending = {}                 # ticket -> _Request (queued: all tensors; running: variance_noise only)
        self._results = {}
        self._guided = {}                  # ticket -> n: the guided requests, queued or running, and their samples (they hold 2n rows)

    # ---- plans
    def _plan(self, steps):
        steps = int(steps)
        if steps < 1:
            raise ValueError("num_inference_steps must be at least 1")
        hit = self._plans.get(steps)
        if hit is not None:
            return hit
        ts, recs = plan_records(self._sched, steps, self.eta)
        base, T = len(self.plan_host), len(ts)
        raw = b"".join(bytes(r) for r in recs)
        cur = torch.cuda.current_stream(self.device)
        # uploaded on the CALLER's stream (as denoise() uploads its timesteps): the copy queues behind the caller's work, not the engine's
        rec_dev = torch.frombuffer(bytearray(raw), dtype=torch.uint8).to(self.device)
        ts_dev = torch.tensor(ts, dtype=torch.int64).to(self.device)
        self.stream.wait_stream(cur)
        rec_dev.record_stream(self.stream); ts_dev.record_stream(self.stream)
        with torch.cuda.stream(self.stream):
            rows = self.unet.temb_table(ts_dev)
            self.table = rows if self.table is None else torch.cat([self.table, rows], 0)
            self.plan_dev = rec_dev.clone() if self.plan_dev is None else torch.cat([self.plan_dev, rec_dev], 0)
        self.plan_host.extend(recs)
        self._plans[steps] = (base, T)
        return base, T

    # ---- requests
    def submit(self, latents, mask, masked_image_latents, encoder_hidden_states, num_inference_steps, variance_noise=None, guidance=None):
        if guidance is not None and not isinstance(guidance, Guidance):
            raise TypeError(f"guidance must be a diffute_amd.Guidance or None, got {type(guidance).__name__}")
        _cabi.require_cuda(latents, mask, masked_image_latents, encoder_hidden_states, variance_noise)
        if self.kind == _cabi.SCHED_DPMPP and variance_noise is not None:
            raise ValueError("DPMSolverMultistepScheduler is deterministic: no variance_noise, eta = 0")
        C, h, w = self.latent_shape
        n = int(latents.shape[0]) if latents.dim() == 4 else -1
        if latents.dim() != 4 or tuple(latents.shape[1:]) != self.latent_shape:
            raise ValueError(f"latents {tuple(latents.shape)}: expected [n, {C}, {h}, {w}]")
        if n < 1 or n > self.capacity:
            raise ValueError(f"a request of {n} rows does not fit an engine of capacity {self.capacity}")
        if tuple(mask.shape) != (n, 1, h, w) or tuple(masked_image_latents.shape) != (n,) + tuple(self.mlat.shape[1:]):
            raise ValueError(f"mask {tuple(mask.shape)} / masked_image_latents {tuple(masked_image_latents.shape)} do not match {n} rows of "
                             f"latents [{C}, {h}, {w}]")
        D = self.unet.config.cross_attention_dim
        if tuple(encoder_hidden_states.shape) != (n, self.ctx_len, D):
            raise ValueError(f"encoder_hidden_states {tuple(encoder_hidden_states.shape)}: expected [{n}, {self.ctx_len}, {D}] (the engine's "
                             "context length is fixed)")
        if guidance is not None:
            guidance.check_context(encoder_hidden_states)
            guidance = guidance if guidance.active else None
        if guidance is not None and 2 * n > self.capacity:
            raise ValueError(f"a guided request of {n} samples holds {2 * n} rows and does not fit an engine of capacity {self.capacity}")
        base, T = self._plan(num_inference_steps)
        if variance_noise is not None and (variance_noise.dim() != 5 or variance_noise.shape[0] < T or tuple(variance_noise.shape[1:]) != (n, C, h, w)):
            raise ValueError(f"variance_noise {tuple(variance_noise.shape)}: expected [{T}, {n}, {C}, {h}, {w}]")
        ticket = self.planner.submit(n if guidance is None else 2 * n, T, base)
        self.stream.wait_stream(torch.cuda.current_stream(self.device))      # the inputs were produced on the caller's stream
        for t in (latents, mask, masked_image_latents, encoder_hidden_states, variance_noise, None if guidance is None else guidance.uncond):
            if t is not None:
                t.record_stream(self.stream)
        self._pending[ticket] = _Request(latents, mask, masked_image_latents, encoder_hidden_states, variance_noise, guidance)
        if guidance is not None:
            self._guided[ticket] = n
        self._admit()
        return ticket

    def _admit(self):
        lib = self.unet._lib
        for ticket, s0, rows, T, base in self.planner.admit():
            rq = self._pending[ticket]
            g = rq.guidance
            n = rows if g is None else rows // 2
            with torch.cuda.stream(self.stream):
                st = _cabi.current_stream()
                lat = rq.lat.to(torch.float32) * self._sched.init_noise_sigma      # app.ipynb:800
                for lo in range(s0, s0 + rows, n):                                  # guided: the second half is a duplicate of the first
                    self.x[lo:lo + n].copy_(lat)
                    self.mask[lo:lo + n].copy_(rq.mask)
                    self.mlat[lo:lo + n].copy_(rq.mlat)
                self.unet.set_context_rows(rq.ctx if g is None else torch.cat([rq.ctx, g.uncond_for(rq.ctx)], 0), s0, slot=self.slot)
                for b in range(s0, s0 + rows):
                    _cabi.check(lib.dmx_rows_admit(_cabi.ptr(self.row_index), _cabi.ptr(self.row_left), b, base, T, st), "rows_admit", lib)
                if g is not None:
                    _cabi.check(lib.dmx_rows_guide(_cabi.ptr(self.guide), s0, n, 1, g.scale, g.rescale, float(1 - g.rescale), st), "rows_guide", lib)
            rq.lat = rq.mask = rq.mlat = rq.ctx = rq.guidance = None
            if rq.variance_noise is None:
                del self._pending[ticket]

    def _fill_noise(self):
        """the noise rows of this tick: a request's injected variance_noise[step], device randn for the rest (drawn for the whole buffer).
        A guided request's noise goes to its conditional rows; the step never reads the noise of the unconditional ones."""
        pl = self.planner
        inject, draw = [], False
        for ticket, (s0, n, _, _) in pl.running.items():
            n = self._guided.get(ticket, n)
            if not self.plan_host[pl.row_index[s0]].use_noise:
                continue
            rq = self._pending.get(ticket)
            if rq is None:
                draw = True
            else:
                inject.append((s0, n, rq.variance_noise[pl.step_of(ticket)]))
        if draw:
            self.noise.normal_()
        for s0, n, vn in inject:
            self.noise[s0:s0 + n].copy_(vn)

    def tick(self):
        """Admit what fits, then one step of every active row.  -> the tickets that finished in this tick (their results are ready on the
        engine's stream: result()).  Without an active row nothing is launched."""
        _cabi.poll_device_error()            # what a kernel of an EARLIER tick raised (no sync)
        self._admit()
        pl = self.planner
        if not pl.active():
            return []
        lib = self.unet._lib
        with torch.cuda.stream(self.stream):
            st = _cabi.current_stream()
            self.unet.forward_parts([self.x, self.mask, self.mlat], self.timesteps, out=self.eps, graph=self.use_graph, slot=self.slot,
                                    temb=(self.table, self.row_index, self.plan_dev))
            if self.noise is not None:
                self._fill_noise()
            if any(t in pl.running for t in self._guided):       # a guided request is running (the mirror knows: no readback)
                launch_step_rows_guided(self.kind, self.x, self.eps, self.noise, self.hist, self.plan_dev, self.row_index, self.guide, self.vpred,
                                        st, lib=lib)
            else:
                _cabi.check(lib.dmx_sched_step_rows(_cabi.ptr(self.x), _cabi.ptr(self.eps), _cabi.ptr(self.noise), _cabi.ptr(self.hist), self.n_hist,
                                                    _cabi.ptr(self.plan_dev), _cabi.ptr(self.row_index), self.capacity, self.per, self.kind,
                                                    self.vpred, st), "sched_step_rows", lib)
            for ticket, s0, n in pl.finishing():
                samples = self._guided.pop(ticket, None)         # guided: n = 2 * samples rows, the result is the conditional half
                self._results[ticket] = self.x[s0:s0 + (n if samples is None else samples)].clone()
                self.x[s0:s0 + n].zero_(); self.mask[s0:s0 + n].zero_(); self.mlat[s0:s0 + n].zero_()
                if samples is not None:
                    _cabi.check(lib.dmx_rows_guide(_cabi.ptr(self.guide), s0, n, 0, 1.0, 0.0, 1.0, st), "rows_guide", lib)
                self._pending.pop(ticket, None)
            _cabi.check(lib.dmx_rows_advance(_cabi.ptr(self.row_index), _cabi.ptr(self.row_left), self.capacity, st), "rows_advance", lib)
        return pl.advance()

    def result(self, ticket):
        """The final latents of a finished request (fp32 [n,4,h,w]); the caller's current stream is made to wait for the engine's."""
        if ticket not in self._results:
            raise KeyError(f"ticket {ticket}: not finished (or its result was taken already)")
        torch.cuda.current_stream(self.device).wait_stream(self.stream)
        return self._results.pop(ticket)

    def run_until_idle(self):
        """tick() until the queue is empty and every row is idle -> the finished tickets in finishing order"""
        done = []
        while self.planner.busy():
            done += self.tick()
        return done

    def close(self):
        """release the engine's UNet execution slot (workspace, K/V cache)"""
        self.unet._slots.pop(self.slot, None)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
