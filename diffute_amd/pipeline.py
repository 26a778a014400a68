"""The reference's denoise loop (app.ipynb:796-816) driven through the C-ABI.

`denoise()` is the hot path BASELINE.json names: per step one `dmx_unet_forward` (which fuses
torch.cat([latents, mask, masked_image_latents], 1)) and one scheduler-step kernel.  What a step is
comes from the scheduler's plan (`scheduler.iter_plan(eta)`, the records of `plan(eta)` one at a time) -
one record per step with the scalars, whether noise is added and,
for DPM-Solver++, the slots of the per-chain history ring it writes and reads - and goes to the kernel
through `schedulers.launch_step`; the loop knows nothing else about the scheduler.  The glyph context
K/V are projected once per image, timesteps live on the device, nothing synchronises with the host
inside the loop.
"""
import numpy as np
import torch

from . import _cabi, glyphs, prepost
from .schedulers import Guidance, launch_step, launch_step_guided


_SIDE = {}
TEMB_TABLE = True      # denoise(): time-embedding projections of all steps in one batched pass (False: four small launches per step; A/B aid)


def _side_streams(device, n):
    key = str(device)
    pool = _SIDE.setdefault(key, [])
    while len(pool) < n:
        pool.append(torch.cuda.Stream(device=device))
    return pool


def mask_to_latent(mask, vae_scale_factor=8):
    """F.interpolate(mask, size=(H/8, W/8)) with the default nearest mode (app.ipynb:787-791,
    train_diffute_v1.py:880-884): out[y, x] = in[floor(y*8), floor(x*8)]."""
    return mask[:, :, ::vae_scale_factor, ::vae_scale_factor].to(torch.float32).contiguous()


class _Run:
    """One micro-batch of the denoise loop: its own stream, UNet execution slot and fixed-address buffers."""

    def __init__(self, unet, scheduler, latents, mask, mlat, ctx, slot, stream, use_graph, ts_dev, temb_table, table_rows, cache_interval=1,
                 guidance=None):
        self.unet, self.slot, self.stream, self.use_graph = unet, slot, stream, use_graph
        self.guidance, self.B = guidance, latents.shape[0]
        self.cache_interval, self.cache = cache_interval, None
        self.kind, self.vpred = scheduler.kind, int(scheduler.config.prediction_type == "v_prediction")
        self.ts_dev, self.temb_table, self.table_rows = ts_dev, temb_table, table_rows
        with torch.cuda.stream(stream):
            self.x = (latents.to(torch.float32) * scheduler.init_noise_sigma).contiguous()      # app.ipynb:800
            self.m = mask.to(torch.float32).contiguous()
            self.ml = mlat.to(torch.float32).contiguous()
            if guidance is not None:
                # guided: rows [0,B) run on the glyph context and rows [B,2B) on the unconditional one.  The second half of x / mask / masked
                # latents is a duplicate made once, here; the guided step writes both halves of x.  The ring and the noise stay [B].
                self.x, self.m, self.ml = (torch.cat([t, t], 0) for t in (self.x, self.m, self.ml))
                ctx = torch.cat([ctx, guidance.uncond_for(ctx)], 0)
            self.eps = torch.empty_like(self.x)
            # DPM-Solver++: the ring of the data predictions of the last solver_order steps; a step's record names the slots it writes and reads
            n_hist = scheduler.config.solver_order if self.kind == _cabi.SCHED_DPMPP else 0
            if guidance is None:
                self.hist = [torch.empty_like(self.x) for _ in range(n_hist)]
            else:                        # one tensor [n_hist][B][...]: the guided step takes the ring whole and finds the slots from the record
                self.hist = torch.empty((n_hist, self.B) + tuple(self.x.shape[1:]), dtype=torch.float32, device=self.x.device) if n_hist else None
            self.t_cur = torch.empty(1, dtype=torch.int64, device=self.x.device)   # fixed address: the captured graph reads it
            self.step_idx = torch.zeros(1, dtype=torch.int32, device=self.x.device)   # likewise: the row of temb_table this step fetches
            unet.set_context(ctx, slot=slot)
            if cache_interval > 1:       # this chain's own step cache: step i is full (and refills it) iff i % cache_interval == 0
                self.cache = unet.step_cache(*self.x.shape[:1], *self.x.shape[2:])

    def step(self, i, rec, noise):
        x, eps = self.x, self.eps
        sc = {} if self.cache is None else dict(step_cache=(self.cache, "use" if i % self.cache_interval else "fill"))
        with torch.cuda.stream(self.stream):
            if self.temb_table is not None:
                self.step_idx.copy_(self.table_rows[i:i + 1], non_blocking=True)
                self.unet.forward_parts([x, self.m, self.ml], self.t_cur, out=eps, graph=self.use_graph, slot=self.slot,
                                        temb=(self.temb_table, self.step_idx), **sc)
            else:
                self.t_cur.copy_(self.ts_dev[i:i + 1], non_blocking=True)
                self.unet.forward_parts([x, self.m, self.ml], self.t_cur, out=eps, graph=self.use_graph, slot=self.slot, **sc)
            # the update is elementwise, so prev_sample overwrites the sample in place (stable pointers for the graph)
            if self.guidance is not None:
                launch_step_guided(self.kind, rec, x, eps, noise, self.hist, self.vpred, self.guidance.scale, self.guidance.rescale,
                                   _cabi.current_stream())
                return
            launch_step(self.kind, rec, x, eps, noise, self.hist[rec.ring_m1] if rec.order >= 2 else None,
                        self.hist[rec.ring_m2] if rec.order >= 3 else None, self.hist[rec.ring_w] if self.hist else None, x, self.vpred,
                        _cabi.current_stream())


def _rows(runs, name):
    """the chains' x (the [B] latents) or eps (the raw model output: [B], guided [2B] with the conditional rows first) as one tensor"""
    if runs[0].guidance is None:
        return getattr(runs[0], name) if len(runs) == 1 else torch.cat([getattr(r, name) for r in runs], 0)
    if name == "x":
        return runs[0].x[:runs[0].B] if len(runs) == 1 else torch.cat([r.x[:r.B] for r in runs], 0)
    return runs[0].eps if len(runs) == 1 else torch.cat([r.eps[:r.B] for r in runs] + [r.eps[r.B:] for r in runs], 0)


def _check_guidance(guidance, encoder_hidden_states=None, N=None):
    """the guidance= argument of denoise and the edit functions, checked on the host -> the Guidance to run, None for the plain loop.
    encoder_hidden_states: the conditional contexts where they are known already (a per-row uncond must fit them), N their number."""
    if guidance is None:
        return None
    if not isinstance(guidance, Guidance):
        raise TypeError(f"guidance must be a diffute_amd.Guidance or None, got {type(guidance).__name__}")
    if encoder_hidden_states is not None:
        guidance.check_context(encoder_hidden_states, N)
    elif guidance.uncond is not None and N is not None and guidance.uncond.shape[0] not in (1, N):
        raise ValueError(f"Guidance: uncond {tuple(guidance.uncond.shape)} does not fit {N} boxes")
    return guidance if guidance.active else None


def _check_cache_interval(cache_interval):
    """denoise's cache_interval, checked before anything touches the device -> the int"""
    if isinstance(cache_interval, bool) or not isinstance(cache_interval, (int, np.integer)) or cache_interval < 1:
        raise ValueError(f"cache_interval must be an int >= 1, got {cache_interval!r}")
    return int(cache_interval)


@torch.no_grad()
def denoise(unet, scheduler, latents, mask, masked_image_latents, encoder_hidden_states,
            num_inference_steps, variance_noise=None, eta=0.0, callback=None, use_graph=True, micro_batches=1, cache_interval=1,
            guidance=None):
    """latents/masked_image_latents [B,4,h,w], mask [B,1,h,w] (already at latent resolution), context
    [B,S,1024]; all on the GPU.  variance_noise: optional [steps,B,4,h,w] injected in place of the
    per-step device randn of DDPMScheduler.step (app.ipynb:816).  Returns the final latents (fp32).

    micro_batches=n splits the batch into n independent chains (images do not interact), each on its own stream
    with its own captured graph: one chain's kernels fill the CUs the other chain's small / draining kernels
    leave idle.  Results are identical to micro_batches=1 up to per-kernel tile-plan rounding.

    cache_interval=n > 1 reuses the deep UNet features across steps (DeepCache; Ma et al., CVPR 2024): step i of the plan runs the whole
    UNet iff i % n == 0 and keeps the tensor entering the last up-block; the other steps run only conv_in, down-block 0, the last up-block
    on the kept tensor and the output layers (UNet2DConditionModel.forward_parts(step_cache=)).  Every step still produces an eps, so the
    schedulers - DPM-Solver++'s history ring included - see nothing of it.  The result differs from the plain loop's by design (how much
    depends on the weights; not a rounding effect).  n = 1 is the plain loop: no cache, the plain entry points.

    guidance: a Guidance - classifier-free guidance.  Each chain then holds 2b rows (its b rows on the glyph context, then the same b rows
    on the unconditional context), runs one 2b-row forward per step and one guided step (schedulers.launch_step_guided: the combination,
    the optional rescale and the scheduler update in one launch, which also writes the new latents into both halves), so a guided pass at
    B launches what a plain pass at 2B launches.  The result is rows [0,B); `callback` gets those and the raw [2B] model output
    (conditional rows first).  None, or a Guidance with scale 1.0 and rescale 0, is the plain loop, bit for bit."""
    cache_interval = _check_cache_interval(cache_interval)
    guidance = _check_guidance(guidance, encoder_hidden_states)
    _cabi.require_cuda(latents, mask, masked_image_latents, encoder_hidden_states)
    if scheduler.kind == _cabi.SCHED_DPMPP and (variance_noise is not None or eta != 0):
        raise ValueError("DPMSolverMultistepScheduler is deterministic: no variance_noise, eta = 0")
    _cabi.poll_device_error()            # what a kernel of an EARLIER pass raised (no sync; include/diffute_hip.h dmx_device_error)
    unet._ensure_packed()
    scheduler.set_timesteps(int(num_inference_steps))
    dev = latents.device
    ts_dev = scheduler.timesteps.to(device=dev, dtype=torch.int64).contiguous()
    B = latents.shape[0]
    n = max(1, min(int(micro_batches), B))
    bounds = [(B * j // n, B * (j + 1) // n) for j in range(n)]
    main = torch.cuda.current_stream(dev)
    # the time-embedding MLP + every resnet's time_emb_proj depend on the timestep only: all steps' rows in one batched pass up
    # front (bit-identical rows), each step then fetches its row with one tiny launch instead of recomputing four small layers
    temb_table = unet.temb_table(ts_dev) if (len(ts_dev) and TEMB_TABLE) else None
    table_rows = torch.arange(len(ts_dev), dtype=torch.int32, device=dev)
    streams = _side_streams(dev, n)[:n]         # the loop runs on side streams: graph capture needs a non-default stream
    # several chains at once share the CUs: plans whose blocks wait for co-resident peers are off while they are enqueued (the plans are
    # chosen - and baked into the captured graphs, which are keyed on the setting - at enqueue time)
    lib_ = unet._lib
    old_exclusive = lib_.dmx_set_exclusive_device(0) if n > 1 else None
    try:
        runs = []
        for j, (lo, hi) in enumerate(bounds):
            streams[j].wait_stream(main)
            runs.append(_Run(unet, scheduler, latents[lo:hi], mask[lo:hi], masked_image_latents[lo:hi],
                             encoder_hidden_states[lo:hi].contiguous(), j, streams[j], use_graph, ts_dev, temb_table, table_rows, cache_interval,
                             None if guidance is None else guidance.rows(slice(lo, hi))))
        # the plan, one record per step, is all the loop knows about the scheduler; it is walked lazily, so that the host computes a step's
        # scalars while the GPU works through the steps already enqueued
        for i, rec in enumerate(scheduler.iter_plan(eta)):
            for (lo, hi), run in zip(bounds, runs):
                nz = None
                if rec.use_noise:
                    with torch.cuda.stream(run.stream):
                        nz = (variance_noise[i][lo:hi] if variance_noise is not None else torch.randn_like(run.x[:run.B])).to(torch.float32).contiguous()
                run.step(i, rec, nz)
            if callback is not None:
                for s_ in streams:
                    main.wait_stream(s_)
                callback(i, int(rec.timestep), _rows(runs, "x"), _rows(runs, "eps"))
                for s_ in streams:
                    s_.wait_stream(main)            # the callback's reads finish before the next step overwrites x / eps
        for s_ in streams:
            main.wait_stream(s_)
        return _rows(runs, "x")
    finally:
        if old_exclusive is not None:
            lib_.dmx_set_exclusive_device(old_exclusive)


@torch.no_grad()
def edit_latents(unet, vae, scheduler, image, masked_image, mask, encoder_hidden_states, num_inference_steps,
                 init_latents=None, generator=None, enc_noise=None, variance_noise=None, cache_interval=1, *, guidance=None):
    """The model part of text_editing() (app.ipynb:779-819): VAE-encode the masked crop, downsample the
    mask, denoise from seeded noise, VAE-decode.  `image` is unused by the arithmetic (the reference's encode of it,
    app.ipynb:781, is dead code: its result is overwritten at :798); enc_noise / variance_noise inject the two device-RNG
    draws (latent_dist.sample(), DDPMScheduler.step) for tests.  Crop / resize / paste: diffute_amd.prepost.  cache_interval, guidance: denoise's."""
    cache_interval = _check_cache_interval(cache_interval)
    _check_guidance(guidance, encoder_hidden_states)
    sf = vae.config.scaling_factor
    f = 2 ** (len(vae.config.block_out_channels) - 1)
    m = mask_to_latent(mask, f)
    dist = vae.encode(masked_image).latent_dist
    mlat = (dist.sample(noise=enc_noise) if enc_noise is not None else dist.sample(generator=generator)) * sf   # app.ipynb:793-794
    B, _, H, W = masked_image.shape
    if init_latents is None:
        init_latents = torch.randn((B, vae.config.latent_channels, H // f, W // f),
                                   generator=torch.manual_seed(0), dtype=torch.float32).to(masked_image.device)  # :798
    lat = denoise(unet, scheduler, init_latents, m, mlat, encoder_hidden_states, num_inference_steps, variance_noise=variance_noise,
                  cache_interval=cache_interval, guidance=guidance)
    return vae.decode(lat / sf).sample                                                    # app.ipynb:818-819


@torch.no_grad()
def edit_boxes(unet, vae, scheduler, instance_image, locations, encoder_hidden_states, num_inference_steps, *, origins=None,
               crop_scales=None, rng=None, batch_size=4, generator=None, enc_noise=None, variance_noise=None,
               return_intermediate=False, size=512, cache_interval=1, texts=None, glyph=None, guidance=None, blend=None):
    """text_editing() (app.ipynb:674-846) for several boxes of ONE image as one batch: instance_image uint8 CUDA [h][w][3], locations
    N boxes (x1, y1, x2, y2), encoder_hidden_states [N,L,D] the glyph context of each box.  One preprocess_batch launch, the boxes
    through edit_latents in chunks of `batch_size` (the last chunk may be smaller), one postprocess_batch launch; returns the uint8
    [h][w][3] result, with return_intermediate=True also image_vae [N,3,S,S] and the preprocess dict.

    origins / crop_scales: N crop origins (x_s, y_s) / crop sides; what is not given comes from the reference's ladder and origin rule
    (prepost.plan_edits), random origins drawn from `rng` (default numpy's global state) in box order.  Every box starts from the
    reference's seed-0 [1,4,h,w] draw (app.ipynb:796-801), not from row b of a [N,...] draw: a box edited in a batch starts where a
    single call starts it.  enc_noise [N,4,h,w] / variance_noise [steps,N,4,h,w] inject the device-RNG draws as in edit_latents.

    Difference from N sequential text_editing() calls: every crop is taken from the ORIGINAL image, so box k's context does not contain
    the edits of boxes < k.  The pastes are identical (a later box wins where boxes overlap).  cache_interval: denoise's.

    texts / glyph: instead of encoder_hidden_states (pass None there), the N strings the boxes should show and
    glyph = (renderer, processor, encoder) - a GlyphRenderer, a TrOCRProcessor and a TrOCREncoder; the contexts are then
    glyph_contexts(texts, *glyph), rendered on the device.  Exactly one of encoder_hidden_states and texts must be given.

    guidance: a Guidance, denoise's classifier-free guidance for every chunk; an uncond of [N,S,D] is one unconditional context per box
    and is chunked like encoder_hidden_states.

    blend: None - the reference's hard paste -, or a PasteBlend: the paste gets a feathered edge and / or a colour match of every patch
    against the page around it (prepost.postprocess_batch), so the edited box does not show as a rectangle."""
    return _edit(False, unet, vae, scheduler, [instance_image], [locations], encoder_hidden_states, num_inference_steps, _one(origins),
                 _one(crop_scales), rng, batch_size, generator, enc_noise, variance_noise, return_intermediate, size, cache_interval, texts, glyph,
                 guidance, blend)


@torch.no_grad()
def edit_pages(unet, vae, scheduler, images, locations, encoder_hidden_states, num_inference_steps, *, origins=None, crop_scales=None,
               rng=None, batch_size=4, generator=None, enc_noise=None, variance_noise=None, return_intermediate=False, size=512,
               cache_interval=1, texts=None, glyph=None, guidance=None, blend=None):
    """edit_boxes for boxes on SEVERAL pages as one batch - what a service holding requests for different images, or a training batch
    of one box per image, needs.  images: a list of P contiguous uint8 CUDA [h_p][w_p][3] tensors on one device; locations: P lists of
    boxes (x1, y1, x2, y2); origins / crop_scales: None or P lists, as for edit_boxes per page (what is not given is planned page after
    page, random origins drawn from `rng` in that order: prepost.plan_pages).  Rows are page-major - page 0's boxes in order, then
    page 1's -, N in all: encoder_hidden_states [N,L,D], enc_noise [N,4,h,w], variance_noise [steps,N,4,h,w].

    One preprocess_pages launch, the N rows through edit_latents in chunks of `batch_size` (chunks cross page boundaries; every box
    starts from the seed-0 single-sample draw), one postprocess_pages launch.  Returns the list of P edited pages, with
    return_intermediate=True also image_vae [N,3,S,S] and the preprocess dict.  With one page this is [edit_boxes(...)], bit for bit.
    texts / glyph: as for edit_boxes, N strings page-major.  guidance: as for edit_boxes, a per-box uncond [N,S,D] page-major.
    blend: as for edit_boxes."""
    return _edit(True, unet, vae, scheduler, images, locations, encoder_hidden_states, num_inference_steps, origins, crop_scales, rng,
                 batch_size, generator, enc_noise, variance_noise, return_intermediate, size, cache_interval, texts, glyph, guidance, blend)


def _edit(paged, unet, vae, scheduler, images, locations, encoder_hidden_states, num_inference_steps, origins, crop_scales, rng, batch_size,
          generator, enc_noise, variance_noise, return_intermediate, size, cache_interval=1, texts=None, glyph=None, guidance=None, blend=None):
    """edit_boxes (paged=False: one page, its lists wrapped into one-element lists) and edit_pages"""
    if int(batch_size) < 1:
        raise ValueError("batch_size must be at least 1")
    _check_blend(blend)
    cache_interval = _check_cache_interval(cache_interval)
    images, locations, origins, crop_scales, sizes, N = _page_lists(paged, images, locations, origins, crop_scales)
    _check_contexts(N, encoder_hidden_states, texts, glyph)
    guidance = _check_guidance(guidance, encoder_hidden_states, N)
    where = _plan_pages(paged, images, locations, sizes, origins, crop_scales, rng)
    encoder_hidden_states = _contexts(encoder_hidden_states, texts, glyph)
    pre = (prepost.preprocess_pages if paged else prepost.preprocess_batch)(*where, size=size)
    image_vae = _edit_rows(unet, vae, scheduler, pre, images[0].device, encoder_hidden_states, num_inference_steps, int(batch_size), generator,
                           enc_noise, variance_noise, int(size), cache_interval, guidance)
    out = (prepost.postprocess_pages if paged else prepost.postprocess_batch)(image_vae, *where, blend=blend)
    return (out, image_vae, pre) if return_intermediate else out


@torch.no_grad()
def edit_quads(unet, vae, scheduler, images, quads, encoder_hidden_states, num_inference_steps, *, frames=None, batch_size=4, generator=None,
               enc_noise=None, variance_noise=None, return_intermediate=False, size=512, cache_interval=1, texts=None, glyph=None, guidance=None,
               perspective=False, blend=None):
    """edit_pages for skewed and rotated text: every region is a QUAD - the four corners of the line as an OCR record gives them (top-left,
    top-right, bottom-right, bottom-left as read) - instead of a rectangle.  images: a list of P contiguous uint8 CUDA [h_p][w_p][3] tensors
    on one device; quads: P lists of quads; frames: None or P lists of oriented crops (cx2, cy2, crop_scale, ux, uy), planned by
    prepost.plan_quads where not given (deterministic: nothing is drawn).  The mask is the quad itself, so the lines above and below a
    tilted line stay out of it; the crop is turned to the line's baseline, so the network sees the text upright, as its glyph image shows
    it; the paste maps page pixels back through the inverse of that frame and touches no pixel outside the quads.

    One preprocess_quads launch, the N rows (page-major) through edit_latents in chunks of `batch_size` exactly as edit_pages sends them
    (chunks cross page boundaries; every row starts from the seed-0 single-sample draw), one postprocess_quads launch.  Returns the list of
    P edited pages, with return_intermediate=True also image_vae [N,3,S,S] and the preprocess dict.  encoder_hidden_states / texts / glyph /
    enc_noise / variance_noise / cache_interval / guidance: as for edit_pages.

    perspective=True - for phone photos, signs and scene text, where a line is a trapezoid: frames are PROJECTIVE, (ci2, cj2, crop_scale),
    planned by prepost.plan_quads(..., perspective=True) where not given.  The crop is taken through the homography that makes the quad an
    upright rectangle, so the network sees the text without keystone, and the paste goes back through its inverse; everything between the
    two launches is the same.  Limits: the window is not moved to stay on the page (the border is replicated), a window over which the
    homography's denominator changes by more than 4x is refused; a line on an arc is edit_curved's.

    blend: None - the hard paste of the quad -, or a prepost.QuadBlend: the paste gets a feathered edge and / or a colour match of every
    patch against the page around it ([stats ->] blended paste on the device, prepost.postprocess_quads(blend=...)).  The ramp is measured
    perpendicular to the quad's edges in whole pixel steps, so it follows a tilted line or a trapezoid and survives a quarter turn of the
    page; with grow > 0 pixels outside the quad change, but none outside blend.grown(quads).  A PasteBlend - the box blend, whose ramp runs
    along the page's axes - raises NotImplementedError; anything else TypeError."""
    _check_quad_blend(blend, "edit_quads")
    perspective = bool(perspective)
    if int(batch_size) < 1:
        raise ValueError("batch_size must be at least 1")
    cache_interval = _check_cache_interval(cache_interval)
    images, quads, frames, sizes, N = _quad_lists(images, quads, frames)
    _check_contexts(N, encoder_hidden_states, texts, glyph)
    guidance = _check_guidance(guidance, encoder_hidden_states, N)
    if frames is None:
        frames = prepost.plan_quads(quads, sizes, perspective, int(size))
    encoder_hidden_states = _contexts(encoder_hidden_states, texts, glyph)
    pre = prepost.preprocess_quads(images, quads, frames, size=size, perspective=perspective)
    image_vae = _edit_rows(unet, vae, scheduler, pre, images[0].device, encoder_hidden_states, num_inference_steps, int(batch_size), generator,
                           enc_noise, variance_noise, int(size), cache_interval, guidance)
    out = prepost.postprocess_quads(image_vae, images, quads, frames, perspective=perspective, blend=blend)
    return (out, image_vae, pre) if return_intermediate else out


@torch.no_grad()
def edit_curved(unet, vae, scheduler, images, polygons, encoder_hidden_states, num_inference_steps, *, frames=None, batch_size=4, generator=None,
                enc_noise=None, variance_noise=None, return_intermediate=False, size=512, cache_interval=1, texts=None, glyph=None, guidance=None,
                blend=None):
    """edit_quads for CURVED text - signs, logos, seals, stamps, labels, arched shop fronts: every region is a polygon of 2n points,
    2 <= n <= 17, as scene-text OCR gives a curved line (the n top points left to right as read, then the n bottom points right to left).
    images: a list of P contiguous uint8 CUDA [h_p][w_p][3] tensors on one device; polygons: P lists of polygons; frames: None or P lists
    of (ci2, cj2, crop_scale) - a square window in the pixels of the polygon's straightened strip -, planned by prepost.plan_curved where
    not given (deterministic: nothing is drawn).  The polygon is cut into n - 1 quad cells and every cell into two triangles; each
    triangle goes to the strip by its own affine map, and neighbouring maps agree on the line they share.  So the mask is the polygon
    itself - what lies inside the arc's chord stays out of it -, the network sees the line STRAIGHT beside its upright glyph image, and
    the paste puts the result back BENT, without a tear, touching no pixel outside the polygons.

    One preprocess_curved launch, the N rows (page-major) through edit_latents in chunks of `batch_size` exactly as edit_pages sends them
    (chunks cross page boundaries; every row starts from the seed-0 single-sample draw), one postprocess_curved launch.  Returns the list
    of P edited pages, with return_intermediate=True also image_vae [N,3,S,S] and the preprocess dict.  encoder_hidden_states / texts /
    glyph / enc_noise / variance_noise / cache_interval / guidance: as for edit_pages.

    Limits: blend must be None (no blend for curved regions yet: anything else raises NotImplementedError); there is no
    edit_curved_verified (no fused read-back and select-paste; prepost.rectify_curved gives the straightened strips for an OCR pass of
    one's own); no fan cells - a point repeated on one side is refused -, and top and bottom carry the same number of points; the window
    is not moved to stay on the page (the border is replicated)."""
    if blend is not None:
        raise NotImplementedError("edit_curved: no blend for curved regions yet (blend must be None)")
    if int(batch_size) < 1:
        raise ValueError("batch_size must be at least 1")
    cache_interval = _check_cache_interval(cache_interval)
    images, polygons, frames, sizes, N = _quad_lists(images, polygons, frames)
    _check_contexts(N, encoder_hidden_states, texts, glyph)
    guidance = _check_guidance(guidance, encoder_hidden_states, N)
    if frames is None:
        frames = prepost.plan_curved(polygons, sizes, int(size))
    encoder_hidden_states = _contexts(encoder_hidden_states, texts, glyph)
    pre = prepost.preprocess_curved(images, polygons, frames, size=size)
    image_vae = _edit_rows(unet, vae, scheduler, pre, images[0].device, encoder_hidden_states, num_inference_steps, int(batch_size), generator,
                           enc_noise, variance_noise, int(size), cache_interval, guidance)
    out = prepost.postprocess_curved(image_vae, images, polygons, frames)
    return (out, image_vae, pre) if return_intermediate else out


def _check_quad_blend(blend, who):
    """the blend rule of the quad edits: None or a QuadBlend; a PasteBlend is the box blend"""
    if isinstance(blend, prepost.PasteBlend):
        raise NotImplementedError(f"{who}: a PasteBlend is not supported for quads (its ramp is measured along the page's axes); pass a QuadBlend or None")
    if blend is not None and not isinstance(blend, prepost.QuadBlend):
        raise TypeError(f"{who}: blend: expected a QuadBlend or None, got {type(blend).__name__}")


def _quad_lists(images, quads, frames):
    """the list arguments of the quad edit functions, checked: P pages, P lists of quads, frames None or P lists of one frame per quad.
    Returns (images, quads, frames, sizes, N)."""
    images, quads = list(images), [list(q) for q in quads]
    if len(quads) != len(images):
        raise ValueError(f"{len(images)} pages, {len(quads)} lists of quads: the lengths must agree")
    sizes = [_page_size(img, f"images[{p}]") for p, img in enumerate(images)]
    if frames is not None:
        frames = [list(f) for f in frames]
        if len(frames) != len(images) or any(len(f) != len(q) for f, q in zip(frames, quads)):
            raise ValueError(f"frames must be {len(images)} lists, one frame per quad: the lengths must agree")
    return images, quads, frames, sizes, sum(len(q) for q in quads)


def _check_blend(blend):
    if blend is not None and not isinstance(blend, prepost.PasteBlend):
        raise TypeError(f"blend: expected a PasteBlend or None, got {type(blend).__name__}")


def _one(lst):
    """a one-page function's optional list as the paged form's list of lists"""
    return None if lst is None else [lst]


def _page_size(image, name):
    """(h, w) of one page; only that it is a 3-d tensor is asked here - dtype, device and layout are prepost's to check"""
    if not isinstance(image, torch.Tensor) or image.dim() != 3:
        raise TypeError(f"{name}: expected a contiguous uint8 CUDA tensor [h][w][3]")
    return int(image.shape[0]), int(image.shape[1])


def _plan_boxes(locations, h, w, origins, crop_scales, rng):
    """crop_scales / origins of the boxes of one h x w page where they are not given: the reference's ladder and origin rule, random
    origins drawn from `rng` (default numpy's global state) in box order.  Returns (crop_scales, origins)."""
    N = len(locations)
    if crop_scales is None:
        crop_scales = [prepost.crop_scale_for(loc, h, w) for loc in locations]
    crop_scales = list(crop_scales)
    if origins is None:
        if len(crop_scales) != N:
            raise ValueError(f"{N} boxes, {len(crop_scales)} crop scales: the lengths must agree")
        origins = [prepost.crop_origin(loc, cs, w, rng if rng is not None else np.random) for loc, cs in zip(locations, crop_scales)]
    return crop_scales, origins


def _check_contexts(N, encoder_hidden_states, texts=None, glyph=None):
    """the context arguments of the four edit functions: exactly one of encoder_hidden_states [N,L,D] and texts (N strings, which need
    glyph = (renderer, processor, encoder)).  Host work only - a text the atlas cannot lay out raises here, before anything is launched."""
    if (encoder_hidden_states is None) == (texts is None):
        raise ValueError("exactly one of encoder_hidden_states and texts must be given")
    if texts is None:
        if encoder_hidden_states.shape[0] != N:
            raise ValueError(f"{N} boxes but {encoder_hidden_states.shape[0]} glyph contexts")
        return
    if glyph is None:
        raise ValueError("texts needs glyph=(renderer, processor, encoder)")
    if not isinstance(glyph, (tuple, list)) or len(glyph) != 3 or not isinstance(getattr(glyph[0], "atlas", None), glyphs.GlyphAtlas):
        raise ValueError("glyph must be a (renderer, processor, encoder) triple: a GlyphRenderer, a TrOCRProcessor, a TrOCREncoder")
    if isinstance(texts, str) or len(texts) != N:
        raise ValueError(f"{N} boxes but " + ("one str, not a list of texts" if isinstance(texts, str) else f"{len(texts)} texts"))
    glyphs.layout(glyph[0].atlas, texts)


def _contexts(encoder_hidden_states, texts, glyph):
    """what _check_contexts passed -> the contexts [N,L,D]"""
    return encoder_hidden_states if texts is None else glyphs.glyph_contexts(list(texts), *glyph)


def _page_lists(paged, images, locations, origins, crop_scales):
    """the list arguments of the four edit functions, checked: P pages, P lists of boxes, origins / crop_scales None or P lists whose
    entries are None or as long as the page's boxes.  Nothing is planned here, so nothing is drawn.  Returns (images, locations, origins,
    crop_scales, sizes, N) with P lists each.  A one-page call (paged=False) is named by its own argument, not as page 0."""
    images, locations = list(images), [list(l) for l in locations]
    P = len(images)
    if len(locations) != P:
        raise ValueError(f"{P} pages, {len(locations)} lists of boxes: the lengths must agree")
    both = []
    for name, lst in (("origins", origins), ("crop_scales", crop_scales)):
        lst = [None] * P if lst is None else [None if l is None else list(l) for l in lst]      # materialised once: a generator would not
        if len(lst) != P:                                                                       # survive the length checks
            raise ValueError(f"{P} pages, {len(lst)} lists of {name}: the lengths must agree")
        both.append(lst)
    sizes = [_page_size(img, f"images[{p}]" if paged else "instance_image") for p, img in enumerate(images)]
    for p, locs in enumerate(locations):
        for name, lst in (("origins", both[0][p]), ("crop_scales", both[1][p])):
            if lst is not None and len(lst) != len(locs):
                raise ValueError((f"page {p}: " if paged else "") + f"{len(locs)} boxes, {len(lst)} {name}: the lengths must agree")
    return images, locations, both[0], both[1], sizes, sum(len(l) for l in locations)


def _plan_pages(paged, images, locations, sizes, origins, crop_scales, rng):
    """the crops that _page_lists left open, planned page after page on one rng stream (prepost.plan_pages' draws) -> the leading
    arguments of the prepost functions of the caller's form: (images, locations, origins, crop_scales), of the one page if not paged"""
    for p, (h, w) in enumerate(sizes):
        crop_scales[p], origins[p] = _plan_boxes(locations[p], h, w, origins[p], crop_scales[p], rng)
    return (images, locations, origins, crop_scales) if paged else (images[0], locations[0], origins[0], crop_scales[0])


@torch.no_grad()
def _edit_rows(unet, vae, scheduler, pre, dev, encoder_hidden_states, num_inference_steps, bs, generator, enc_noise, variance_noise, S,
               cache_interval=1, guidance=None):
    """the model part of edit_boxes / edit_pages: the N rows of the preprocess dict `pre` through edit_latents in chunks of `bs` (the last
    chunk may be smaller) -> image_vae [N,3,S,S].  A row's page plays no part here."""
    N = pre["image"].shape[0]
    f = 2 ** (len(vae.config.block_out_channels) - 1)
    # app.ipynb:796-801: ONE seed-0 draw of a single sample, shared by every box
    init = torch.randn((1, vae.config.latent_channels, S // f, S // f), generator=torch.manual_seed(0), dtype=torch.float32).to(dev)
    outs = []
    for lo in range(0, N, bs):
        hi = min(N, lo + bs)
        outs.append(edit_latents(unet, vae, scheduler, pre["image"][lo:hi], pre["masked_image"][lo:hi], pre["mask"][lo:hi],
                                 encoder_hidden_states[lo:hi], num_inference_steps,
                                 init_latents=init.expand(hi - lo, -1, -1, -1).contiguous(), generator=generator,
                                 enc_noise=None if enc_noise is None else enc_noise[lo:hi],
                                 variance_noise=None if variance_noise is None else variance_noise[:, lo:hi], cache_interval=cache_interval,
                                 guidance=None if guidance is None else guidance.rows(slice(lo, hi))))
    return outs[0] if len(outs) == 1 else torch.cat(outs, 0)


class VerifiedEdit:
    """what edit_boxes_verified(return_intermediate=True) returns: image uint8 [h][w][3] (edit_pages_verified: the list of P pages); choice
    int32 [N] (the pasted candidate of each box, -1 = kept the original); scores fp32 [N,K] (mean log-probability per label token);
    image_vae fp32 [N,K,3,S,S]; pixel_values fp32 [N*K,3,S_h,S_w] (what the OCR model read, box-major); pre (the preprocess_batch dict).
    All on the device."""

    def __init__(self, image, choice, scores, image_vae, pixel_values, pre):
        self.image, self.choice, self.scores, self.image_vae, self.pixel_values, self.pre = image, choice, scores, image_vae, pixel_values, pre


def _check_verified_counts(N, candidates, seeds, min_score, batch_size, ocr_batch_size):
    """-> (K, seeds)"""
    if N < 1 or N > _cabi.EDIT_MAX_ITEMS:
        raise ValueError(f"{N} boxes, expected 1 .. {_cabi.EDIT_MAX_ITEMS}")
    if int(batch_size) < 1 or int(ocr_batch_size) < 1:
        raise ValueError("batch_size and ocr_batch_size must be at least 1")
    K = int(candidates)
    if not 1 <= K <= _cabi.SELECT_MAX_CANDIDATES:
        raise ValueError(f"candidates = {K}, expected 1 .. {_cabi.SELECT_MAX_CANDIDATES}")
    seeds = list(range(K)) if seeds is None else [int(s) for s in seeds]
    if len(seeds) != K:
        raise ValueError(f"{K} candidates but {len(seeds)} seeds")
    if min_score is not None and float(min_score) != float(min_score):
        raise ValueError("min_score is NaN")
    return K, seeds


def _check_verified_labels(ocr, N, encoder_hidden_states, labels, texts=None, glyph=None):
    _check_contexts(N, encoder_hidden_states, texts, glyph)
    if not torch.is_tensor(labels) or labels.dtype != torch.int64:
        raise ValueError(f"labels must be an int64 tensor, got {getattr(labels, 'dtype', type(labels))}")
    if labels.ndim != 2 or labels.shape[0] != N or labels.shape[1] < 1:
        raise ValueError(f"labels must be [N, T] with N = {N} and T >= 1, got {tuple(labels.shape)}")
    V, P = ocr.decoder.config.vocab_size, ocr.decoder.config.max_position_embeddings
    if labels.shape[1] > P:
        raise ValueError(f"labels have T = {labels.shape[1]} positions, the decoder {P}")
    if not labels.is_cuda and bool((((labels < 0) | (labels >= V)) & (labels != -100)).any()):      # (labels on the device: ocr.score checks them)
        raise ValueError(f"labels must lie in [0, {V}) or equal -100")


def _check_verified_processor(ocr, processor, size):
    """-> the image processor"""
    ip = getattr(processor, "image_processor", processor)
    if not getattr(ip, "do_resize", False):
        raise ValueError("the processor must resize (do_resize=True)")
    want = int(ocr.encoder.config.image_size)
    if (ip.size["height"], ip.size["width"]) != (want, want):
        raise ValueError(f"the processor resizes to {ip.size['width']}x{ip.size['height']}, ocr.encoder reads {want}x{want}")
    if int(size) < 8 or int(size) % 8:
        raise ValueError(f"size = {size} is no positive multiple of 8")
    return ip


@torch.no_grad()
def _candidate_rows(unet, vae, scheduler, pre, dev, ctx, num_inference_steps, seeds, bs, generator, enc_noise, variance_noise, S,
                    cache_interval=1, guidance=None):
    """the generating half of the verified edits, after the preprocess: the N rows of the preprocess dict `pre`, whatever pages they come
    from -> image_vae [N,K,3,S,S].  Each box is VAE-encoded once; the N*K rows (box-major, candidate k from seeds[k]) go through denoise +
    vae.decode in chunks of `bs`.  With one seed this is _edit_rows' loop, chunk for chunk."""
    N, K = pre["image"].shape[0], len(seeds)
    sf = vae.config.scaling_factor
    f = 2 ** (len(vae.config.block_out_channels) - 1)
    init = torch.cat([torch.randn((1, vae.config.latent_channels, S // f, S // f), generator=torch.manual_seed(s), dtype=torch.float32)
                      for s in seeds], 0).to(dev)                                          # [K,4,h,w]; app.ipynb:796-801 for seed 0
    mask_lat = mask_to_latent(pre["mask"], f)
    mlat = [None] * N                        # box b's masked-image latents: encoded when the first chunk that holds one of its rows comes up
    outs = []
    for lo in range(0, N * K, bs):
        hi = min(N * K, lo + bs)
        b0, b1 = lo // K, (hi - 1) // K + 1
        new = [b for b in range(b0, b1) if mlat[b] is None]
        if new:                              # (consecutive boxes; with K = 1 exactly the chunk's boxes: edit_boxes' encode)
            dist = vae.encode(pre["masked_image"][new[0]:new[-1] + 1]).latent_dist
            z = (dist.sample(noise=enc_noise[new[0]:new[-1] + 1]) if enc_noise is not None else dist.sample(generator=generator)) * sf
            for j, b in enumerate(new):
                mlat[b] = z[j:j + 1]
        rows = torch.arange(lo, hi)
        box = (rows // K).tolist()
        lat = denoise(unet, scheduler, init[(rows % K).to(dev)].contiguous(), mask_lat[box], torch.cat([mlat[b] for b in box], 0), ctx[box],
                      num_inference_steps, variance_noise=None if variance_noise is None else variance_noise[:, lo:hi],
                      cache_interval=cache_interval, guidance=None if guidance is None else guidance.rows(box))
        outs.append(vae.decode(lat / sf).sample)
        for b in range(b0, b1):
            if (b + 1) * K <= hi:
                mlat[b] = False              # all K rows done: the latents are released (and never encoded again)
    return (outs[0] if len(outs) == 1 else torch.cat(outs, 0)).reshape(N, K, 3, S, S)


@torch.no_grad()
def edit_boxes_verified(unet, vae, scheduler, ocr, processor, instance_image, locations, encoder_hidden_states, labels, num_inference_steps, *,
                        candidates=4, seeds=None, min_score=None, batch_size=4, ocr_batch_size=32, origins=None, crop_scales=None, rng=None,
                        generator=None, enc_noise=None, variance_noise=None, size=512, return_intermediate=False, cache_interval=1, texts=None,
                        glyph=None, guidance=None, blend=None):
    """edit_boxes with a read-back: K = `candidates` edits per box from K starting noises, each read by the OCR model `ocr` (a
    VisionEncoderDecoderModel) against the text the box should show, the best-reading one pasted (the reference sketches the read-back at
    app.ipynb:842-846).  labels: int64 [N,T] token ids of the requested texts, -100 = padding (the tokenizer is out of scope).

    Candidate k of every box starts from `torch.randn((1,4,h,w), generator=torch.manual_seed(seeds[k]))` on the CPU, seeds = range(K) by
    default, so candidate 0 is edit_boxes' (the reference's) start.  The masked crop of a box is VAE-encoded and its posterior sampled
    ONCE (enc_noise [N,4,h,w] injects the draw) and shared by the box's K candidates, as is its glyph context.  The N*K rows, box-major,
    go through denoise + vae.decode in chunks of `batch_size` (variance_noise, if given, is [steps, N*K, 4, h, w] in that order), through
    prepost.readback_pixel_values in one launch and through ocr.score in chunks of `ocr_batch_size`; a candidate's score is the mean
    log-probability of its label tokens, sequence_logprobs / num_tokens.clamp(min=1).  prepost.postprocess_select_batch picks and pastes
    on the device: no score is read on the host.  min_score: a box whose best candidate scores below it keeps the original pixels.

    Returns the uint8 [h][w][3] page, or a VerifiedEdit with return_intermediate=True.  candidates=1 with min_score=None returns the
    page of edit_boxes with the same arguments, bit for bit.  cache_interval: denoise's, for every chunk of candidate rows.
    texts / glyph: as for edit_boxes, in place of encoder_hidden_states (labels stay token ids: the tokenizer is out of scope).
    guidance: as for edit_boxes; a per-box uncond [N,S,D] is shared by the box's K candidates, like its glyph context.
    blend: as for edit_boxes, applied to the chosen candidates (choose -> [stats ->] paste on the device, still no score read on the host).
    The read-back scores the candidates as the hard paste would show them."""
    return _edit_verified(_BoxRegions(False, [instance_image], [locations], _one(origins), _one(crop_scales), rng), unet, vae, scheduler, ocr,
                          processor, encoder_hidden_states, labels, num_inference_steps, candidates, seeds, min_score, batch_size, ocr_batch_size,
                          generator, enc_noise, variance_noise, size, return_intermediate, cache_interval, texts, glyph, guidance, blend)


@torch.no_grad()
def edit_pages_verified(unet, vae, scheduler, ocr, processor, images, locations, encoder_hidden_states, labels, num_inference_steps, *,
                        candidates=4, seeds=None, min_score=None, batch_size=4, ocr_batch_size=32, origins=None, crop_scales=None, rng=None,
                        generator=None, enc_noise=None, variance_noise=None, size=512, return_intermediate=False, cache_interval=1, texts=None,
                        glyph=None, guidance=None, blend=None):
    """edit_boxes_verified for boxes on several pages: images / locations / origins / crop_scales as for edit_pages, everything per box
    (encoder_hidden_states [N,L,D], labels [N,T], enc_noise [N,4,h,w]) page-major.  The N*K rows go through edit_boxes_verified's chunk
    loop, prepost.readback_pixel_values_pages, ocr.score and prepost.postprocess_select_pages - chunks cross page boundaries, no score is
    read on the host.  Returns the list of P pages, or a VerifiedEdit whose `image` is that list with return_intermediate=True.
    candidates=1 with min_score=None returns edit_pages' pages, bit for bit.  texts / glyph, guidance: as for edit_boxes, page-major.
    blend: as for edit_boxes_verified."""
    return _edit_verified(_BoxRegions(True, images, locations, origins, crop_scales, rng), unet, vae, scheduler, ocr, processor,
                          encoder_hidden_states, labels, num_inference_steps, candidates, seeds, min_score, batch_size, ocr_batch_size, generator,
                          enc_noise, variance_noise, size, return_intermediate, cache_interval, texts, glyph, guidance, blend)


class _BoxRegions:
    """the regions of edit_boxes_verified (paged=False: one page, its lists wrapped into one-element lists) and edit_pages_verified, as
    _edit_verified sees them: lists checked at construction, N, then the stages in the order it calls them"""

    def __init__(self, paged, images, locations, origins, crop_scales, rng):
        self.paged, self.rng = paged, rng
        self.images, self.locations, self.origins, self.crop_scales, self.sizes, self.N = _page_lists(paged, images, locations, origins, crop_scales)

    def check_blend(self, blend):
        _check_blend(blend)

    def check_readback(self):
        if self.paged:
            prepost.check_readback_boxes_pages([loc for l in self.locations for loc in l], [len(l) for l in self.locations], self.sizes)
        else:
            prepost.check_readback_boxes(self.locations[0], *self.sizes[0])

    def plan(self, size):
        self.where = _plan_pages(self.paged, self.images, self.locations, self.sizes, self.origins, self.crop_scales, self.rng)

    def preprocess(self, size):
        return (prepost.preprocess_pages if self.paged else prepost.preprocess_batch)(*self.where, size=size)

    def readback(self, image_vae, ip):
        return (prepost.readback_pixel_values_pages if self.paged else prepost.readback_pixel_values)(image_vae, *self.where, ip)

    def select_paste(self, image_vae, scores, min_score, blend):
        return (prepost.postprocess_select_pages if self.paged else prepost.postprocess_select_batch)(image_vae, scores, *self.where,
                                                                                                       threshold=min_score, blend=blend)


class _QuadRegions:
    """the regions of edit_quads_verified: quads on several pages, frames given or planned (deterministic: nothing is drawn)"""

    def __init__(self, images, quads, frames, perspective):
        self.images, self.quads, self.frames, self.sizes, self.N = _quad_lists(images, quads, frames)
        self.perspective = bool(perspective)

    def check_blend(self, blend):
        _check_quad_blend(blend, "edit_quads_verified")

    def check_readback(self):
        pass                                                           # (a prepared quad has a strip of at least one pixel)

    def plan(self, size):
        if self.frames is None:
            self.frames = prepost.plan_quads(self.quads, self.sizes, self.perspective, size)

    def preprocess(self, size):
        return prepost.preprocess_quads(self.images, self.quads, self.frames, size=size, perspective=self.perspective)

    def readback(self, image_vae, ip):
        return prepost.readback_pixel_values_quads(image_vae, self.images, self.quads, self.frames, ip, perspective=self.perspective)

    def select_paste(self, image_vae, scores, min_score, blend):
        return prepost.postprocess_select_quads(image_vae, scores, self.images, self.quads, self.frames, threshold=min_score,
                                                perspective=self.perspective, blend=blend)


def _edit_verified(regions, unet, vae, scheduler, ocr, processor, encoder_hidden_states, labels, num_inference_steps, candidates, seeds, min_score,
                   batch_size, ocr_batch_size, generator, enc_noise, variance_noise, size, return_intermediate, cache_interval=1, texts=None,
                   glyph=None, guidance=None, blend=None):
    """the verified edits of every region kind - `regions` is a _BoxRegions or a _QuadRegions, whose construction has checked the list
    arguments.  Every argument is checked on the host side first: nothing touches the GPU and no crop is planned - so nothing is drawn from
    rng - before all have passed."""
    N = regions.N
    K, seeds = _check_verified_counts(N, candidates, seeds, min_score, batch_size, ocr_batch_size)
    regions.check_blend(blend)
    cache_interval = _check_cache_interval(cache_interval)
    _check_verified_labels(ocr, N, encoder_hidden_states, labels, texts, glyph)
    guidance = _check_guidance(guidance, encoder_hidden_states, N)
    regions.check_readback()
    ip = _check_verified_processor(ocr, processor, size)
    regions.plan(int(size))
    encoder_hidden_states = _contexts(encoder_hidden_states, texts, glyph)
    pre = regions.preprocess(int(size))
    image_vae = _candidate_rows(unet, vae, scheduler, pre, regions.images[0].device, encoder_hidden_states, num_inference_steps, seeds,
                                int(batch_size), generator, enc_noise, variance_noise, int(size), cache_interval, guidance)
    pixel_values = regions.readback(image_vae, ip)
    scores = _score_candidates(ocr, pixel_values, labels, N, K, int(ocr_batch_size))
    out, choice = regions.select_paste(image_vae, scores, min_score, blend)
    return VerifiedEdit(out, choice, scores, image_vae, pixel_values, pre) if return_intermediate else out


@torch.no_grad()
def edit_quads_verified(unet, vae, scheduler, ocr, processor, images, quads, encoder_hidden_states, labels, num_inference_steps, *, frames=None,
                        candidates=4, seeds=None, min_score=None, batch_size=4, ocr_batch_size=32, generator=None, enc_noise=None,
                        variance_noise=None, size=512, return_intermediate=False, cache_interval=1, texts=None, glyph=None, guidance=None,
                        perspective=False, blend=None):
    """edit_quads with edit_pages_verified's read-back - for skewed lines, scene text and phone photos, where a single sample most often
    reads wrong: K = `candidates` edits per quad, each read by the OCR model as its upright strip, the best-reading one pasted through the
    quad's frame.  images / quads / frames / perspective: as for edit_quads; everything per quad (encoder_hidden_states [N,L,D], labels
    [N,T], enc_noise [N,4,h,w]) page-major; candidates / seeds / min_score / batch_size / ocr_batch_size and the chunking of the N*K rows:
    as for edit_boxes_verified.

    One preprocess_quads launch, the N*K rows through edit_boxes_verified's chunk loop, prepost.readback_pixel_values_quads in one launch -
    row (b, k) is what the processor makes of rectify_quads of the page with candidate k of quad b ALONE pasted on it -, ocr.score, and
    prepost.postprocess_select_quads: no score is read on the host.  A quad whose best candidate scores below min_score keeps the original
    pixels and is transparent: an earlier chosen quad under it still shows.

    Returns the list of P pages, or a VerifiedEdit whose `image` is that list with return_intermediate=True.  candidates=1 with
    min_score=None returns edit_quads' pages, bit for bit.  blend: as for edit_quads, applied to the chosen candidates (choose -> [stats ->]
    blended paste on the device, still no score read on the host).  The read-back keeps scoring every candidate as the HARD paste shows
    it - candidate k of quad b pasted alone, without feather, grow or colour match -: the blend changes how the chosen candidate is put on
    the page, not which one is chosen."""
    return _edit_verified(_QuadRegions(images, quads, frames, perspective), unet, vae, scheduler, ocr, processor, encoder_hidden_states, labels,
                          num_inference_steps, candidates, seeds, min_score, batch_size, ocr_batch_size, generator, enc_noise, variance_noise, size,
                          return_intermediate, cache_interval, texts, glyph, guidance, blend)


def _score_candidates(ocr, pixel_values, labels, N, K, ocr_bs):
    """scores fp32 [N,K] on the device: ocr.score over the N*K read-back rows in chunks of `ocr_bs`, mean log-probability per label token"""
    lab = labels.to(pixel_values.device).repeat_interleave(K, 0)
    seq, num = [], []
    for lo in range(0, N * K, ocr_bs):
        r = ocr.score(pixel_values[lo:lo + ocr_bs], labels=lab[lo:lo + ocr_bs])
        seq.append(r.sequence_logprobs); num.append(r.num_tokens)
    return (torch.cat(seq) / torch.cat(num).clamp(min=1)).reshape(N, K)
