"""The fused OCR read-back kernel (csrc/readback.hip dmx_readback_pixel_values through prepost.readback_pixel_values): K = 3 candidates
of B = 4 boxes per launch, bit for bit against the chain it replaces - postprocess (the single-box paste kernel) over the ORIGINAL page,
the slice [y1:y2, x1:x2], ViTImageProcessor on the slice - for the fp32 pixel_values and the uint8 bytes before normalisation, and against
the numpy restatement of that chain (tests/readback_restatement.py, pinned against Pillow in tests/test_readback_host.py).  The cases
(identity / enlarged / shrunk / border-clipped / exact-2x crops, a box wider than its crop, skipped passes, a 1-pixel-high box, many
taps, both filters, 32 x 32 and 384 x 384 outputs) are listed there.  Outputs go into sentinel-filled buffers with guard bands."""
import ctypes

import numpy as np
import pytest
import torch

import readback_restatement as RB

pytestmark = pytest.mark.gpu

GUARD = 4096
F32_SENTINEL = 12345.0              # pixel_values lie in [-1, 1]


@pytest.fixture(scope="module")
def img(cuda):
    return torch.from_numpy(RB.page()).to(cuda)


def _guarded(n, dtype, fill, dev):
    buf = torch.full((n + 2 * GUARD,), fill, dtype=dtype, device=dev)
    return buf, buf[GUARD:GUARD + n]


def _chain(D, vae, img, items, size, resample):
    """what the fused kernel replaces, from existing functions: B * K pastes, a slice each, one processor call over the slices"""
    ip = D.ViTImageProcessor(size=size, resample=resample)
    slices = []
    for b, (box, (x_s, y_s), crop) in enumerate(items):
        x1, y1, x2, y2 = box
        for k in range(vae.shape[1]):
            slices.append(D.prepost.postprocess(vae[b, k], img, box, x_s, y_s, crop)[y1:y2, x1:x2])
    got = ip(images=slices, return_resized=True)
    return got.pixel_values, got["resized"]


@pytest.mark.parametrize("case", RB.CASES, ids=RB.CASE_IDS)
def test_readback_equals_paste_slice_processor(cuda, img, case):
    import diffute_amd as D
    _, names, resample, size = case
    items = [RB.ITEMS[n] for n in names]
    vae_np = RB.decoder_outputs(names)
    vae = torch.from_numpy(vae_np).to(cuda)
    assert float(vae.min()) < -1.1 and float(vae.max()) > 1.1
    want_pv, want_u8 = _chain(D, vae, img, items, size, resample)
    boxes, origins, crops = [i[0] for i in items], [i[1] for i in items], [i[2] for i in items]
    ip = D.TrOCRProcessor(size=size, resample=resample)
    n = len(items) * RB.K * 3 * size * size
    for fill in (0, 255):                                  # a byte nobody wrote shows under one fill or the other
        fbuf, fout = _guarded(n, torch.float32, F32_SENTINEL, cuda)
        ubuf, uout = _guarded(n, torch.uint8, fill, cuda)
        shape = (len(items) * RB.K, 3, size, size)
        pv, u8 = D.prepost.readback_pixel_values(vae, img, boxes, origins, crops, ip, out=fout.view(shape), out_resized=uout.view(shape))
        D.synchronize()
        assert pv.data_ptr() == fout.data_ptr() and u8.data_ptr() == uout.data_ptr()
        assert bool((pv != F32_SENTINEL).all()), "an element of pixel_values was not written"
        assert torch.equal(u8, want_u8), "resized bytes differ from paste -> slice -> processor"
        assert torch.equal(pv, want_pv), "pixel_values differ from paste -> slice -> processor"
        for buf, f in ((fbuf, F32_SENTINEL), (ubuf, fill)):
            assert bool((buf[:GUARD] == f).all()) and bool((buf[-GUARD:] == f).all()), "a guard band was written"
    # without the optional outputs: the same values in tensors of its own
    assert torch.equal(D.prepost.readback_pixel_values(vae, img, boxes, origins, crops, ip), want_pv)
    # the CPU anchor: the numpy chain, one candidate of every box (every candidate where that is cheap)
    pv_h, u8_h = pv.cpu().numpy(), u8.cpu().numpy()
    for b in range(len(items)):
        for k in (range(RB.K) if size == 32 else (b % RB.K,)):
            r_u8, r_pv = RB.readback(vae_np[b, k], RB.page(), items[b], size, resample)
            assert np.array_equal(u8_h[b * RB.K + k], r_u8) and np.array_equal(pv_h[b * RB.K + k].view(np.uint32), r_pv.view(np.uint32)), (names[b], k)


def test_candidates_of_one_box_and_k1(cuda, img):
    """K = 1 (the shape edit_boxes_verified(candidates=1) launches) and K = 16, the cap: row (b, k) depends on image_vae[b, k] alone"""
    import diffute_amd as D
    items = [RB.ITEMS[n] for n in RB.SET_A]
    boxes, origins, crops = [i[0] for i in items], [i[1] for i in items], [i[2] for i in items]
    vae = torch.from_numpy(RB.decoder_outputs(RB.SET_A)).to(cuda)
    ip = D.TrOCRProcessor(size=32)
    full = D.prepost.readback_pixel_values(vae, img, boxes, origins, crops, ip).reshape(4, RB.K, 3, 32, 32)
    for k in range(RB.K):
        one = D.prepost.readback_pixel_values(vae[:, k:k + 1], img, boxes, origins, crops, ip)
        assert torch.equal(one, full[:, k])
    wide = vae.repeat(1, 6, 1, 1, 1)[:, :16].contiguous()
    got = D.prepost.readback_pixel_values(wide, img, boxes, origins, crops, ip).reshape(4, 16, 3, 32, 32)
    D.synchronize()
    assert all(torch.equal(got[:, k], full[:, k % RB.K]) for k in range(16))
    assert not torch.equal(full[:, 0], full[:, 1])
    with pytest.raises(ValueError):
        D.prepost.readback_pixel_values(vae.repeat(1, 6, 1, 1, 1)[:, :17].contiguous(), img, boxes, origins, crops, ip)


def test_refusals_launch_nothing(cuda, img):
    """every refused argument returns DMX_ERR_ARG and leaves the sentinel-filled outputs as they were"""
    from diffute_amd import _cabi
    lib = _cabi.lib()
    items = [RB.ITEMS[n] for n in RB.SET_A]
    vae = torch.from_numpy(RB.decoder_outputs(RB.SET_A)).to(cuda)
    n = 4 * RB.K * 3 * 32 * 32
    out = torch.full((n,), F32_SENTINEL, dtype=torch.float32, device=cuda)
    u8 = torch.full((n,), 0x5A, dtype=torch.uint8, device=cuda)

    def call(spoil=None, K=RB.K, max_taps=None, short=0):
        arr, pa, tables, norm, taps = RB.entry_tables(items, 32, RB.BILINEAR)
        d_items = torch.from_numpy(np.frombuffer(bytes(arr), dtype=np.uint8).copy()).to(cuda)      # the device copies stay good: only the
        d_pass = torch.from_numpy(np.frombuffer(bytes(pa), dtype=np.uint8).copy()).to(cuda)        # host tables are spoiled below
        d_tab, d_norm = torch.from_numpy(tables.copy()).to(cuda), torch.from_numpy(norm.copy()).to(cuda)
        if spoil:
            spoil(arr, pa)
        rc = lib.dmx_readback_pixel_values(_cabi.ptr(vae), RB.S, _cabi.ptr(img), RB.H, RB.W, arr, _cabi.ptr(d_items), 4, K, _cabi.ptr(d_tab),
                                           tables.size - short, _cabi.ptr(d_norm), pa, _cabi.ptr(d_pass), taps if max_taps is None else max_taps,
                                           32, 32, _cabi.ptr(out), _cabi.ptr(u8), _cabi.current_stream())
        _cabi.synchronize()
        return rc

    def box(b, *v):
        def f(arr, pa):
            arr[b].x1, arr[b].y1, arr[b].x2, arr[b].y2 = v
        return f
    bad = [dict(K=0), dict(K=17), dict(max_taps=65), dict(short=1), dict(spoil=box(1, 200, 150, 200, 180)), dict(spoil=box(1, 200, 180, 330, 180)),
           dict(spoil=box(3, 310, 260, 385, 280)), dict(spoil=box(0, 40, 60, 150, 321)), dict(spoil=box(0, -1, 60, 150, 78))]
    for kw in bad:
        assert call(**kw) == -1, kw
        assert bool((out == F32_SENTINEL).all()) and bool((u8 == 0x5A).all()), f"{kw}: refused, yet something was written"
    assert call() == 0                                      # the same call unspoiled is accepted and writes everything
    assert bool((out != F32_SENTINEL).all())
