"""diffute_amd.metrics on the GPU (csrc/metrics.hip) against the numpy restatement (metrics_restatement.py) on the cases of metrics_cases.py,
in both builds of the library.  The integer outputs - sse, n, changed_outside, sse_outside - are bit-exact; ssim_rgb is within
4 x floor + 2^-22 of the float64 restatement per box and channel, floor being the recorded error of the fp32 formulation
(metrics_floors.py, pinned by test_metrics_host.py); too-small boxes give NaN, identical inputs exactly 1.0.  A box's row is bit-equal
alone and in the batch, through the one-page and the paged function, from run to run and between the builds.  Every kernel output goes
into a sentinel-filled buffer whose guard bands must survive; refused calls leave it untouched."""
import numpy as np
import pytest
import torch

import metrics_cases as C
import metrics_restatement as M
from metrics_floors import FLOORS

pytestmark = pytest.mark.gpu

CASE_IDS = [c[0] for c in C.CASES]
SENTINEL = {torch.int64: 0x7A5A5A5A5A5A5A5A, torch.float32: 0x7A5A5A5A}
PAD = 16


def _guarded(shape, dtype, dev):
    """(buffer, contiguous view of `shape` in its middle): all of it sentinel, PAD elements of guard band either side"""
    it = torch.int64 if dtype == torch.int64 else torch.int32
    n = int(np.prod(shape))
    buf = torch.full((n + 2 * PAD,), SENTINEL[dtype], dtype=it, device=dev).view(dtype)
    return buf, buf[PAD:PAD + n].view(shape)


def _guard_intact(buf, written, name):
    it = torch.int64 if buf.dtype == torch.int64 else torch.int32
    raw = buf.view(it).cpu()
    s = SENTINEL[buf.dtype]
    assert (raw[:PAD] == s).all() and (raw[-PAD:] == s).all(), f"{name}: a guard band was overwritten"
    inside = raw[PAD:-PAD] == s
    assert (not inside.any()) if written else inside.all(), f"{name}: {'unwritten outputs' if written else 'a refused call wrote outputs'}"


def _bits(t):
    return t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int64).cpu()


@pytest.fixture(scope="module")
def refs():
    """per case: the pages and, per box, the float64 restatement; per page the outside diff - computed once, only read"""
    out = {}
    for name, content, geometry in C.CASES:
        A, B = C.pages(content)
        rows = [M.ref64(A[p], B[p], bx) for p, bx in C.flat_boxes(geometry)]
        out[name] = dict(A=A, B=B, boxes=C.GEOMETRY[geometry], rows=rows, outside=[M.outside_ref(A[p], B[p], C.GEOMETRY[geometry][p]) for p in range(len(A))])
    return out


@pytest.fixture(scope="module")
def dev_pages(cuda):
    out = {}
    for content in C.CONTENTS:
        A, B = C.pages(content)
        out[content] = ([torch.from_numpy(a).to(cuda) for a in A], [torch.from_numpy(b).to(cuda) for b in B])
    return out


def _tables(dev_pages, content, boxes):
    from diffute_amd import metrics
    a, b, flat, counts, dev = metrics._check_pairs(*dev_pages[content], boxes)
    return metrics._upload(a, b, flat, counts, dev)


def _run_raw(t, elem):
    """both kernels' outputs for the tables t from the given build, through guarded buffers -> (sse, ssim, outside) on the host"""
    from diffute_amd import _cabi, metrics
    lib = _cabi.lib(elem)
    bs, sse = _guarded((t.B, 3), torch.int64, t.dev)
    bf, ssim = _guarded((t.B, 3), torch.float32, t.dev)
    bo, out = _guarded((t.P, 2), torch.int64, t.dev)
    metrics._box_metrics_raw(t, sse, ssim, lib)
    metrics._outside_diff_raw(t, out, lib)
    _cabi.synchronize()
    for buf, name in ((bs, "sse"), (bf, "ssim"), (bo, "outside")):
        _guard_intact(buf, True, name)
    return sse.cpu(), ssim.cpu(), out.cpu()


@pytest.mark.parametrize("elem", ["bf16", "fp16"])
@pytest.mark.parametrize("name,content,geometry", C.CASES, ids=CASE_IDS)
def test_kernels_against_the_restatement(cuda, refs, dev_pages, name, content, geometry, elem):
    r = refs[name]
    sse, ssim, outside = _run_raw(_tables(dev_pages, content, r["boxes"]), elem)
    want_sse = np.array([row["sse"] for row in r["rows"]], dtype=np.int64)
    assert np.array_equal(sse.numpy(), want_sse), f"{name}: sse differs in rows {np.nonzero((sse.numpy() != want_sse).any(1))[0][:5]}"
    worst = 0.0
    for i, row in enumerate(r["rows"]):
        for c in range(3):
            got, ref, floor = float(ssim[i, c]), row["ssim"][c], FLOORS[name][i][c]
            if not np.isnan(ref):
                worst = max(worst, abs(got - ref) / M.bound(floor))
            assert M.ssim_ok(got, ref, floor), f"{name} box {i} channel {c}: ssim {got!r} vs {ref!r}, |diff| {abs(got - ref):.3e} > {M.bound(floor):.3e}"
            if content == "same" and not np.isnan(ref):
                assert got == 1.0
    print(f"{name} [{elem}]: worst |ssim - fp64| / bound = {worst:.3f}")
    assert outside.tolist() == [list(o) for o in r["outside"]], f"{name}: outside diff {outside.tolist()} vs {r['outside']}"
    if geometry == "one":
        H, W = C.SIZES[0]
        assert int(outside[0, 0]) == int((r["A"][0] != r["B"][0]).any(2).sum()) > 0.9 * H * W        # a page without boxes counts all its pixels


@pytest.mark.parametrize("name,content,geometry", C.CASES, ids=CASE_IDS)
def test_public_functions_and_derived_fields(cuda, refs, dev_pages, name, content, geometry):
    from diffute_amd import _cabi, metrics
    r = refs[name]
    a, b = dev_pages[content]
    m = metrics.box_metrics_pages(a, b, r["boxes"])
    o = metrics.outside_diff_pages(a, b, r["boxes"])
    _cabi.synchronize()
    N = len(r["rows"])
    assert m.n.dtype == m.sse.dtype == o.changed.dtype == o.sse.dtype == torch.int64 and m.ssim_rgb.dtype == torch.float32
    assert m.n.shape == m.mse.shape == m.psnr.shape == m.ssim.shape == (N,) and m.sse.shape == m.ssim_rgb.shape == (N, 3)
    assert all(t.device == a[0].device for t in m) and o.changed.shape == o.sse.shape == (len(a),)
    assert m.n.tolist() == [row["n"] for row in r["rows"]]
    assert np.array_equal(m.sse.cpu().numpy(), np.array([row["sse"] for row in r["rows"]]))
    assert (o.changed.tolist(), o.sse.tolist()) == ([x[0] for x in r["outside"]], [x[1] for x in r["outside"]])
    for i, row in enumerate(r["rows"]):
        mse, psnr = M.derived(row["n"], row["sse"])
        assert abs(float(m.mse[i]) - mse) <= 1e-15 * mse and (float(m.psnr[i]) == psnr if np.isinf(psnr) else abs(float(m.psnr[i]) - psnr) <= 1e-12)
        if np.isnan(row["ssim"]).any():
            assert torch.isnan(m.ssim[i]) and torch.isnan(m.ssim_rgb[i]).all()
        else:
            assert abs(float(m.ssim[i]) - float(m.ssim_rgb[i].double().mean())) <= 1e-15
        if content == "same":
            assert int(m.sse[i].sum()) == 0 and float(m.psnr[i]) == float("inf") and (np.isnan(row["ssim"]).any() or float(m.ssim[i]) == 1.0)


@pytest.mark.parametrize("content", ["noise", "page"])
def test_a_box_alone_is_the_box_in_the_batch(cuda, dev_pages, content):
    """every box of the main table measured alone through the one-page function, a page's boxes through the one-page function, the batch
    twice, and the batch from the other build: the same bits"""
    from diffute_amd import _cabi, metrics
    a, b = dev_pages[content]
    batch = metrics.box_metrics_pages(a, b, C.MAIN)
    again = metrics.box_metrics_pages(a, b, C.MAIN)
    t = _tables(dev_pages, content, C.MAIN)
    other = metrics._box_metrics_raw(t, lib=_cabi.lib("fp16"))
    other_out = metrics._outside_diff_raw(t, lib=_cabi.lib("fp16"))
    this_out = metrics._outside_diff_raw(t, lib=_cabi.lib("bf16"))
    paged_out = metrics.outside_diff_pages(a, b, C.MAIN)
    _cabi.synchronize()
    for f in ("n", "sse", "ssim_rgb"):
        assert torch.equal(_bits(getattr(batch, f)), _bits(getattr(again, f))), f"two runs differ in {f}"
    assert torch.equal(_bits(batch.sse), _bits(other[0])) and torch.equal(_bits(batch.ssim_rgb), _bits(other[1])), "the two builds differ"
    assert torch.equal(other_out, this_out)
    i = 0
    for p in range(len(a)):
        page = metrics.box_metrics(a[p], b[p], C.MAIN[p])
        od = metrics.outside_diff(a[p], b[p], C.MAIN[p])
        k = len(C.MAIN[p])
        for f in ("n", "sse", "ssim_rgb", "mse", "psnr", "ssim"):
            got, want = getattr(page, f), getattr(batch, f)[i:i + k]
            assert torch.equal(_bits(got), _bits(want)), (p, f)
        assert int(od.changed[0]) == int(paged_out.changed[p]) and int(od.sse[0]) == int(paged_out.sse[p])
        for j, bx in enumerate(C.MAIN[p]):
            alone = metrics.box_metrics(a[p], b[p], [bx])
            assert torch.equal(_bits(alone.sse), _bits(batch.sse[i + j:i + j + 1])), (p, j, "sse")
            assert torch.equal(_bits(alone.ssim_rgb), _bits(batch.ssim_rgb[i + j:i + j + 1])), (p, j, "ssim_rgb")
        i += k
    # the two identical boxes and nothing else share a row's bits with a neighbour
    assert torch.equal(_bits(batch.ssim_rgb[16]), _bits(batch.ssim_rgb[17])) and torch.equal(batch.sse[16], batch.sse[17])


def test_refusals_report_the_index_and_write_nothing(cuda, dev_pages):
    from diffute_amd import _cabi, metrics
    lib = _cabi.lib()
    a, b = dev_pages["noise"]
    t = _tables(dev_pages, "noise", C.MAIN)
    base, st = t.dbuf.data_ptr(), _cabi.current_stream()
    bs, sse = _guarded((t.B, 3), torch.int64, cuda)
    bf, ssim = _guarded((t.B, 3), torch.float32, cuda)
    bo, out = _guarded((t.P, 2), torch.int64, cuda)
    need = int(lib.dmx_box_metrics_workspace_bytes(t.boxes, t.B))
    ws = torch.empty(need, dtype=torch.uint8, device=cuda)

    def box_call(ws_bytes=need):
        return lib.dmx_box_metrics_pages(t.pages, base, t.P, t.boxes, base + t.off_boxes, t.B, _cabi.ptr(sse), _cabi.ptr(ssim), _cabi.ptr(ws), ws_bytes, st)

    def out_call():
        return lib.dmx_page_outside_diff(t.pages, base, t.P, t.boxes, base + t.off_boxes, t.B, _cabi.ptr(out), st)

    def refused(msg):
        for call in (box_call, out_call):
            assert call() == _cabi.ERR_ARG
            assert msg in lib.dmx_last_error().decode(), lib.dmx_last_error().decode()

    keep = (t.boxes[9].x2, t.boxes[12].y2, t.boxes[4].x2)
    t.boxes[9].x2 = t.boxes[9].x1                                    # an empty box
    refused("box 9: (30, 2, 30, 28) is empty")
    t.boxes[9].x2 = keep[0]
    t.boxes[12].y2 = 65                                              # a box outside its page
    refused("box 12: (90, 30, 116, 65) lies outside the 150x64 page 1")
    t.boxes[12].y2 = keep[1]
    t.boxes[4].x2 = 20                                               # inside the page, but not the box the tables were prepared for
    refused("box 4: derived fields do not belong to this box table")
    t.boxes[4].x2 = keep[2]
    t.pages[1].H = 63                                                # the host table no longer describes the page the blocks were laid out for
    refused("page 1: derived fields do not belong to this page table")
    t.pages[1].H = 64
    assert box_call(need - 1) == _cabi.ERR_WORKSPACE and "workspace" in lib.dmx_last_error().decode()
    assert lib.dmx_box_metrics_pages(t.pages, base, t.P, t.boxes, base + t.off_boxes, 0, _cabi.ptr(sse), _cabi.ptr(ssim), _cabi.ptr(ws), need, st) == _cabi.ERR_ARG
    with pytest.raises(ValueError, match="page 1: the two versions differ in size"):
        metrics.box_metrics_pages(a, [b[0], b[1][:, :149].contiguous()], C.MAIN)
    with pytest.raises(ValueError, match="page 1: box 2: .* lies outside"):
        metrics.outside_diff_pages(a, b, [C.MAIN[0], C.MAIN[1][:2] + [(100, 0, 151, 20)]])
    with pytest.raises(ValueError, match="page 0: box 1: .* is empty"):
        metrics.box_metrics(a[0], b[0], [(0, 0, 11, 11), (5, 5, 5, 20)])
    _cabi.synchronize()
    for buf, name in ((bs, "sse"), (bf, "ssim"), (bo, "outside")):
        _guard_intact(buf, False, name)
    assert box_call() == 0 and out_call() == 0                       # the restored tables run
    _cabi.synchronize()
    for buf, name in ((bs, "sse"), (bf, "ssim"), (bo, "outside")):
        _guard_intact(buf, True, name)


def test_edit_boxes_changes_nothing_outside_its_boxes(cuda):
    """edit_boxes on the tiny UNet / VAE of the model tests: the page-level check of the paste kernels' promise, on the user's side"""
    import diffute_amd as D
    from diffute_amd.init import normal
    from test_models_gpu import TINY_UNET, TINY_VAE
    H, W, S = 320, 384, 128
    boxes = [(40, 60, 150, 78), (200, 150, 330, 180), (60, 250, 140, 266)]
    unet = D.UNet2DConditionModel(**TINY_UNET).cuda().requires_grad_(False)
    vae = D.AutoencoderKL(**TINY_VAE).cuda().requires_grad_(False)
    img = torch.from_numpy(np.random.RandomState(11).randint(0, 256, (H, W, 3), dtype=np.uint8)).to(cuda)
    ctx = normal(2, 13, 3 * 77 * 128, cuda).reshape(3, 77, 128)
    edited = D.edit_boxes(unet, vae, D.DDIMScheduler(), img, boxes, ctx, 1, origins=[(30, 20), (150, 90), (50, 210)], crop_scales=[128, 200, 96], size=S)
    o = D.metrics.outside_diff(img, edited, boxes)
    m = D.metrics.box_metrics(img, edited, boxes)
    same = D.metrics.box_metrics(edited, edited, boxes)
    D.synchronize()
    assert o.changed.tolist() == [0] and o.sse.tolist() == [0]
    assert (m.sse.sum(1) > 0).all() and torch.isfinite(m.psnr).all() and (m.ssim < 1.0).all()          # the edit did change its boxes
    assert same.sse.sum().item() == 0 and torch.isinf(same.psnr).all() and (same.ssim_rgb == 1.0).all() and (same.ssim == 1.0).all()
    assert D.metrics.outside_diff(img, edited, boxes[:2]).changed.item() > 0                           # ... and a box left out shows up
