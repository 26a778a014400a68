"""diffute_amd.metrics without a GPU: the numpy restatement (metrics_restatement.py) is pinned to scipy's Gaussian filter, the recorded floors
of its fp32 formulation (metrics_floors.py) are measured again, the bound the GPU test uses (4 x floor + 2^-22 per box and channel) lets
the honest fp32 formulation through on every case and is broken by each injected fault on at least one, and the Python layer - argument
checks, host tables, derived quantities - is tested on hand-made inputs."""
import ctypes

import numpy as np
import pytest
import torch

import metrics_cases as C
import metrics_restatement as M
from metrics_floors import FLOORS

CASE_IDS = [c[0] for c in C.CASES]


def test_cases_hold_what_they_promise():
    """the shapes of the issue's table, with TILE = 16"""
    assert (M.TILE, M.WIN, C.E) == (16, 11, 26)
    hw = [(y2 - y1, x2 - x1) for _, (x1, y1, x2, y2) in C.flat_boxes("main")]
    for want in ((11, 11), (11, 12), (12, 11), (10, 30), (30, 10), (1, 1), (26, 25), (26, 26), (26, 27), (25, 26), (27, 26)):
        assert want in hw, want
    tiles = [(max(1, -(-(h - 10) // 16)), max(1, -(-(w - 10) // 16))) for h, w in hw]
    assert any(ty >= 2 and tx >= 3 for ty, tx in tiles)
    for p, (H, W) in enumerate(C.SIZES):
        boxes = C.MAIN[p]
        assert (0, 0, W, H) in boxes
        if p == 0:
            assert any(b[:2] == (0, 0) and b[2:] != (W, H) for b in boxes) and any(b[0] == 0 and b[3] == H and b[1] > 0 for b in boxes)
            assert any(b[1] == 0 and b[2] == W and b[0] > 0 for b in boxes) and any(b[2:] == (W, H) and b[0] > 0 for b in boxes)
    assert len(set(C.MAIN[1])) == len(C.MAIN[1]) - 1                                     # two identical boxes
    assert len(C.flat_boxes("one")) == 1 and C.ONE[0] == [] and len(C.flat_boxes("b65")) == 65
    for g in C.GEOMETRY.values():
        for p, boxes in enumerate(g):
            assert all(0 <= x1 < x2 <= C.SIZES[p][1] and 0 <= y1 < y2 <= C.SIZES[p][0] for x1, y1, x2, y2 in boxes)
    a, b = C.pages("pixel")
    assert [int((x != y).any(2).sum()) for x, y in zip(a, b)] == [1, 1]


@pytest.mark.parametrize("name,content,geometry", C.CASES, ids=CASE_IDS)
def test_restatement_is_scipys_gaussian_filter(name, content, geometry):
    """scikit-image's structural_similarity, written out with scipy: filter with the reflected border, crop 5, mean"""
    ndi = pytest.importorskip("scipy.ndimage")
    A, B = C.pages(content)
    c1, c2 = (0.01 * 255) ** 2, (0.03 * 255) ** 2
    worst = 0.0
    for p, (x1, y1, x2, y2) in C.flat_boxes(geometry):
        ref = M.ref64(A[p], B[p], (x1, y1, x2, y2))
        if min(y2 - y1, x2 - x1) < 11:
            assert np.isnan(ref["ssim"]).all()
            continue
        for c in range(3):
            x, y = A[p][y1:y2, x1:x2, c].astype(np.float64), B[p][y1:y2, x1:x2, c].astype(np.float64)
            g = lambda t: ndi.gaussian_filter(t, sigma=1.5, truncate=3.5, mode="reflect")
            ux, uy = g(x), g(y)
            vx, vy, vxy = g(x * x) - ux * ux, g(y * y) - uy * uy, g(x * y) - ux * uy
            s = ((2 * ux * uy + c1) * (2 * vxy + c2)) / ((ux * ux + uy * uy + c1) * (vx + vy + c2))
            want = s[5:-5, 5:-5].mean()
            worst = max(worst, abs(want - ref["ssim"][c]))
    print(f"{name}: restatement vs scipy.ndimage.gaussian_filter, worst difference {worst:.2e}")
    assert worst <= 1e-12


@pytest.mark.parametrize("name,content,geometry", C.CASES, ids=CASE_IDS)
def test_floors_are_the_measured_ones_and_the_honest_evaluation_passes(name, content, geometry):
    got, rec = np.array(C.measure(content, geometry)), np.array(FLOORS[name])
    assert got.shape == rec.shape == (len(C.flat_boxes(geometry)), 3)
    print(f"{name}: floor of the fp32 formulation, worst {got.max():.3e} (recorded {rec.max():.3e})")
    assert (np.abs(got - rec) <= 0.02 * rec + 1e-12).all(), f"{name}: recorded floors differ from the measured ones; regenerate metrics_floors.py"
    A, B = C.pages(content)
    for i, (p, bx) in enumerate(C.flat_boxes(geometry)):
        ref, ev = M.ref64(A[p], B[p], bx)["ssim"], M.eval32(A[p], B[p], bx)
        assert all(M.ssim_ok(ev[c], ref[c], rec[i][c]) for c in range(3)), (name, i, bx, ev, ref)
        if content == "same":
            assert (ev == np.float32(1.0)).all() or np.isnan(ref).all()


def _breaks(fault, cases):
    """the (case, box, channel) at which eval32 with the fault misses the GPU bound"""
    out = []
    for name, content, geometry in cases:
        A, B = C.pages(content)
        for i, (p, bx) in enumerate(C.flat_boxes(geometry)):
            ref, ev = M.ref64(A[p], B[p], bx)["ssim"], M.eval32(A[p], B[p], bx, fault)
            out += [(name, i, c) for c in range(3) if not M.ssim_ok(ev[c], ref[c], FLOORS[name][i][c])]
    return out


@pytest.mark.parametrize("fault", M.FAULTS)
def test_injected_fault_breaks_the_bound(fault):
    cases = [c for c in C.CASES if c[2] == "main"]
    if fault == "unpivoted":                                                              # the issue's case: plain fp32 moments on flat bright pages
        cases = [c for c in cases if c[1] in ("flat", "pixel")]
    bad = _breaks(fault, cases)
    print(f"{fault}: breaks {len(bad)} (case, box, channel) of {sum(3 * len(C.flat_boxes(c[2])) for c in cases)}, first {bad[:1]}")
    assert bad, f"the bound lets `{fault}` through on every case"


def test_unpivoted_moments_cancel_on_a_flat_page():
    """the figures of the issue: a 20 x 20 box of 255 against 253"""
    a, b = np.full((20, 20, 3), 255, np.uint8), np.full((20, 20, 3), 253, np.uint8)
    ref = M.ref64(a, b, (0, 0, 20, 20))["ssim"][0]
    plain, pivoted = float(M.eval32(a, b, (0, 0, 20, 20), "unpivoted")[0]), float(M.eval32(a, b, (0, 0, 20, 20))[0])
    print(f"flat 255 / 253: fp64 {ref:.9f}, plain fp32 off by {abs(plain - ref):.2e}, pivoted by {abs(pivoted - ref):.2e}")
    assert abs(plain - ref) > 1e-5 and abs(pivoted - ref) < 2.0 ** -22


# ---------------------------------------------------------------------------------------------------------------- the Python layer
def test_derived_quantities_on_hand_made_kernel_outputs():
    from diffute_amd import metrics
    n = torch.tensor([4, 100, 121, 1], dtype=torch.int64)
    sse = torch.tensor([[0, 0, 0], [300, 0, 0], [1, 2, 3], [65025, 65025, 65025]], dtype=torch.int64)
    nan = float("nan")
    ssim_rgb = torch.tensor([[nan, nan, nan], [1.0, 0.5, 0.0], [0.25, 0.25, 0.25], [nan, nan, nan]], dtype=torch.float32)
    m = metrics.derive(n, sse, ssim_rgb)
    assert m.n is n and m.sse is sse and m.ssim_rgb is ssim_rgb
    assert m.mse.dtype == m.psnr.dtype == m.ssim.dtype == torch.float64
    assert m.mse.tolist() == [0.0, 1.0, 6.0 / 363.0, 65025.0]
    assert m.psnr[0].item() == float("inf") and m.psnr[3].item() == 0.0
    assert abs(m.psnr[1].item() - 10.0 * np.log10(65025.0)) < 1e-12
    for i in (1, 2):
        mse, psnr = M.derived(int(n[i]), sse[i].numpy())
        assert abs(m.mse[i].item() - mse) <= 1e-15 * mse and abs(m.psnr[i].item() - psnr) <= 1e-12
    assert torch.isnan(m.ssim[[0, 3]]).all() and m.ssim[1].item() == 0.5 and m.ssim[2].item() == 0.25


def test_argument_checks_name_page_and_box(monkeypatch):
    from diffute_amd import metrics
    monkeypatch.setattr(torch.Tensor, "is_cuda", property(lambda self: True))             # meta tensors stand in for CUDA tensors
    pg = lambda h, w, dtype=torch.uint8: torch.empty((h, w, 3), dtype=dtype, device="meta")
    a, b = [pg(37, 53), pg(64, 150)], [pg(37, 53), pg(64, 150)]
    ok = [[(0, 0, 11, 11)], [(3, 2, 28, 28), (0, 0, 150, 64)]]
    A, B, flat, counts, _ = metrics._check_pairs(a, b, ok)
    assert flat == [ok[0][0], ok[1][0], ok[1][1]] and counts == [1, 2]
    assert metrics._check_pairs(a, b, [[], ok[1]])[3] == [0, 2]                            # a page without boxes is fine
    for args, msg in (
        (([], [], []), "no pages"),
        ((a, b[:1], ok), "lengths must agree"),
        ((a, b, ok[:1]), "lengths must agree"),
        ((a, [b[0], pg(64, 149)], ok), "page 1: the two versions differ in size"),
        ((a, [b[0], pg(64, 150, torch.float32)], ok), "page 1: images_b[1] must be a contiguous uint8"),
        (([a[0], pg(150, 64).permute(1, 0, 2)], b, ok), "page 1: images_a[1] must be a contiguous uint8"),
        (([a[0], torch.empty((64, 150), dtype=torch.uint8, device="meta")], b, ok), "page 1: images_a[1] must be HWC"),
        ((a, b, [[(0, 0, 11, 11)], [(3, 2, 3, 28)]]), "page 1: box 0: (3, 2, 3, 28) is empty"),
        ((a, b, [[(0, 0, 11, 11), (50, 0, 54, 5)], ok[1]]), "page 0: box 1: (50, 0, 54, 5) lies outside the 53x37 image"),
        ((a, b, [[(0, -1, 11, 11)], ok[1]]), "page 0: box 0"),
        ((a, b, [[(0, 0, 11)], ok[1]]), "page 0: box 0: expected (x1, y1, x2, y2)"),
    ):
        with pytest.raises(ValueError) as e:
            metrics._check_pairs(*args)
        assert msg in str(e.value), (msg, str(e.value))
    with pytest.raises(ValueError, match="no boxes"):
        metrics.box_metrics_pages(a, b, [[], []])
    monkeypatch.undo()
    with pytest.raises(ValueError, match="page 0: images_a\\[0\\] must be a contiguous uint8 CUDA tensor"):
        metrics.box_metrics(torch.zeros(20, 20, 3, dtype=torch.uint8), torch.zeros(20, 20, 3, dtype=torch.uint8), [(0, 0, 11, 11)])


def _tables(sizes, boxes):
    """host tables as metrics._upload fills them, with fake addresses"""
    from diffute_amd import _cabi
    P, flat = len(sizes), [(p, bx) for p, bs in enumerate(boxes) for bx in bs]
    pages, tab = (_cabi.MetricPage * P)(), (_cabi.MetricBox * max(len(flat), 1))()
    lo = 0
    for p, ((H, W), bs) in enumerate(zip(sizes, boxes)):
        pages[p].a, pages[p].b, pages[p].H, pages[p].W, pages[p].box_lo, pages[p].box_hi = 4096, 8192, H, W, lo, lo + len(bs)
        lo += len(bs)
    for i, (p, bx) in enumerate(flat):
        tab[i].page, (tab[i].x1, tab[i].y1, tab[i].x2, tab[i].y2) = p, bx
    return pages, tab, P, len(flat)


def test_host_tables_and_their_refusals():
    """the C side of the tables, which needs no GPU: the derived fields, and bad input reported by index with nothing launched"""
    from diffute_amd import _cabi
    lib = _cabi.lib()
    pages, tab, P, B = _tables(C.SIZES, C.MAIN)
    assert lib.dmx_metric_tables_prepare(pages, P, tab, B) == 0
    tiles = 0
    for i, (p, (x1, y1, x2, y2)) in enumerate(C.flat_boxes("main")):
        tx, ty = max(1, -(-(x2 - x1 - 10) // 16)), max(1, -(-(y2 - y1 - 10) // 16))
        assert (tab[i].tiles_x, tab[i].tiles_y, tab[i].tile_lo) == (tx, ty, tiles), i
        tiles += tx * ty
    assert lib.dmx_box_metrics_workspace_bytes(tab, B) == tiles * 48
    assert [(pg.block_lo, pg.blocks) for pg in pages] == [(0, 37 * 1), (37, 64 * 1)]
    w = (ctypes.c_float * 11)()
    assert lib.dmx_box_metrics_weights(w) == 0
    assert np.array_equal(np.array(w[:], dtype=np.float32), M.weights32()), "the library's window weights are not the restatement's, bit for bit"

    def refused(pages, tab, P, B, msg):
        assert lib.dmx_metric_tables_prepare(pages, P, tab, B) == _cabi.ERR_ARG
        assert msg in lib.dmx_last_error().decode(), lib.dmx_last_error().decode()

    for i, bx, msg in ((3, (42, 25, 42, 37), "box 3: (42, 25, 42, 37) is empty"), (9, (30, 2, 151, 28), "box 9: (30, 2, 151, 28) lies outside the 150x64 page 1"),
                       (0, (-1, 0, 11, 11), "box 0: (-1, 0, 11, 11) lies outside the 53x37 page 0")):
        pages, tab, P, B = _tables(C.SIZES, C.MAIN)
        tab[i].x1, tab[i].y1, tab[i].x2, tab[i].y2 = bx
        refused(pages, tab, P, B, msg)
    pages, tab, P, B = _tables(C.SIZES, C.MAIN)
    tab[8].page = 0
    refused(pages, tab, P, B, "box 8: page index 0, the box lies in the range of page 1")
    pages, tab, P, B = _tables(C.SIZES, C.MAIN)
    pages[1].box_lo = 7
    refused(pages, tab, P, B, "page 1: its boxes [7, 20) must start at 8")
    pages, tab, P, B = _tables(C.SIZES, C.MAIN)
    pages[0].W = 0
    refused(pages, tab, P, B, "page 0: bad size")
    pages, tab, P, B = _tables(C.SIZES, C.MAIN)
    pages[1].b = 0
    refused(pages, tab, P, B, "page 1: null image")
    # a page without boxes and no boxes at all are fine for the tables (the outside diff takes them)
    pages, tab, P, B = _tables(C.SIZES, [[], []])
    assert lib.dmx_metric_tables_prepare(pages, P, None, 0) == 0 and lib.dmx_box_metrics_workspace_bytes(None, 0) == 0
