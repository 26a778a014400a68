"""Choose the best of K candidates per box and paste the winners in ONE launch (csrc/prepost_batch.hip dmx_postprocess_paste_select
through prepost.postprocess_select_batch): injected score tables - distinct scores, exact ties, NaNs, a box whose scores are all NaN,
-inf, a threshold that skips boxes, K = 1, overlapping boxes - against the numpy selection rule (tests/readback_restatement.py) and, bit
for bit, against postprocess_batch of the chosen rows over the kept boxes."""
import numpy as np
import pytest
import torch

import readback_restatement as RB

pytestmark = pytest.mark.gpu

nan, inf = float("nan"), float("inf")
# the three boxes of tests/test_edit_boxes_gpu.py, then two that overlap box 1 and each other (a later item wins), the last one clipped
BOXES = [(40, 60, 150, 78), (200, 150, 330, 180), (60, 250, 140, 266), (280, 160, 360, 200), (300, 170, 380, 230)]
ORIGINS = [(30, 20), (150, 90), (50, 210), (250, 120), (290, 150)]
CROPS = [128, 200, 96, 128, 128]
TABLES = {
    "distinct": [[-1.0, -0.5, -2.0], [-3.0, -4.0, -0.25], [-0.1, -0.2, -0.3], [-9.0, -8.0, -8.5], [-2.0, -1.0, -1.5]],
    "ties": [[-0.5, -0.5, -0.5], [-2.0, -1.0, -1.0], [-1.0, -2.0, -1.0], [0.0, -0.0, -1.0], [-3.0, -3.0, -2.0]],
    "nans": [[nan, -3.0, nan], [nan, nan, nan], [-1.0, nan, -0.5], [nan, nan, -7.0], [-0.2, -0.1, nan]],
    "infs": [[-inf, -inf, -inf], [-inf, -5.0, -inf], [nan, -inf, nan], [inf, 1.0, inf], [-inf, nan, -inf]],
}


@pytest.fixture(scope="module")
def setup(cuda):
    rng = np.random.RandomState(5)
    vae = torch.from_numpy((rng.rand(5, 3, 3, RB.S, RB.S) * 2.4 - 1.2).astype(np.float32)).to(cuda)
    return dict(img=torch.from_numpy(RB.page()).to(cuda), vae=vae)


def _want(D, s, scores, threshold, idx=None):
    """the numpy rule for the choice; the existing batched paste of the chosen rows over the kept boxes for the page"""
    idx = list(range(5)) if idx is None else idx
    choice = RB.select(scores, -np.inf if threshold is None else threshold)
    keep = [j for j, c in enumerate(choice) if c >= 0]
    sel = lambda lst: [lst[idx[j]] for j in keep]
    boxes = [BOXES[i] for i in idx]
    if keep:
        rows = torch.stack([s["vae"][idx[j], int(choice[j])] for j in keep])
        page = D.prepost.postprocess_batch(rows, s["img"], sel(BOXES), sel(ORIGINS), sel(CROPS))
    else:
        page = s["img"]
    _, union = D.prepost.postprocess_batch(s["vae"][idx, 0], s["img"], boxes, [ORIGINS[i] for i in idx], [CROPS[i] for i in idx], return_mask=True)
    return choice, page, union


@pytest.mark.parametrize("threshold", [None, -1.0, -0.3, inf], ids=["none", "thr-1", "thr-0.3", "thr+inf"])
@pytest.mark.parametrize("table", sorted(TABLES))
def test_select_and_paste(cuda, setup, table, threshold):
    import diffute_amd as D
    scores = np.array(TABLES[table], dtype=np.float32)
    want_choice, want_page, want_union = _want(D, setup, scores, threshold)
    out, choice, union = D.prepost.postprocess_select_batch(setup["vae"], torch.from_numpy(scores).to(cuda), setup["img"], BOXES, ORIGINS, CROPS,
                                                            threshold=threshold, return_mask=True)
    D.synchronize()
    assert choice.dtype == torch.int32 and choice.cpu().numpy().tolist() == want_choice.tolist()
    assert torch.equal(out, want_page), "the page differs from postprocess_batch of the chosen rows over the kept boxes"
    assert torch.equal(union, want_union), "the union mask covers the boxes of ALL items, skipped ones included"
    if (want_choice < 0).all():
        assert torch.equal(out, setup["img"]), "every box skipped: the page is the original"
    out2, choice2 = D.prepost.postprocess_select_batch(setup["vae"], torch.from_numpy(scores).to(cuda), setup["img"], BOXES, ORIGINS, CROPS,
                                                       threshold=threshold)
    assert torch.equal(out2, out) and torch.equal(choice2, choice)


def test_cases_cover_what_they_claim():
    c = {k: RB.select(v).tolist() for k, v in TABLES.items()}
    assert c == {"distinct": [1, 2, 0, 1, 1], "ties": [0, 1, 0, 0, 2], "nans": [1, 0, 2, 2, 1], "infs": [0, 1, 1, 0, 0]}
    assert RB.select(TABLES["distinct"], -1.0).tolist() == [1, 2, 0, -1, 1]                      # the threshold skips one box
    assert all((RB.select(v, inf) < 0).sum() >= 3 for v in TABLES.values())
    x = lambda a, b: a[0] < b[2] and b[0] < a[2] and a[1] < b[3] and b[1] < a[3]
    assert x(BOXES[1], BOXES[3]) and x(BOXES[3], BOXES[4]) and x(BOXES[1], BOXES[4])


@pytest.mark.parametrize("threshold", [None, -1.0])
def test_k1_and_a_single_box(cuda, setup, threshold):
    import diffute_amd as D
    scores = np.array([[-0.5], [-2.0], [nan], [-1.0], [-inf]], dtype=np.float32)
    want_choice, want_page, want_union = _want(D, setup, scores, threshold)
    out, choice, union = D.prepost.postprocess_select_batch(setup["vae"][:, :1], torch.from_numpy(scores).to(cuda), setup["img"], BOXES, ORIGINS, CROPS,
                                                            threshold=threshold, return_mask=True)
    D.synchronize()
    assert choice.cpu().numpy().tolist() == want_choice.tolist() and torch.equal(out, want_page) and torch.equal(union, want_union)
    if threshold is None:                                   # K = 1, no threshold: exactly the existing batched paste
        assert choice.cpu().numpy().tolist() == [0] * 5
        assert torch.equal(out, D.prepost.postprocess_batch(setup["vae"][:, 0], setup["img"], BOXES, ORIGINS, CROPS))
    one = np.array([[-3.0, -1.0, -2.0]], dtype=np.float32)
    c1, p1, u1 = _want(D, setup, one, threshold, idx=[4])
    out, choice, union = D.prepost.postprocess_select_batch(setup["vae"][4:5], torch.from_numpy(one).to(cuda), setup["img"], BOXES[4:], ORIGINS[4:],
                                                            CROPS[4:], threshold=threshold, return_mask=True)
    D.synchronize()
    assert choice.cpu().numpy().tolist() == c1.tolist() == [1] and torch.equal(out, p1) and torch.equal(union, u1)


def test_the_cap_of_64_boxes_and_16_candidates(cuda, setup):
    """B = 64, K = 16: the score table fills its LDS array; boxes tile the page in a grid, scores random with NaNs"""
    import diffute_amd as D
    rng = np.random.RandomState(9)
    boxes = [(8 + 46 * (i % 8), 6 + 39 * (i // 8), 8 + 46 * (i % 8) + 40, 6 + 39 * (i // 8) + 30) for i in range(64)]
    origins, crops = [(min(b[0], RB.W - 64), min(b[1], RB.H - 64)) for b in boxes], [64] * 64
    vae = torch.from_numpy((rng.rand(64, 16, 3, 16, 16) * 2 - 1).astype(np.float32)).to(cuda)
    scores = rng.randn(64, 16).astype(np.float32)
    scores[rng.rand(64, 16) < 0.2] = nan
    scores[5] = nan
    want = RB.select(scores, 1.5)
    out, choice = D.prepost.postprocess_select_batch(vae, torch.from_numpy(scores).to(cuda), setup["img"], boxes, origins, crops, threshold=1.5)
    D.synchronize()
    assert choice.cpu().numpy().tolist() == want.tolist() and (want < 0).any() and (want > 0).any()
    keep = [b for b in range(64) if want[b] >= 0]
    rows = torch.stack([vae[b, int(want[b])] for b in keep])
    assert torch.equal(out, D.prepost.postprocess_batch(rows, setup["img"], [boxes[b] for b in keep], [origins[b] for b in keep], [64] * len(keep)))
