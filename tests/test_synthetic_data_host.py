"""Host side of the synthetic document dataset (diffute_amd/data.py), no GPU: ds[i] as a pure function of (seed, i), its layout rules
and the shape of its OCR records; sample_boxes against hand-worked cases of every rule of the reference's __getitem__
(train_diffute_v1.py:445-489)."""
import numpy as np
import pytest

import page_compose_cases as C


@pytest.fixture(scope="module")
def atlas():
    from diffute_amd.glyphs import GlyphAtlas
    return GlyphAtlas.from_arrays(C.load_atlas_arrays(), "atlas.")


def test_public_names():
    import diffute_amd as D
    from diffute_amd import data
    for name in ("SyntheticDocuments", "sample_boxes", "training_batch"):
        assert name in D.__all__ and getattr(D, name) is getattr(data, name)


def test_a_page_is_a_pure_function_of_seed_and_index(atlas):
    import diffute_amd as D
    a, b = D.SyntheticDocuments(atlas, seed=5), D.SyntheticDocuments(atlas, seed=5)
    first = [a[i] for i in (0, 1, 2, 3)]
    again = [b[i] for i in (3, 1, 0, 2, 3)]
    assert [again[2], again[1], again[3], again[0]] == first and again[0] == again[4]
    assert a[7] == a[7] and a[0] != a[1]
    assert D.SyntheticDocuments(atlas, seed=6)[0] != first[0]
    with pytest.raises(IndexError):
        a[-1]


def _exclusive(box):
    xs, ys = [p[0] for p in box], [p[1] for p in box]
    return min(xs), min(ys), max(xs) + 1, max(ys) + 1


def test_layout_rules_and_the_document_shape(atlas):
    import diffute_amd as D
    from diffute_amd import data
    ragged = D.SyntheticDocuments(atlas, page_size=lambda rng: (int(rng.integers(300, 500)), int(rng.integers(280, 700))), lines=(1, 24), seed=1)
    sets = [(D.SyntheticDocuments(atlas, seed=2), range(6), (1100, 1300)), (ragged, range(12), None),
            (D.SyntheticDocuments(atlas, page_size=(1300, 1100), lines=(24, 24), seed=3, chars="il.,", tex_amp=0), range(3), (1300, 1100))]
    low = high = dark = light = 0
    for ds, idx, size in sets:
        for i in idx:
            r = ds[i]
            H, W = r["size"]
            assert size is None or (H, W) == size
            assert set(r) == {"size", "bg", "tex_seed", "tex_amp", "lines", "document"}
            assert len(r["lines"]) == len(r["document"]) >= 1 and len(r["lines"]) <= ds.lines[1]
            assert 0 <= r["tex_seed"] < 1 << 32 and r["tex_amp"] == ds.tex_amp and all(0 <= v <= 255 for v in r["bg"])
            boxes = []
            for ln, d in zip(r["lines"], r["document"]):
                assert set(d) == {"text", "box", "score"} and set(ln) == {"text", "pen", "ink"}
                assert d["text"] == ln["text"] and ln["text"] == ln["text"].strip() and ln["text"]
                assert all(c in ds.chars + " " for c in ln["text"])
                assert len(d["box"]) == 4 and all(len(p) == 2 and all(isinstance(v, int) for v in p) for p in d["box"])
                assert isinstance(d["score"], float) and 0.5 <= d["score"] < 1.0
                x0, y0, x1, y1 = _exclusive(d["box"])
                assert 0 <= x0 < x1 <= W and 0 <= y0 < y1 <= H, (d["box"], r["size"])
                # the box IS the ink extent of the line as the atlas lays it out
                assert (x0, y0, x1, y1) == data.ink_extent(atlas, atlas.place(ln["text"], ln["pen"]))
                # ink against the background: dark on light or light on dark, with contrast
                assert abs(sum(ln["ink"]) - sum(r["bg"])) >= 3 * 100
                boxes.append((x0, y0, x1, y1))
                low += d["score"] <= 0.8; high += d["score"] > 0.8
            for a in range(len(boxes)):
                for b in range(a + 1, len(boxes)):
                    p, q = boxes[a], boxes[b]
                    assert p[2] <= q[0] or q[2] <= p[0] or p[3] <= q[1] or q[3] <= p[1], (p, q)
            assert [b[1] for b in boxes] == sorted(b[1] for b in boxes)                    # stacked top to bottom
            assert any(d["score"] > 0.8 for d in r["document"])
            dark += sum(r["bg"]) < 3 * 128; light += sum(r["bg"]) >= 3 * 128
    assert low > 20 and high > 20 and dark >= 1 and light > dark
    assert max(len(sets[2][0][i]["lines"]) for i in range(3)) == C.MAX_LINES                # a 1300-row page holds the maximum of 24
    with pytest.raises(ValueError, match="missing"):
        D.SyntheticDocuments(atlas, chars="aé")
    with pytest.raises(ValueError, match="lines"):
        D.SyntheticDocuments(atlas, lines=(5, 4))


class _Script:
    """an rng that hands out scripted values and records the ranges it was asked for"""

    def __init__(self, values):
        self.values, self.asked = list(values), []

    def integers(self, lo, hi):
        self.asked.append((lo, hi))
        assert lo < hi, "an empty range reached the generator"
        v = self.values.pop(0)
        v = {"lo": lo, "hi": hi - 1}.get(v, v)
        assert lo <= v < hi
        return v


def _rec(size, document):
    return {"size": size, "document": [dict(text=t, box=b, score=s) for t, b, s in document]}


def _box(x1, y1, x2, y2):
    return [[x1, y1], [x2, y1], [x2, y2], [x1, y2]]


def test_sample_boxes_hand_worked_rules():
    from diffute_amd import sample_boxes
    # the score filter: 0.8 itself is out, the pick indexes the KEPT lines; the hull of a skewed quadrilateral; bottom + h / 10
    quad = [[303, 498], [400, 500], [398, 541], [300, 539]]
    r = _rec((1000, 800), [("low", _box(0, 0, 10, 10), 0.8), ("skewed text", quad, 0.81), ("other", _box(5, 600, 90, 640), 0.99)])
    rng = _Script([0, "lo", "hi"])
    loc, org, txt = sample_boxes([r], rng)
    # hull (300, 498, 400, 541); h = 43 -> y2 = 545.3 -> 545; x in [max(0, 400 - 256), 300) = [144, 300); y in [545 - 256, 498) = [289, 498)
    assert loc == [[(300, 498, 400, 545)]] and rng.asked == [(0, 2), (144, 300), (289, 498)]
    assert org == [[(144, 497)]] and txt == ["skewed text"]
    rng = _Script([1, "hi", "lo"])
    loc, org, txt = sample_boxes([r], rng)
    assert loc == [[(5, 600, 90, 644)]] and rng.asked == [(0, 2), (0, 5), (388, 600)] and org == [[(4, 388)]] and txt == ["other"]
    # the clip of the extended bottom to H - 1
    r = _rec((650, 800), [("clip", _box(400, 600, 500, 648), 0.9)])
    loc, org, _ = sample_boxes([r], _Script([0, "lo", "lo"]))
    assert loc == [[(400, 600, 500, 649)]] and org == [[(244, 393)]]                        # 648 + 4.8 = 652.8 -> 649
    # a box as wide as the crop or wider: the crop starts at x1 and the text keeps int(len * 256 / width) characters; nothing drawn for x
    r = _rec((600, 1200), [("abcdefghijklmnopqrst", _box(100, 50, 612, 90), 0.9)])          # width 512 -> 10 of 20 characters
    rng = _Script([0, "hi"])
    loc, org, txt = sample_boxes([r], rng)
    assert loc == [[(100, 50, 612, 94)]] and org == [[(100, 49)]] and txt == ["abcdefghij"] and rng.asked == [(0, 1), (0, 50)]
    r = _rec((600, 1200), [("abcdefghijklmnopqrst", _box(100, 50, 356, 90), 0.9)])          # width 256 exactly: not shorter, all 20 kept
    loc, org, txt = sample_boxes([r], _Script([0, 7]))
    assert org == [[(100, 7)]] and txt == ["abcdefghijklmnopqrst"]
    r = _rec((600, 1200), [("abcdefghijklmnopqrst", _box(100, 50, 401, 90), 0.9)])          # width 301: int(20 * 256 / 301) = 17
    assert sample_boxes([r], _Script([0, 0]))[2] == ["abcdefghijklmnopq"]
    # a tall box: 300 + 30 = 330 rows -> the text is cut a second time, int(17 * 256 / 330) = 13; no draw for either origin
    r = _rec((900, 1200), [("abcdefghijklmnopqrst", _box(100, 50, 401, 350), 0.9)])
    rng = _Script([0])
    loc, org, txt = sample_boxes([r], rng)
    assert loc == [[(100, 50, 401, 380)]] and org == [[(100, 50)]] and txt == ["abcdefghijklm"] and rng.asked == [(0, 1)]
    # the fall-backs to 0: a box at the left / top edge leaves an empty range [max(0, x2 - 256), x1)
    r = _rec((600, 1200), [("edge", _box(0, 0, 80, 30), 0.9)])
    rng = _Script([0])
    loc, org, _ = sample_boxes([r], rng)
    assert loc == [[(0, 0, 80, 33)]] and org == [[(0, 0)]] and rng.asked == [(0, 1)]
    r = _rec((600, 1200), [("narrow", _box(300, 0, 301, 40), 0.9)])                         # x range [45, 300); y range [0, 0) is empty
    rng = _Script([0, "hi"])
    assert sample_boxes([r], rng)[1] == [[(299, 0)]] and rng.asked == [(0, 1), (45, 300)]
    # float corners, as OCR json has them: the hull is truncated to int32 after the extension
    r = _rec((600, 1200), [("float", [[10.6, 20.2], [99.9, 20.2], [99.9, 59.7], [10.6, 59.7]], 0.9)])
    assert sample_boxes([r], _Script([0, 0, 0]))[0] == [[(10, 20, 99, 63)]]                  # 59.7 + 3.95 = 63.65
    # several pages share one stream, page after page; another crop scale moves every threshold
    two = [_rec((600, 1200), [("a", _box(300, 200, 350, 240), 0.9)]), _rec((700, 900), [("b", _box(500, 400, 560, 430), 0.95)])]
    rng = _Script([0, "lo", "lo", 0, "hi", "hi"])
    loc, org, txt = sample_boxes(two, rng, crop_scale=128)
    assert rng.asked == [(0, 1), (222, 300), (116, 200), (0, 1), (432, 500), (305, 400)]
    assert org == [[(222, 116)], [(499, 399)]] and txt == ["a", "b"] and len(loc) == 2
    with pytest.raises(ValueError, match="no line with score"):
        sample_boxes([_rec((600, 600), [("x", _box(0, 0, 5, 5), 0.5)])], _Script([]))
    with pytest.raises(ValueError, match="smaller than the crop"):
        sample_boxes([_rec((200, 600), [("x", _box(0, 0, 5, 5), 0.9)])], _Script([]))


def test_sample_boxes_on_the_dataset_with_numpy_generators(atlas):
    import diffute_amd as D
    ds = D.SyntheticDocuments(atlas, seed=4)
    recs = [ds[i] for i in range(4)]
    a = D.sample_boxes(recs, np.random.default_rng(3))
    assert a == D.sample_boxes(recs, np.random.default_rng(3)) and a != D.sample_boxes(recs, np.random.default_rng(4))
    legacy = D.sample_boxes(recs, np.random.RandomState(3))                                 # the reference's np.random interface works too
    for r, loc, org, text in zip(recs, *a):
        (x1, y1, x2, y2), (x_s, y_s) = loc[0], org[0]
        H, W = r["size"]
        d = next(d for d in r["document"] if d["text"].startswith(text) and _exclusive(d["box"])[:2] == (x1, y1))
        assert d["score"] > 0.8 and 0 <= x1 < x2 < W and 0 <= y1 < y2 <= H - 1
        assert 0 <= x_s <= x1 and 0 <= y_s <= y1 and x_s < W and y_s < H
        assert text == d["text"] or x2 - x1 >= 256
    assert len(legacy[0]) == 4
