"""Host side of the page composer (csrc/page_compose.hip, diffute_amd/data.py), no GPU: the numpy restatement of the rule in
include/diffute_hip.h (tests/page_compose_restatement.py) against the pages Pillow drew, stored in tests/golden/page_compose.npz, and -
where Pillow with FreeType and the font are installed - against a live ImageDraw.text on an RGB image; six injected faults, which the
case list must be able to see; the host tables diffute_amd.data builds; the refusals of the C-ABI entry, which checks the host copies of
its tables before anything is launched."""
import ctypes
import os

import numpy as np
import pytest

import page_compose_cases as C
import page_compose_restatement as T


@pytest.fixture(scope="module")
def golden():
    return C.load_golden()


@pytest.fixture(scope="module")
def atlas():
    from diffute_amd.glyphs import GlyphAtlas
    return GlyphAtlas.from_arrays(C.load_atlas_arrays(), "atlas.")


@pytest.fixture(scope="module")
def restated(atlas):
    out = {name: T.compose(atlas, pg) for name, pg in C.CASES}
    for v in out.values():
        v.setflags(write=False)
    return out


def test_restatement_reproduces_pillows_pages(golden, restated):
    for name, pg in C.CASES:
        want = golden["page." + name]
        assert want.shape == pg["size"] + (3,) and want.dtype == np.uint8
        assert np.array_equal(restated[name], want), f"{name}: {int((restated[name] != want).sum())} bytes differ from Pillow's page"


def test_the_cases_hold_what_they_claim(golden, atlas):
    """both clamps of the texture fire, the overlapping lines do overlap, the off-page lines leave ink on the edges or none at all"""
    for bg, edge in ((0, 0), (3, 0), (252, 255), (255, 255)):
        flat, tex = golden[f"page.clamp_{bg}_0"], golden[f"page.clamp_{bg}_6"]
        blank = T.background((20, 130), (bg,) * 3, 7 + bg, 6)
        assert (blank == edge).any() and len(np.unique(blank)) > 3, bg                    # clamped at the edge, and textured
        assert len(np.unique(T.background((20, 130), (bg,) * 3, 7 + bg, 0))) == 1
        assert not np.array_equal(flat, tex)
    wrapped = T.background((20, 130), (3, 3, 3), 10, 6, fault="tex_wrap")
    assert (wrapped > 250).any()
    a, b = C.BY_ID["overlap_ab"], C.BY_ID["overlap_ba"]
    size = a["size"]
    both = (T.line_coverage(atlas, a["lines"][0], size) > 0) & (T.line_coverage(atlas, a["lines"][1], size) > 0)
    assert both.sum() > 100 and not np.array_equal(golden["page.overlap_ab"], golden["page.overlap_ba"])
    assert a["lines"] == b["lines"][::-1]
    pg = C.BY_ID["partly_off"]
    ink = (golden["page.partly_off"].astype(int) - T.background(pg["size"], pg["bg"], pg["tex_seed"], pg["tex_amp"])).any(axis=2)
    assert ink[:, 0].any() and ink[:, -1].any() and ink[0].any() and ink[-1].any()
    pg = C.BY_ID["wholly_off"]
    only_in = dict(pg, lines=pg["lines"][:1])
    assert np.array_equal(golden["page.wholly_off"], T.compose(atlas, only_in)) and len(pg["lines"]) == 5
    kern = {(atlas.chars[i], atlas.chars[j]) for i, j in atlas.kern_pairs}
    assert {("A", "V"), ("T", "o"), ("r", "n")} <= kern


@pytest.mark.parametrize("fault", T.FAULTS)
def test_the_case_list_sees_an_injected_fault(golden, atlas, fault):
    changed = [name for name, pg in C.CASES if not np.array_equal(T.compose(atlas, pg, fault=fault), golden["page." + name])]
    assert changed, f"no case notices the fault {fault!r}"
    want = {"max": "kerned", "merged": "overlap_ab", "no_round": "inks", "reverse": "overlap_ba", "tex_wrap": "clamp_3_6", "two_round": "inks"}[fault]
    assert want in changed, (fault, changed)


def _pil():
    PIL = pytest.importorskip("PIL")
    from PIL import ImageFont, features
    if not features.check("freetype2"):
        pytest.skip("Pillow without FreeType")
    if not os.path.exists(C.FONT_PATH):
        pytest.skip(f"{C.FONT_PATH} is not installed")
    return ImageFont.truetype(C.FONT_PATH, C.FONT_SIZE, layout_engine=ImageFont.Layout.BASIC)


def _pil_page(font, pg):
    from PIL import Image, ImageDraw
    img = Image.fromarray(T.background(pg["size"], pg["bg"], pg["tex_seed"], pg["tex_amp"]), "RGB")
    draw = ImageDraw.Draw(img)
    for ln in pg["lines"]:
        draw.text(tuple(ln["pen"]), ln["text"], font=font, fill=tuple(ln["ink"]))
    return np.asarray(img)


def test_live_pillow_draws_the_cases_and_random_pages(golden, atlas, restated):
    font = _pil()
    for name, pg in C.CASES:
        live = _pil_page(font, pg)
        assert np.array_equal(live, golden["page." + name]), f"{name}: this Pillow draws another page than the fixture ({golden['versions']})"
    rng = np.random.default_rng(20240519)
    for k in range(12):                                 # random inks, pens (off every edge too), backgrounds and line counts
        H, W = int(rng.integers(30, 120)), int(rng.integers(60, 300))
        lines = [("".join(chr(int(c)) for c in rng.integers(32, 127, int(rng.integers(1, 9)))),
                  (int(rng.integers(-60, W)), int(rng.integers(-40, H))), tuple(int(v) for v in rng.integers(0, 256, 3)))
                 for _ in range(int(rng.integers(0, 6)))]
        pg = C.page((H, W), tuple(int(v) for v in rng.integers(0, 256, 3)), lines, int(rng.integers(0, 1 << 32)), int(rng.integers(0, 20)))
        assert np.array_equal(T.compose(atlas, pg), _pil_page(font, pg)), pg


def test_the_host_tables(atlas):
    from diffute_amd import _cabi, data
    assert ctypes.sizeof(_cabi.PageRec) == 72 and ctypes.sizeof(_cabi.PageLine) == 40
    recs = [C.BY_ID[n] for n in ("empty", "inks", "wholly_off")]
    pages, lines, places = data.page_tables(atlas, recs)
    assert pages.shape == (3,) and lines.shape == (10,) and places.dtype == np.int32
    assert list(pages["first_line"]) == [0, 0, 5] and list(pages["n_lines"]) == [0, 5, 5]
    assert list(pages["H"]) == [9, 196, 50] and list(pages["W"]) == [130, 257, 140] and pages["bg"][1].tolist() == [200, 190, 180]
    assert int(lines["first"][-1] + lines["count"][-1]) == places.shape[0] == sum(len(l["text"]) for r in recs for l in r["lines"])
    for l, ln in zip(lines, [l for r in recs for l in r["lines"]]):
        pl = places[l["first"]:l["first"] + l["count"]]
        assert np.array_equal(pl, atlas.place(ln["text"], ln["pen"])) and l["rgb"].tolist() == list(ln["ink"])
        for g, x, y in pl:                              # the box holds every bitmap of the line
            w, h = int(atlas.rec[g, 1]), int(atlas.rec[g, 2])
            assert w * h == 0 or (l["x0"] <= x and l["y0"] <= y and x + w <= l["x1"] and y + h <= l["y1"])
    # the box holds the restatement's coverage and is no looser than a bitmap's blank border (FreeType pads some bitmaps by a column or two)
    m = T.line_coverage(atlas, recs[1]["lines"][0], recs[1]["size"])
    ys, xs = np.nonzero(m)
    ink, box = (xs.min(), ys.min(), xs.max() + 1, ys.max() + 1), tuple(int(lines[k][0]) for k in ("x0", "y0", "x1", "y1"))
    assert box[0] <= ink[0] <= box[0] + 4 and box[1] <= ink[1] <= box[1] + 4 and box[2] - 4 <= ink[2] <= box[2] and box[3] - 4 <= ink[3] <= box[3]


def test_the_entry_refuses_bad_tables_on_the_host(atlas):
    """the "device" pointers here are never read: every call is refused before a launch"""
    from diffute_amd import _cabi, data
    lib = _cabi.lib()
    fake = 0x1000
    rec = np.ascontiguousarray(atlas.rec)

    def call(mutate=None, P=None, n_lines=None, n_places=None, pages_dev=fake, lines_dev=fake):
        pages, lines, places = data.page_tables(atlas, [C.BY_ID["overlap_ab"], C.BY_ID["empty"]])
        pages["dst"], pages["stride_y"], pages["stride_x"], pages["stride_c"] = fake, pages["W"] * 3, 3, 1
        if mutate:
            mutate(pages, lines, places)
        a = _cabi.GlyphAtlas(pool=fake, pool_bytes=atlas.pool.size, glyphs_host=rec.ctypes.data, glyphs_device=fake, n_glyphs=len(atlas))
        rc = lib.dmx_page_compose(ctypes.byref(a), pages.ctypes.data, pages_dev, len(pages) if P is None else P, lines.ctypes.data, lines_dev,
                                  len(lines) if n_lines is None else n_lines, places.ctypes.data, fake,
                                  places.shape[0] if n_places is None else n_places, None)
        return rc, lib.dmx_last_error().decode()

    def setv(table, field, index, value):
        def f(pages, lines, places):
            t = {"pages": pages, "lines": lines, "places": places}[table]
            if field is None:
                t[index] = value
            else:
                t[field][index] = value
        return f

    cases = [(dict(mutate=setv("lines", "count", 1, 7)), "placements [6, 6 + 7) end past the table of 12"),
             (dict(mutate=setv("lines", "first", 0, -1)), "end past the table"),
             (dict(n_places=11), "end past the table of 11"),
             (dict(mutate=setv("pages", "n_lines", 0, 3)), "lines [0, 0 + 3) end past the table of 2"),
             (dict(mutate=setv("pages", "first_line", 1, 3)), "end past the table"),
             (dict(n_lines=1), "end past the table of 1"),
             (dict(mutate=setv("pages", "dst", 1, 0)), "page 1: null destination"),
             (dict(P=0), "P = 0"), (dict(P=65536), "P = 65536"),
             (dict(pages_dev=None), "null argument"), (dict(lines_dev=None), "no line table"),
             (dict(mutate=setv("pages", "H", 0, 0)), "bad size"), (dict(mutate=setv("pages", "W", 1, 0)), "bad size"),
             (dict(mutate=setv("pages", "H", 0, 65536)), "bad size"),
             (dict(mutate=setv("pages", "tex_amp", 0, 256)), "tex_amp"), (dict(mutate=setv("pages", "tex_amp", 0, -1)), "tex_amp"),
             (dict(mutate=setv("pages", "bg", (0, 2), 256)), "background"), (dict(mutate=setv("lines", "rgb", (1, 0), -1)), "ink"),
             (dict(mutate=setv("lines", "x1", 0, 50)), "leaves the line's box"), (dict(mutate=setv("lines", "y0", 1, 40)), "leaves the line's box"),
             (dict(mutate=setv("places", None, (0, 0), 95)), "outside the atlas"), (dict(mutate=setv("places", None, (3, 1), 1 << 25)), "beyond")]
    for kw, msg in cases:
        rc, err = call(**kw)
        assert rc == _cabi.ERR_ARG and msg in err, (msg, rc, err)
