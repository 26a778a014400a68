"""Host side of the glyph renderer (diffute_amd/glyphs.py), no GPU: the numpy restatement of the compositing rule
(tests/glyph_text_restatement.py) against Pillow's canvases stored in tests/golden/glyph_text.npz and - where Pillow with FreeType is
installed - against a live `ImageDraw.text` under the BASIC layout; GlyphAtlas's layout and persistence against the restatement; the
refusals of the argument checks; and three injected faults, which the case list must be able to see."""
import os
import random

import numpy as np
import pytest

import glyph_text_cases as C
import glyph_text_restatement as T


@pytest.fixture(scope="module")
def golden():
    return C.load_golden()


@pytest.fixture(scope="module")
def atlas(golden):
    from diffute_amd.glyphs import GlyphAtlas
    return GlyphAtlas.from_arrays(golden, "atlas.")


def test_restatement_reproduces_pillows_canvases(golden, atlas):
    assert len(atlas) == 95 and atlas.size == C.FONT_SIZE and atlas.chars == "".join(chr(c) for c in range(32, 127))
    for name, text, size, origin in C.CASES:
        want = golden["canvas." + name]
        assert want.shape == C.canvas_size(text, size)
        got = T.draw_text_grey(atlas, text, size, origin)
        assert np.array_equal(got, want), f"{name}: {int((got != want).sum())} pixels differ from Pillow's canvas"
    assert (golden["canvas.empty"] == 255).all() and (golden["canvas.one_letter"] < 255).any()
    for name in ("clip_a", "clip_b"):                                      # the clipped cases do clip: ink on the canvas's right and bottom edge
        c = golden["canvas." + name]
        assert (c[:, -1] < 255).any() and (c[-1] < 255).any(), name
    assert (golden["canvas.clip_b"][:, 0] < 255).any()                     # ... and on the left


def test_atlas_layout_and_persistence(atlas, tmp_path):
    from diffute_amd.glyphs import GlyphAtlas
    p = str(tmp_path / "atlas.npz")
    atlas.save(p)
    again = GlyphAtlas.load(p)
    for k in ("rec", "pool", "kern_pairs", "kern_values"):
        assert np.array_equal(getattr(again, k), getattr(atlas, k)), k
    assert (again.chars, again.size, again.font_name) == (atlas.chars, atlas.size, atlas.font_name)
    rng = random.Random(7)
    texts = [c[1] for c in C.CASES] + ["".join(rng.choice(atlas.chars) for _ in range(rng.randint(1, 20))) for _ in range(50)]
    for t in texts:
        for origin in ((40, 10), (-3, 25)):
            got = again.place(t, origin)
            assert got.dtype == np.int32 and got.shape == (len(t), 3)
            assert np.array_equal(got, np.array(T.place(atlas, t, origin), dtype=np.int32).reshape(-1, 3)), (t, origin)
    assert again.place("").shape == (0, 3)
    assert GlyphAtlas.canvas_size("") == (60, 80) and GlyphAtlas.canvas_size("x" * 20) == (60, 880)
    # the kernings Pillow's BASIC layout applies are a few 1/64 px: "rn" by -1, "AV" by -3, "To" by -7
    kern = {(atlas.chars[a], atlas.chars[b]): int(v) for (a, b), v in zip(atlas.kern_pairs, atlas.kern_values)}
    assert (kern[("r", "n")], kern[("A", "V")], kern[("T", "o")]) == (-1, -3, -7)


def _pil_fonts():
    PIL = pytest.importorskip("PIL")
    from PIL import ImageFont, features
    if not features.check("freetype2"):
        pytest.skip("Pillow without FreeType")
    return PIL, ImageFont


def _pil_draw(font, text, size, origin):
    from PIL import Image, ImageDraw
    H, W = size
    img = Image.new("RGB", (W, H), (255, 255, 255))
    ImageDraw.Draw(img).text(tuple(origin), text, fill=(0, 0, 0), font=font)
    return np.asarray(img)


def _check_against_live_pillow(font, atlas):
    rng = random.Random(20240519)
    texts = ["".join(chr(rng.randint(32, 126)) for _ in range(rng.randint(1, 20))) for _ in range(200)]
    for t in texts + [c[1] for c in C.CASES]:
        size = C.canvas_size(t, None)
        assert np.array_equal(T.draw_text(atlas, t), _pil_draw(font, t, size, C.ORIGIN)), repr(t)
    for _, text, size, origin in C.CASES[7:9]:
        assert np.array_equal(T.draw_text(atlas, text, size, origin), _pil_draw(font, text, size, origin)), (text, origin)


def test_live_pillow_dejavu_rebuilds_the_fixture_and_matches_200_strings(golden, atlas):
    PIL, ImageFont = _pil_fonts()
    if not os.path.exists(C.FONT_PATH):
        pytest.skip(f"{C.FONT_PATH} is not installed")
    from diffute_amd.glyphs import GlyphAtlas
    built = GlyphAtlas.from_font(C.FONT_PATH, C.FONT_SIZE)
    for k in ("rec", "pool", "kern_pairs", "kern_values"):
        assert np.array_equal(getattr(built, k), getattr(atlas, k)), f"{k} differs from the fixture ({golden['versions']}, here Pillow {PIL.__version__})"
    assert built.chars == atlas.chars
    # a FreeTypeFont opened by the caller - with whatever layout engine - is reopened with BASIC
    assert np.array_equal(GlyphAtlas.from_font(ImageFont.truetype(C.FONT_PATH, 17), C.FONT_SIZE).pool, atlas.pool)
    _check_against_live_pillow(ImageFont.truetype(C.FONT_PATH, C.FONT_SIZE, layout_engine=ImageFont.Layout.BASIC), built)


def test_live_pillow_default_font_matches_200_strings():
    """ImageFont.load_default(size=40): Pillow's embedded font, BASIC layout, no font file needed"""
    _, ImageFont = _pil_fonts()
    from diffute_amd.glyphs import GlyphAtlas
    font = ImageFont.load_default(size=40)
    if not isinstance(font, ImageFont.FreeTypeFont):
        pytest.skip("this Pillow's default font is a bitmap font")
    _check_against_live_pillow(font, GlyphAtlas.from_font(font, 40))


def test_refusals_before_any_device_work(atlas):
    import torch
    from diffute_amd import glyphs, pipeline
    with pytest.raises(ValueError, match="U\\+00E9"):
        atlas.place("café")
    for bad in ("a\nb", "a\rb"):
        with pytest.raises(ValueError, match="line break"):
            atlas.place(bad)
        with pytest.raises(ValueError, match="line break"):
            atlas.canvas_size(bad)
    with pytest.raises(TypeError):
        glyphs.layout(atlas, "one string")
    with pytest.raises(ValueError, match="2 texts but 1 sizes"):
        glyphs.layout(atlas, ["a", "b"], sizes=[(60, 80)])

    class Renderer:                              # what the checks ask of glyph[0]: an atlas.  No device behind it.
        pass
    r = Renderer()
    r.atlas = atlas
    glyph = (r, object(), object())
    ctx = torch.zeros(3, 5, 8)
    pipeline._check_contexts(3, ctx)                                        # the existing form is unchanged
    pipeline._check_contexts(3, None, ["a", "b", ""], glyph)
    with pytest.raises(ValueError, match="3 boxes but 2 glyph contexts"):
        pipeline._check_contexts(3, ctx[:2])
    with pytest.raises(ValueError, match="exactly one"):
        pipeline._check_contexts(3, ctx, ["a", "b", "c"], glyph)
    with pytest.raises(ValueError, match="exactly one"):
        pipeline._check_contexts(3, None, None, glyph)
    with pytest.raises(ValueError, match="texts needs glyph"):
        pipeline._check_contexts(3, None, ["a", "b", "c"])
    with pytest.raises(ValueError, match="3 boxes but 2 texts"):
        pipeline._check_contexts(3, None, ["a", "b"], glyph)
    with pytest.raises(ValueError, match="3 boxes but one str"):
        pipeline._check_contexts(3, None, "abc", glyph)
    with pytest.raises(ValueError, match="triple"):
        pipeline._check_contexts(3, None, ["a", "b", "c"], (r, object()))
    with pytest.raises(ValueError, match="not in the atlas"):
        pipeline._check_contexts(3, None, ["a", "b", "é"], glyph)
    with pytest.raises(ValueError, match="line break"):
        pipeline._check_contexts(3, None, ["a", "b", "c\nd"], glyph)
    # the verified edits check their contexts through the same helper, before the labels
    with pytest.raises(ValueError, match="exactly one"):
        pipeline._check_verified_labels(None, 3, None, None, None, glyph)


@pytest.mark.parametrize("fault", ["max", "no_kerning", "truncate"])
def test_the_case_list_sees_an_injected_fault(golden, atlas, fault):
    changed = [name for name, text, size, origin in C.CASES
               if not np.array_equal(T.draw_text_grey(atlas, text, size, origin, fault=fault), golden["canvas." + name])]
    assert changed, f"no case notices the fault {fault!r}"
    assert {"max": "overlap", "no_kerning": "kerning_chain", "truncate": "subpixel_kerning"}[fault] in changed


def test_the_entries_refuse_bad_tables_on_the_host(atlas):
    """the C-ABI entries check the host copies of their tables before anything is launched, so the refusals need no device: the "device"
    pointers here are never read"""
    import ctypes
    from diffute_amd import _cabi, glyphs, prepost, processing
    lib = _cabi.lib()
    fake = 0x1000
    rec = np.ascontiguousarray(atlas.rec)

    def fused(text="rn m", size=384, mutate=None, max_taps=None, n_glyphs=None, pool_bytes=None):
        ip = processing.ViTImageProcessor(size=size)
        _, sizes, places, first, count = glyphs.layout(atlas, [text])
        passes, table, taps = prepost._readback_tables([(0, 0, w, h) for h, w in sizes], ip, 64)
        items = np.zeros(1, dtype=np.dtype(_cabi.GlyphTextItem))
        items["first"], items["count"], items["H"], items["W"] = first, count, sizes[0][0], sizes[0][1]
        for col, k in enumerate(("h_off", "h_taps", "v_off", "v_taps")):
            items[k] = passes[:, col]
        r = rec.copy()
        if mutate:
            mutate(items, places, r)
        a = _cabi.GlyphAtlas(pool=fake, pool_bytes=atlas.pool.size if pool_bytes is None else pool_bytes, glyphs_host=r.ctypes.data, glyphs_device=fake,
                             n_glyphs=len(atlas) if n_glyphs is None else n_glyphs)
        S_h, S_w = ip.size["height"], ip.size["width"]
        rc = lib.dmx_glyph_text_pixel_values(ctypes.byref(a), items.ctypes.data, fake, places.ctypes.data, fake, int(places.shape[0]), 1, fake,
                                             int(table.size), fake, taps if max_taps is None else max_taps, S_h, S_w, fake, None, None)
        err = lib.dmx_last_error().decode()
        # (glyph_render shares the table checks; its items carry no destination here, so it could not launch even with good tables)
        rc2 = lib.dmx_glyph_render(ctypes.byref(a), items.ctypes.data, fake, places.ctypes.data, fake, int(places.shape[0]), 1, None) if mutate else None
        return rc, err, rc2

    def setv(arr, field, value):
        def f(items, places, r):
            {"items": items, "places": places, "rec": r}[arr][field] = value
        return f

    cases = [(dict(max_taps=65), "exceed the cap of 64"), (dict(mutate=setv("items", "count", 5)), "end past the table"),
             (dict(mutate=setv("items", "first", -1)), "end past the table"), (dict(mutate=setv("places", (0, 0), 95)), "outside the atlas"),
             (dict(mutate=setv("places", (1, 1), 1 << 25)), "beyond"), (dict(mutate=setv("rec", (94, 1), 60000)), "outside the pool"),
             (dict(mutate=setv("items", "W", 0)), "bad canvas"), (dict(n_glyphs=0), "bad atlas"), (dict(pool_bytes=0), "bad atlas")]
    for kw, msg in cases:
        rc, err, rc2 = fused(**kw)
        assert rc == _cabi.ERR_ARG and msg in err, (kw, rc, err)
        if rc2 is not None and msg not in ("bad canvas",):
            assert rc2 == _cabi.ERR_ARG, (kw, rc2)
    rc, err, _ = fused(mutate=setv("items", "h_off", 1 << 20))
    assert rc == _cabi.ERR_ARG and "ends past" in err
    # the LDS budget: its own code, so that the caller can tell it from a bad argument and take the two-launch path
    rc, err, _ = fused(text="x" * 20, size={"height": 3, "width": 40})
    assert rc == _cabi.ERR_UNSUPPORTED and "36080 bytes of LDS, the budget is 32768" in err
