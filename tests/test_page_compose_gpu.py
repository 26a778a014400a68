"""The page composer on the GPU (csrc/page_compose.hip through diffute_amd/data.py), from tests/golden alone - no Pillow, no font: every
page bit for bit against the numpy restatement of the header's rule (tests/page_compose_restatement.py) AND against the page Pillow drew
(tests/golden/page_compose.npz), in both builds; HWC and planar strided destinations inside sentinel-filled buffers whose guard bytes
must survive; a page's bytes alone, in any batch and from run to run; the refusals of the C-ABI entry, which launch nothing."""
import ctypes

import numpy as np
import pytest
import torch

import page_compose_cases as C
import page_compose_restatement as T

pytestmark = pytest.mark.gpu

GUARD = 4096


@pytest.fixture(scope="module")
def ref():
    """the atlas, Pillow's pages and the restatement's pages of every case: computed once, read-only"""
    from diffute_amd.glyphs import GlyphAtlas
    atlas = GlyphAtlas.from_arrays(C.load_atlas_arrays(), "atlas.")
    g = C.load_golden()
    pages = {}
    for name, pg in C.CASES:
        pages[name] = T.compose(atlas, pg)
        pages[name].setflags(write=False)
        assert np.array_equal(pages[name], g["page." + name]), name
    return dict(atlas=atlas, pages=pages)


@pytest.fixture(params=["bf16", "fp16"])
def build(request, monkeypatch, cuda):
    """route every call of the test through one build of the library"""
    from diffute_amd import _cabi
    real = _cabi.lib
    real(request.param)
    monkeypatch.setattr(_cabi, "lib", lambda elem=None: real(request.param))
    return request.param


def _sizes(names):
    return [C.BY_ID[n]["size"] for n in names]


@pytest.mark.parametrize("names", [C.RAGGED, [n for n in C.CASE_IDS if n not in C.RAGGED], ["many"], ["empty"]],
                         ids=["ragged_p8", "the_other_16", "p1_many", "p1_no_lines"])
def test_hwc_pages_equal_pillow_and_the_restatement(cuda, build, ref, names):
    import diffute_amd as D
    from diffute_amd import data
    r = D.GlyphRenderer(ref["atlas"], cuda)
    recs = [C.BY_ID[n] for n in names]
    n = sum(h * w * 3 for h, w in _sizes(names))
    for sentinel in (0xA5, 0x5A):              # equal to the expected bytes under two different fills: every byte was written
        buf = torch.full((n + 2 * GUARD,), sentinel, dtype=torch.uint8, device=cuda)
        got = data.compose_pages(r, recs, out=buf[GUARD:GUARD + n])
        D.synchronize()
        assert bool((buf[:GUARD] == sentinel).all()) and bool((buf[GUARD + n:] == sentinel).all()), "guard band overwritten"
        assert len(got) == len(names) and got[0].data_ptr() == buf.data_ptr() + GUARD
        for name, img, (h, w) in zip(names, got, _sizes(names)):
            assert img.is_cuda and img.dtype == torch.uint8 and tuple(img.shape) == (h, w, 3)
            host = img.cpu().numpy()
            bad = np.argwhere(host != ref["pages"][name])
            assert bad.size == 0, f"{name}: {len(bad)} bytes differ from the restatement and Pillow, first at (y, x, c) = {bad[0]}"


def test_planar_and_strided_destinations_keep_their_guards(cuda, build, ref):
    """page k planar (CHW) with padded rows and padded planes, page k + 1 HWC with padded rows and a pixel stride of 4, in one buffer with
    guard bytes between and around them: every page byte is written, every other byte survives"""
    import diffute_amd as D
    from diffute_amd import data
    r = D.GlyphRenderer(ref["atlas"], cuda)
    names = ["grid_61x257", "partly_off", "grid_1x127", "overlap_ba", "clamp_255_6", "grid_61x128"]
    recs = [C.BY_ID[n] for n in names]
    layout, total = [], GUARD
    for k, (h, w) in enumerate(_sizes(names)):
        if k % 2 == 0:                          # planar: row pitch w + 5, plane pitch h * (w + 5) + 11
            sy, sx, sc = w + 5, 1, h * (w + 5) + 11
            span = 3 * sc
        else:                                   # interleaved: 4 bytes per pixel, row pitch 4 * w + 7
            sy, sx, sc = 4 * w + 7, 4, 1
            span = h * sy
        layout.append((total, sy, sx, sc, span))
        total += span + GUARD
    for sentinel in (0xA5, 0x5A):
        buf = torch.full((total,), sentinel, dtype=torch.uint8, device=cuda)
        assert data.compose_pages(r, recs, dst=[(buf.data_ptr() + o, sy, sx, sc) for o, sy, sx, sc, _ in layout]) is None
        D.synchronize()
        host = buf.cpu().numpy()
        written = np.zeros(total, dtype=bool)
        for name, (h, w), (o, sy, sx, sc, _) in zip(names, _sizes(names), layout):
            y, x, c = np.meshgrid(np.arange(h), np.arange(w), np.arange(3), indexing="ij")
            at = o + y * sy + x * sx + c * sc
            assert not written[at].any() and len(np.unique(at)) == at.size
            written[at] = True
            assert np.array_equal(host[at], ref["pages"][name]), f"{name}: page bytes differ"
        assert (host[~written] == sentinel).all(), "a byte outside the pages was written"


def test_a_page_is_the_same_alone_in_any_batch_and_from_run_to_run(cuda, build, ref):
    import diffute_amd as D
    from diffute_amd import data
    r = D.GlyphRenderer(ref["atlas"], cuda)
    names = C.RAGGED
    batch = data.compose_pages(r, [C.BY_ID[n] for n in names])
    again = data.compose_pages(r, [C.BY_ID[n] for n in names])
    back = data.compose_pages(r, [C.BY_ID[n] for n in names[::-1]])[::-1]
    alone = [data.compose_pages(r, [C.BY_ID[n]])[0] for n in names]
    pair = data.compose_pages(r, [C.BY_ID["inks"], C.BY_ID[names[2]], C.BY_ID["kerned"]])[1]
    D.synchronize()
    for k, n in enumerate(names):
        assert torch.equal(batch[k], again[k]) and torch.equal(batch[k], back[k]) and torch.equal(batch[k], alone[k]), n
        assert np.array_equal(batch[k].cpu().numpy(), ref["pages"][n]), n
    assert torch.equal(pair, batch[2])
    # SyntheticDocuments.compose is this call
    ds = D.SyntheticDocuments(r)
    assert all(torch.equal(a, b) for a, b in zip(ds.compose([C.BY_ID[n] for n in names]), batch))


def test_the_entry_refuses_before_it_launches(cuda, build, ref):
    """a placement range past the table, a line range past the table, a null destination, P = 0: an error code and the pages untouched;
    called directly with valid device tables, and the same call with good tables runs"""
    import diffute_amd as D
    from diffute_amd import _cabi, data
    lib = _cabi.lib()
    r = D.GlyphRenderer(ref["atlas"], cuda)
    names = ["overlap_ab", "empty"]
    recs = [C.BY_ID[n] for n in names]
    sizes = _sizes(names)
    starts = np.concatenate([[0], np.cumsum([h * w * 3 for h, w in sizes])])

    def call(mutate=None, P=2):
        pages, lines, places = data.page_tables(ref["atlas"], recs)
        out = torch.full((int(starts[-1]),), 0xA5, dtype=torch.uint8, device=cuda)
        pages["dst"], pages["stride_y"], pages["stride_x"], pages["stride_c"] = out.data_ptr() + starts[:-1], [w * 3 for _, w in sizes], 3, 1
        if mutate:
            mutate(pages, lines)
        d_pages, d_lines = torch.from_numpy(pages.view(np.uint8).copy()).to(cuda), torch.from_numpy(lines.view(np.uint8).copy()).to(cuda)
        d_places = torch.from_numpy(places.copy()).to(cuda)
        rc = lib.dmx_page_compose(ctypes.byref(r._atlas), pages.ctypes.data, _cabi.ptr(d_pages), P, lines.ctypes.data, _cabi.ptr(d_lines),
                                  int(lines.shape[0]), places.ctypes.data, _cabi.ptr(d_places), int(places.shape[0]), _cabi.current_stream())
        D.synchronize()
        return rc, out

    def line_count(pages, lines):
        lines["count"][1] = 7

    def page_lines(pages, lines):
        pages["n_lines"][0] = 3

    def null_dst(pages, lines):
        pages["dst"][1] = 0

    for kw, msg in ((dict(mutate=line_count), "placements .* end past the table"), (dict(mutate=page_lines), "lines .* end past the table"),
                    (dict(mutate=null_dst), "null destination"), (dict(P=0), "P = 0")):
        rc, out = call(**kw)
        assert rc == _cabi.ERR_ARG and bool((out == 0xA5).all()), kw
        with pytest.raises(RuntimeError, match=msg):
            _cabi.check(rc, "page_compose", lib)
    rc, out = call()
    assert rc == 0
    for k, n in enumerate(names):
        assert np.array_equal(out[int(starts[k]):int(starts[k + 1])].cpu().numpy().reshape(sizes[k] + (3,)), ref["pages"][n])
