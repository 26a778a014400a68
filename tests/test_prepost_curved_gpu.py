"""Curved text regions on the GPU (csrc/prepost_curved.hip through prepost.preprocess_curved / postprocess_curved / rectify_curved)
against the restatement of csrc/prepost_curved.h (tests/curved_restatement.py, fed with the integers the prepare entry filled) - bit exact,
on both builds, at S = 32 and 64.  The cases are tests/curved_cases.py: nine polygons on three pages in one launch, n in {2, 3, 4, 7, 17} -
arcs of 90 and 270 degrees, an S-bend, a line read top to bottom, a region two pixel rows high, a cell one column long, a region on the
page's corner, a window overhanging its page, two overlapping regions.  The paste writes into views of one sentinel-filled slab with
guard bands."""
import numpy as np
import pytest
import torch

import curved_cases as CC
import curved_restatement as CR
import quad_restatement as QR

pytestmark = pytest.mark.gpu

N, PAGES = CC.N, CC.PAGES
GUARD = 4096


@pytest.fixture(scope="module")
def ref():
    """pages, decoder outputs, the prepared integers and the restatement's results per crop size, computed once and only read afterwards"""
    from diffute_amd import _cabi
    rs = np.random.RandomState(20261021)
    pages = [rs.randint(0, 256, (h, w, 3), dtype=np.uint8) for h, w in PAGES]
    polygons, frames = CC.lists()
    out = dict(pages=pages, polygons=polygons, frames=frames)
    for S in CC.SIZES:
        vae = (rs.standard_normal((N, 3, S, S)) * 0.6).clip(-1.3, 1.3).astype(np.float32)      # some values leave [-1, 1]
        pt, ct, xt = CC.tables(PAGES, polygons, frames)
        _cabi.check(_cabi.lib().dmx_edit_curved_prepare(pt, len(PAGES), ct, xt, N, S), "edit_curved_prepare")
        items = [CR.from_table(c, xt) for c in ct]
        pre = [CR.preprocess(pages[it["page"]], it, S) for it in items]
        pastes = []
        for p in range(len(PAGES)):
            mine = [b for b, it in enumerate(items) if it["page"] == p]
            pastes.append(CR.paste_page(pages[p], [items[b] for b in mine], [vae[b] for b in mine], S))
        out[S] = dict(vae=vae, items=items, pre=pre, pastes=pastes)
        for a in [vae] + [v for d in pre + pastes for v in d.values()]:
            a.setflags(write=False)
    out["strips"] = [CR.rectify(pages[it["page"]], it) for it in out[CC.S]["items"]]
    for a in pages + out["strips"]:
        a.setflags(write=False)
    return out


@pytest.fixture(params=["bf16", "fp16"])
def build(request, monkeypatch, cuda):
    """route every prepost call of the test through one build of the library"""
    from diffute_amd import _cabi
    real = _cabi.lib
    real(request.param)
    monkeypatch.setattr(_cabi, "lib", lambda elem=None: real(request.param))
    return request.param


def _dev(arrays, cuda):
    return [torch.from_numpy(np.ascontiguousarray(a).copy()).to(cuda) for a in arrays]


def _slab(fill, cuda, sizes=PAGES):
    """one sentinel-filled uint8 buffer: guard | page 0 | guard | page 1 | ... | guard -> (buffer, the pages as views, the guards' slices)"""
    n = sum(h * w * 3 for h, w in sizes) + GUARD * (len(sizes) + 1)
    buf = torch.full((n,), fill, dtype=torch.uint8, device=cuda)
    views, guards, off = [], [], 0
    for h, w in sizes:
        guards.append(slice(off, off + GUARD)); off += GUARD
        views.append(buf[off:off + h * w * 3].view(h, w, 3)); off += h * w * 3
    guards.append(slice(off, off + GUARD))
    return buf, views, guards


def test_reference_covers_what_the_cases_claim(ref):
    """the restatement's own results show the cases do what their names say (no GPU work)"""
    r = ref[CC.S]
    hit0 = r["pastes"][0]["hit"]
    Y, X = np.mgrid[0:PAGES[0][0], 0:PAGES[0][1]]
    both = CR.inside(r["items"][0], X, Y) & CR.inside(r["items"][1], X, Y)
    assert both.sum() > 100 and (hit0[both] == 1).all(), "arc90 and overlap overlap, and the later one decides there"
    assert all(p["pasted"].sum() > 0 for p in r["pastes"]) and all(0 < d["mask"].sum() < CC.S * CC.S for d in r["pre"])
    assert len(np.unique(r["pastes"][1]["piece"][r["pastes"][1]["hit"] == 0])) == 32, "every piece of arc270 pastes pixels of its own"
    assert (r["pastes"][2]["hit"] == 0).sum() >= 60, "two_rows has pixels of its own"


@pytest.mark.parametrize("S", CC.SIZES)
def test_preprocess_curved_rows(cuda, build, ref, S):
    import diffute_amd as D
    imgs = _dev(ref["pages"], cuda)
    got = D.prepost.preprocess_curved(imgs, ref["polygons"], ref["frames"], size=S)
    D.synchronize()
    assert sorted(got) == ["image", "mask", "mask_latent", "masked_image"]
    assert got["image"].shape == (N, 3, S, S) and got["masked_image"].shape == (N, 3, S, S) and got["image"].dtype == torch.float32
    assert got["mask"].shape == (N, 1, S, S) and got["mask"].dtype == torch.uint8 and got["mask_latent"].shape == (N, 1, S // 8, S // 8)
    host = {k: v.cpu().numpy() for k, v in got.items()}
    for b, (p, (name, _, _, _)) in enumerate(CC.FLAT):
        want = ref[S]["pre"][b]
        for k in ("image", "masked_image"):
            assert np.array_equal(host[k][b].view(np.uint32), want[k].view(np.uint32)), f"{name}: {k} of row {b} (page {p}) differs from the restatement"
        for k in ("mask", "mask_latent"):
            assert np.array_equal(host[k][b, 0], want[k]), f"{name}: {k} of row {b} (page {p}) differs from the restatement"


@pytest.mark.parametrize("S", CC.SIZES)
def test_postprocess_curved_pages_and_union_masks(cuda, build, ref, S):
    import diffute_amd as D
    imgs, vae = _dev(ref["pages"], cuda), torch.from_numpy(ref[S]["vae"].copy()).to(cuda)
    for fill in (0, 255):                                  # a byte nobody wrote shows under one fill or the other
        buf, views, guards = _slab(fill, cuda)
        got, unions = D.prepost.postprocess_curved(vae, imgs, ref["polygons"], ref["frames"], return_mask=True, out=views)
        D.synchronize()
        assert all(g.data_ptr() == v.data_ptr() for g, v in zip(got, views))
        assert all(bool((buf[g] == fill).all()) for g in guards), "a guard band between the pages was written"
        for p, want in enumerate(ref[S]["pastes"]):
            host = got[p].cpu().numpy()
            assert host.shape == PAGES[p] + (3,) and got[p].dtype == torch.uint8
            assert np.array_equal(host, want["out"]), f"page {p} differs from the restatement"
            assert np.array_equal(unions[p].cpu().numpy(), want["union"]), f"union mask of page {p} differs from the OR of the polygons"
            # the region, once more from the predicate alone: outside every polygon the page is the input
            Y, X = np.mgrid[0:PAGES[p][0], 0:PAGES[p][1]]
            region = np.zeros(PAGES[p], bool)
            for it in ref[S]["items"]:
                if it["page"] == p:
                    region |= CR.inside(it, X, Y)
            assert np.array_equal(region, want["union"] == 1)
            assert (~region).sum() > 1000 and np.array_equal(host[~region], ref["pages"][p][~region]), "pixels outside every polygon must be untouched"
            assert (host[want["pasted"]] != ref["pages"][p][want["pasted"]]).any()
    plain = D.prepost.postprocess_curved(vae, imgs, ref["polygons"], ref["frames"])     # pages of its own, no mask: the same bytes
    assert all(torch.equal(a, b) for a, b in zip(plain, got))


def test_rectify_curved_strips(cuda, build, ref):
    import diffute_amd as D
    imgs = _dev(ref["pages"], cuda)
    got = D.prepost.rectify_curved(imgs, ref["polygons"])
    D.synchronize()
    assert len(got) == N and all(t.dtype == torch.uint8 and t.is_cuda and t.is_contiguous() for t in got)
    base = got[0].data_ptr()
    for b, (t, want, it) in enumerate(zip(got, ref["strips"], ref[CC.S]["items"])):
        assert t.data_ptr() - base == it["rect_off"], "the strips are views of one buffer, packed in item order"
        assert tuple(t.shape) == (it["rh"], it["rw"], 3) and np.array_equal(t.cpu().numpy(), want), f"{CC.FLAT[b][1][0]}: strip {b} differs from the restatement"
    # an axis-aligned rectangle, whole and in three cells, is the page slice, both corners included
    rect = CC.box(20, 30, 70, 44)
    cut = [(20, 30), (33, 30), (34, 30), (70, 30), (70, 44), (34, 44), (33, 44), (20, 44)]
    for poly in (rect, cut):
        strip, = D.prepost.rectify_curved(imgs[:1], [[poly]])
        assert torch.equal(strip, imgs[0][30:45, 20:71]), f"{len(poly)} points"


def test_parallelograms_equal_the_projective_quads(cuda, build, ref):
    """n = 2 parallelograms, and a parallelogram cut at whole-number cell lengths, give the crop, masked image, masks, pasted page and
    strip of preprocess_quads / postprocess_quads / rectify_quads with perspective=True, bit for bit"""
    import diffute_amd as D
    P = D.prepost
    S = CC.S
    rs = np.random.RandomState(5)
    page = torch.from_numpy(rs.randint(0, 256, CC.PARA_PAGE + (3,), dtype=np.uint8)).to(cuda)
    quads = [CC.PARA, [(30, 100), (90, 104), (88, 116), (28, 112)]]
    polys = [CC.PARA_CUT, quads[1]]
    rw, rh = CC.strip_size(CC.PARA)
    frames = [(rw - 1, rh - 1, 120), CC.frame_of(quads[1], 70)]
    vae = torch.from_numpy((rs.standard_normal((2, 3, S, S)) * 0.6).astype(np.float32)).to(cuda)
    for mine in (polys, quads):                             # the cut parallelogram beside an n = 2 one, then both as n = 2
        a, b = P.preprocess_curved([page], [mine], [frames], size=S), P.preprocess_quads([page], [quads], [frames], size=S, perspective=True)
        assert all(torch.equal(a[k], b[k]) for k in b), "crop, masked image or mask differ"
        (pa,), (ua,) = P.postprocess_curved(vae, [page], [mine], [frames], return_mask=True)
        (pb,), (ub,) = P.postprocess_quads(vae, [page], [quads], [frames], return_mask=True, perspective=True)
        assert torch.equal(pa, pb) and torch.equal(ua, ub) and not torch.equal(pa, page), "the pasted pages differ"
        sa, sb = P.rectify_curved([page], [mine]), P.rectify_quads([page], [quads], perspective=True)
        assert all(torch.equal(x, y) for x, y in zip(sa, sb)), "the strips differ"
    D.synchronize()


def test_a_quarter_turn_of_pages_and_polygons(cuda, build, ref):
    """np.rot90 of every page with its polygons turned along (the frames live in strip space and stay), in one launch each: the crops,
    masks and strips are identical and the pasted page is the turned pasted page, bit for bit"""
    import diffute_amd as D
    P = D.prepost
    S = CC.S
    imgs, vae = _dev(ref["pages"], cuda), torch.from_numpy(ref[S]["vae"].copy()).to(cuda)
    timgs = _dev([QR.rot90_page(p) for p in ref["pages"]], cuda)
    tpolys = [[QR.rot90_corners(c, w) for c in cs] for cs, (h, w) in zip(ref["polygons"], PAGES)]
    a = P.preprocess_curved(imgs, ref["polygons"], ref["frames"], size=S)
    b = P.preprocess_curved(timgs, tpolys, ref["frames"], size=S)
    assert all(torch.equal(a[k], b[k]) for k in a), "the crops of the turned pages differ"
    sa, sb = P.rectify_curved(imgs, ref["polygons"]), P.rectify_curved(timgs, tpolys)
    assert all(torch.equal(x, y) for x, y in zip(sa, sb)), "the strips of the turned pages differ"
    pa, ua = P.postprocess_curved(vae, imgs, ref["polygons"], ref["frames"], return_mask=True)
    pb, ub = P.postprocess_curved(vae, timgs, tpolys, ref["frames"], return_mask=True)
    D.synchronize()
    for p in range(len(PAGES)):
        assert np.array_equal(np.rot90(ua[p].cpu().numpy()), ub[p].cpu().numpy())
        assert np.array_equal(np.rot90(pa[p].cpu().numpy()), pb[p].cpu().numpy()), f"page {p}: the pasted turned page is not the turned pasted page"


class _Recorder:
    """the library, noting the name of every dmx_* function called through it"""

    def __init__(self, lib, names):
        self._lib, self._names = lib, names

    def __getattr__(self, name):
        fn = getattr(self._lib, name)
        if not name.startswith("dmx_"):
            return fn

        def call(*args):
            self._names.append(name)
            return fn(*args)
        return call


def test_one_prepare_and_one_launch_per_call(cuda, build, ref, monkeypatch):
    import diffute_amd as D
    from diffute_amd import _cabi
    names = []
    rec = _Recorder(_cabi.lib(), names)
    monkeypatch.setattr(_cabi, "lib", lambda elem=None: rec)
    S = CC.S
    imgs, vae = _dev(ref["pages"], cuda), torch.from_numpy(ref[S]["vae"].copy()).to(cuda)
    Q, F = ref["polygons"], ref["frames"]
    calls = [("dmx_preprocess_curved", lambda: D.prepost.preprocess_curved(imgs, Q, F, size=S)),
             ("dmx_postprocess_paste_curved", lambda: D.prepost.postprocess_curved(vae, imgs, Q, F, return_mask=True)),
             ("dmx_rectify_curved", lambda: D.prepost.rectify_curved(imgs, Q)),
             ("dmx_preprocess_curved", lambda: D.prepost.preprocess_curved(imgs[:1], Q[:1], F[:1], size=S))]      # one page is P = 1
    for entry, fn in calls:
        del names[:]
        fn()
        assert names == ["dmx_edit_curved_prepare", entry], entry
    del names[:]
    planned = D.prepost.preprocess_curved(imgs, Q, None, size=S)                 # frames None: planned on the host, then the same two
    assert names[-2:] == ["dmx_edit_curved_prepare", "dmx_preprocess_curved"]
    assert set(names[:-2]) <= {"dmx_edit_curved_prepare", "dmx_last_error"} and planned["image"].shape == (N, 3, S, S)
    D.synchronize()


def test_refusals_launch_nothing(cuda, ref):
    """a concave cell, a strip one pixel high, a missing frame, an odd point count and a host table spoiled after the prepare: an error
    naming the item, and the sentinel-filled outputs stay as they were"""
    from diffute_amd import _cabi, prepost
    S = CC.S
    imgs, vae = _dev(ref["pages"], cuda), torch.from_numpy(ref[S]["vae"].copy()).to(cuda)
    buf, views, guards = _slab(0x5A, cuda)
    polygons, frames = ref["polygons"], ref["frames"]

    def swap(p, j, pts, frame):
        qs, fs = [list(q) for q in polygons], [list(f) for f in frames]
        qs[p][j], fs[p][j] = pts, frame
        return qs, fs
    cases = [(swap(0, 1, CC.CONCAVE, (20, 10, 64)), "item 1: cell 0"), (swap(2, 0, CC.FLAT_STRIP, (20, 1, 64)), "item 6"),
             (swap(1, 1, polygons[1][1], (90, 14, 0)), "item 5")]
    for (q, f), word in cases:
        with pytest.raises(RuntimeError, match=word):
            prepost.postprocess_curved(vae, imgs, q, f, out=views)
        with pytest.raises(RuntimeError, match=word):
            prepost.preprocess_curved(imgs, q, f, size=S)
    for (q, f), word in cases[:2]:                         # the strips read no frame
        with pytest.raises(RuntimeError, match=word):
            prepost.rectify_curved(imgs, q)
    with pytest.raises(ValueError, match="odd point count"):
        prepost.preprocess_curved(imgs, *swap(0, 0, CC.ODD, (20, 10, 64)), size=S)
    with pytest.raises(ValueError, match="page 1: polygon 1"):
        prepost.preprocess_curved(imgs, polygons, [frames[0], [frames[1][0], None], frames[2]], size=S)
    # the launch entries themselves, with real addresses and good device tables: only the host tables are spoiled
    lib = _cabi.lib()
    cx = prepost._check_curved(imgs, polygons, frames)
    strips = torch.full((1 << 16,), 0x5A, dtype=torch.uint8, device=cuda)
    pre_out = [torch.full((N * 3 * S * S,), 3.0, device=cuda), torch.full((N * 3 * S * S,), 3.0, device=cuda),
               torch.full((N * S * S,), 0x5A, dtype=torch.uint8, device=cuda), torch.full((N * 64,), 3.0, device=cuda)]
    for spoil in ("map", "item", "page"):
        host, pages, pieces, stage, dbuf, off, xoff = prepost._upload_curved(cx, S, views, None)
        if spoil == "map":
            pieces[host[5].piece_lo + 1].strip.t[0] += 1
            pieces[host[5].piece_lo + 1].crop.t[2] += 1
        elif spoil == "item":
            host[5].x[0] = 150                                 # the first column right of page 1
        else:
            pages[1].W = 300                                   # another tile count: the blocks no longer belong to the table
        base, word = dbuf.data_ptr(), ("page 1" if spoil == "page" else "item 5")
        assert lib.dmx_postprocess_paste_curved(_cabi.ptr(vae), S, pages, base + off, 3, host, base, pieces, base + xoff, N, _cabi.current_stream()) == -1
        assert word in lib.dmx_last_error().decode()
        assert lib.dmx_preprocess_curved(pages, base + off, 3, host, base, pieces, base + xoff, N, S, *(_cabi.ptr(t) for t in pre_out),
                                         _cabi.current_stream()) == -1
        assert word in lib.dmx_last_error().decode()
        assert lib.dmx_rectify_curved(pages, base + off, 3, host, base, pieces, base + xoff, N, _cabi.ptr(strips), strips.numel(),
                                      _cabi.current_stream()) == -1
        assert word in lib.dmx_last_error().decode()
    _cabi.synchronize()
    assert bool((buf == 0x5A).all()) and bool((strips == 0x5A).all()) and bool((pre_out[2] == 0x5A).all()), "refused, yet something was written"
    assert all(bool((t == 3.0).all()) for t in (pre_out[0], pre_out[1], pre_out[3]))


def test_the_strip_of_an_arc_on_a_radial_ramp_is_straight(cuda, build):
    """the page's value is a linear ramp in the distance from a centre, the region an arc band about that centre in M = 6 cells: every row
    of the strip is flat within tests/curved_cases.ramp_bound, 3.79 grey levels.  The same band as ONE quad, through the projective strip,
    exceeds that in every row: the comparison can fail"""
    import diffute_amd as D
    page = torch.from_numpy(CC.ramp_page()).to(cuda)
    bound = CC.ramp_bound(CC.RAMP_M)
    strip, = D.prepost.rectify_curved([page], [[CC.RAMP_ARC]])
    bent, = D.prepost.rectify_quads([page], [[CC.RAMP_QUAD]], perspective=True)
    D.synchronize()
    spread, wide = CC.row_spread(strip.cpu().numpy()), CC.row_spread(bent.cpu().numpy())
    print(f"row spread of the straightened arc: max {spread.max()} levels (bound {bound:.2f}); as one quad: min {wide.min()}, max {wide.max()}")
    assert strip.shape[0] == 21 and spread.max() <= bound, f"the strip is bent: a row spreads over {spread.max()} levels, bound {bound:.2f}"
    assert wide.min() > bound, "one quad leaves the arc's bend in the strip"
