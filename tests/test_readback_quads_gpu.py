"""The quad read-back (dmx_readback_pixel_values_quads[_persp]) and the quad select-paste (dmx_postprocess_paste_select_quads[_persp]) on the
GPU, both builds, both frames: bit for bit the chain of the EXISTING device entries they fuse, and bit for bit the numpy restatement
(tests/readback_quads_restatement.py).  Decoder outputs are drawn in [-1.2, 1.2], so the paste's clamp to a byte is exercised."""
import numpy as np
import pytest
import torch

import persp_cases as PC
import persp_restatement as PR
import quad_cases as QC
import quad_restatement as QR
import readback_quads_cases as C
import readback_quads_restatement as RQ
import readback_restatement as RR

pytestmark = pytest.mark.gpu

S, PAGES, K = C.S, C.PAGES, C.K
GUARD = 4096
BILINEAR, BICUBIC = 2, 3
PROCESSORS = {"bilinear_32": dict(size=32, resample=BILINEAR), "bicubic_24x40": dict(size={"height": 24, "width": 40}, resample=BICUBIC)}


def _case(perspective):
    from diffute_amd import _cabi
    names, quads, frames = C.lists(perspective)
    flat = [(p, n) for p, page in enumerate(names) for n in page]
    N = len(flat)
    rs = np.random.RandomState(20261021 + int(perspective))
    pages = [rs.randint(0, 256, (h, w, 3), dtype=np.uint8) for h, w in PAGES]
    vae = (rs.rand(N, 3, 3, S, S) * 2.4 - 1.2).astype(np.float32)                          # [N][3 candidates]; the read-back tests use the first K
    lib = _cabi.lib()
    if perspective:
        pt, qt, xt = PC.tables(PAGES, quads, frames)
        _cabi.check(lib.dmx_edit_quads_prepare(pt, len(PAGES), qt, N, S), "edit_quads_prepare")
        _cabi.check(lib.dmx_edit_quads_persp_prepare(pt, len(PAGES), qt, xt, N, S), "edit_quads_persp_prepare")
        pms = [PR.from_table(x) for x in xt]
    else:
        pt, qt = QC.tables(PAGES, quads, frames)
        _cabi.check(lib.dmx_edit_quads_prepare(pt, len(PAGES), qt, N, S), "edit_quads_prepare")
        pms = [None] * N
    qs = [QR.from_table(q) for q in qt]
    for a in pages + [vae]:
        a.setflags(write=False)
    return dict(perspective=perspective, flat=flat, N=N, pages=pages, vae=vae, quads=quads, frames=frames, qs=qs, pms=pms,
                page_of=[p for p, _ in flat], flat_quads=[q for page in quads for q in page], flat_frames=[f for page in frames for f in page])


@pytest.fixture(scope="module", params=[False, True], ids=["similarity", "projective"])
def case(request):
    """pages, decoder outputs, lists and the prepared integers of one frame kind: computed once, only read"""
    return _case(request.param)


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


def _guarded(shape, dtype, fill, cuda):
    """guard | tensor | guard in one sentinel-filled buffer -> (buffer, the tensor as a view)"""
    n = int(np.prod(shape))
    buf = torch.full((n + 2 * GUARD,), fill, dtype=dtype, device=cuda)
    return buf, buf[GUARD:GUARD + n].view(*shape)


def _guards_intact(buf, fill):
    return bool((buf[:GUARD] == fill).all()) and bool((buf[-GUARD:] == fill).all())


def _chain(D, ip, case, imgs, vae, rows):
    """rows [(b, k)] through the EXISTING device entries: postprocess_quads on a one-quad table -> rectify_quads -> the processor"""
    strips = []
    for b, k in rows:
        img, quad, frame, persp = imgs[case["page_of"][b]], case["flat_quads"][b], case["flat_frames"][b], case["perspective"]
        pasted = D.prepost.postprocess_quads(vae[b, k][None], [img], [[quad]], [[frame]], perspective=persp)
        strips += D.prepost.rectify_quads(pasted, [[quad]], perspective=persp)
    r = ip(images=strips, return_resized=True)
    return r.pixel_values, r.resized


@pytest.mark.parametrize("proc", sorted(PROCESSORS))
def test_readback_is_the_chain_of_existing_entries(cuda, build, case, proc):
    import diffute_amd as D
    ip = D.ViTImageProcessor(**PROCESSORS[proc])
    S_h, S_w, N = ip.size["height"], ip.size["width"], case["N"]
    imgs, vae = _dev(case["pages"], cuda), torch.from_numpy(case["vae"][:, :K].copy()).to(cuda)
    want_pv, want_u8 = _chain(D, ip, case, imgs, vae, [(b, k) for b in range(N) for k in range(K)])
    shape = (N * K, 3, S_h, S_w)
    for fill_f, fill_b in ((7.0e30, 0), (-7.0e30, 255)):          # an element nobody wrote shows under one fill or the other
        fbuf, out = _guarded(shape, torch.float32, fill_f, cuda)
        bbuf, res = _guarded(shape, torch.uint8, fill_b, cuda)
        got = D.prepost.readback_pixel_values_quads(vae, imgs, case["quads"], case["frames"], ip, perspective=case["perspective"], out=out,
                                                    out_resized=res)
        D.synchronize()
        assert got[0].data_ptr() == out.data_ptr() and got[1].data_ptr() == res.data_ptr()
        assert _guards_intact(fbuf, fill_f) and _guards_intact(bbuf, fill_b), "a guard band around the outputs was written"
        assert not bool((out == fill_f).any()), "an element of pixel_values was not written"
        bad = [(case["flat"][r // K][1], r % K) for r in range(N * K) if not torch.equal(out[r], want_pv[r]) or not torch.equal(res[r], want_u8[r])]
        assert not bad, f"rows (quad, k) differ from postprocess_quads -> rectify_quads -> processor: {bad}"
    plain = D.prepost.readback_pixel_values_quads(vae.reshape(N * K, 3, S, S), imgs, case["quads"], case["frames"], ip, perspective=case["perspective"])
    assert torch.equal(plain, want_pv), "the [N*K,3,S,S] form, tensors of its own, no resized bytes: the same pixel_values"


def test_readback_is_the_numpy_restatement(cuda, build, case):
    """two items per page - the added ones that take the other paths among them - against paste_page -> rectify -> Pillow's resample"""
    import diffute_amd as D
    ip = D.ViTImageProcessor(**PROCESSORS["bilinear_32"])
    imgs, vae = _dev(case["pages"], cuda), torch.from_numpy(case["vae"][:, :K].copy()).to(cuda)
    pv, res = D.prepost.readback_pixel_values_quads(vae, imgs, case["quads"], case["frames"], ip, perspective=case["perspective"], return_resized=True)
    D.synchronize()
    pv, res = pv.cpu().numpy(), res.cpu().numpy()
    by_name = {n: b for b, (_, n) in enumerate(case["flat"])}
    picks = ["skew_30_overlap" if not case["perspective"] else "overlap", "touches_border", "overhang", "off_its_crop", "thin", "rw_40_rh_24"]
    assert {case["page_of"][by_name[n]] for n in picks} == {0, 1, 2}
    for n in picks:
        b, k = by_name[n], 1
        want_u8, want_pv = RQ.readback(case["pages"][case["page_of"][b]], case["qs"][b], case["vae"][b, k], S, (32, 32), BILINEAR, case["pms"][b])
        assert np.array_equal(res[b * K + k], want_u8), f"{n}: the resized bytes differ from the restatement"
        assert np.array_equal(pv[b * K + k].view(np.uint32), want_pv.view(np.uint32)), f"{n}: pixel_values differ from the restatement"
    b = by_name["off_its_crop"]                                   # the case does what its name says: the strip holds original AND generated bytes
    pg, q, pm = case["pages"][case["page_of"][b]], case["qs"][b], case["pms"][b]
    strip, bare = RQ.strip(pg, q, case["vae"][b, 1], S, pm), RQ.rectify(pg, q, pm)
    same = (strip == bare).all(-1)
    assert same[:, :8].all() and same[:, -8:].all() and not same[:, strip.shape[1] // 2].any(), "the ends of the line lie off the crop, its middle on it"


def test_a_row_alone_and_in_the_batch_and_twice(cuda, build, case):
    import diffute_amd as D
    ip = D.ViTImageProcessor(**PROCESSORS["bilinear_32"])
    imgs, vae = _dev(case["pages"], cuda), torch.from_numpy(case["vae"][:, :K].copy()).to(cuda)
    args = (imgs, case["quads"], case["frames"], ip)
    first = D.prepost.readback_pixel_values_quads(vae, *args, perspective=case["perspective"])
    again = D.prepost.readback_pixel_values_quads(vae, *args, perspective=case["perspective"])
    assert torch.equal(first, again), "two runs differ"
    for b in range(case["N"]):
        alone = D.prepost.readback_pixel_values_quads(vae[b:b + 1], [imgs[case["page_of"][b]]], [[case["flat_quads"][b]]], [[case["flat_frames"][b]]], ip,
                                                      perspective=case["perspective"])
        assert torch.equal(alone, first[b * K:(b + 1) * K]), f"{case['flat'][b][1]}: the rows of a one-quad call differ from its rows in the batch"


def test_select_with_one_candidate_is_postprocess_quads(cuda, build, case):
    import diffute_amd as D
    imgs, vae = _dev(case["pages"], cuda), torch.from_numpy(case["vae"][:, :1].copy()).to(cuda)
    scores = torch.full((case["N"], 1), -3.5, device=cuda)
    want, want_union = D.prepost.postprocess_quads(vae[:, 0], imgs, case["quads"], case["frames"], return_mask=True, perspective=case["perspective"])
    got, choice, union = D.prepost.postprocess_select_quads(vae, scores, imgs, case["quads"], case["frames"], return_mask=True,
                                                            perspective=case["perspective"])
    D.synchronize()
    assert choice.dtype == torch.int32 and choice.tolist() == [0] * case["N"]
    for p in range(len(PAGES)):
        assert torch.equal(got[p], want[p]), f"page {p} differs from postprocess_quads"
        assert torch.equal(union[p], want_union[p]), f"union mask of page {p} differs from postprocess_quads"


def test_select_skips_transparently(cuda, build, case):
    """K = 3, hand-made scores, a threshold that skips the LATER quad of the overlapping pair of page 0"""
    import diffute_amd as D
    N, qs, pms, pages = case["N"], case["qs"], case["pms"], case["pages"]
    early, late = C.PERSP_OVERLAP if case["perspective"] else C.SIM_OVERLAP
    sc = np.random.RandomState(5).rand(N, 3).astype(np.float32) + 0.25              # all above the threshold of 0.125 ...
    sc[late] = [-0.5, 0.0, -2.0]                                                    # ... but the later quad's best
    sc[early] = [0.5, np.nan, 0.75]                                                 # a NaN never wins
    sc[3] = [np.nan, np.nan, np.nan]                                                # all NaN: candidate 0, not skipped
    sc[5] = [0.5, 0.875, 0.875]                                                     # a tie: the lowest k
    sc[6] = [np.nan, 0.0625, -1.0]                                                  # the best of the rest is below the threshold: skipped
    thr = 0.125
    want_choice = RR.select(sc, thr)
    assert want_choice[late] == -1 and want_choice[early] == 2 and want_choice[3] == 0 and want_choice[5] == 1 and want_choice[6] == -1
    imgs, vae = _dev(pages, cuda), torch.from_numpy(case["vae"].copy()).to(cuda)
    for fill in (0, 255):
        n = sum(h * w * 3 for h, w in PAGES) + GUARD * (len(PAGES) + 1)
        buf = torch.full((n,), fill, dtype=torch.uint8, device=cuda)
        views, guards, off = [], [], 0
        for h, w in PAGES:
            guards.append(slice(off, off + GUARD)); off += GUARD
            views.append(buf[off:off + h * w * 3].view(h, w, 3)); off += h * w * 3
        guards.append(slice(off, off + GUARD))
        got, choice, union = D.prepost.postprocess_select_quads(vae, torch.from_numpy(sc).to(cuda), imgs, case["quads"], case["frames"], threshold=thr,
                                                                return_mask=True, out=views, perspective=case["perspective"])
        D.synchronize()
        assert all(bool((buf[g] == fill).all()) for g in guards), "a guard band between the pages was written"
        assert choice.cpu().numpy().tolist() == want_choice.tolist()
        for p in range(len(PAGES)):
            mine = [b for b in range(N) if case["page_of"][b] == p]
            want = RQ.select_paste(pages[p], [qs[b] for b in mine], [case["vae"][b] for b in mine], sc[mine], thr, S,
                                   None if not case["perspective"] else [pms[b] for b in mine])
            host = got[p].cpu().numpy()
            assert np.array_equal(host, want["out"]), f"page {p} differs from the restatement"
            assert np.array_equal(union[p].cpu().numpy(), want["union"]), f"union mask of page {p} is not the OR of ALL its quads"
            outside = want["union"] == 0
            assert outside.sum() > 1000 and np.array_equal(host[outside], pages[p][outside]), "pixels outside every quad must be untouched"
    # page 0, pixel by pixel: where the skipped quad lies over the earlier one the earlier one shows; its own pixels are original
    host, un = got[0].cpu().numpy(), union[0].cpu().numpy()
    Y, X = np.mgrid[0:PAGES[0][0], 0:PAGES[0][1]]
    cov = [QR.inside(qs[b], X, Y) for b in range(N) if case["page_of"][b] == 0]
    both = cov[early] & cov[late]
    only_late = cov[late] & ~np.any([c for b, c in enumerate(cov) if b != late], axis=0)
    assert both.sum() > 50 and only_late.sum() > 50
    alone = RQ.pasted_alone(pages[0], qs[early], case["vae"][early, 2], S, pms[early])
    assert np.array_equal(host[both], alone[both]) and (host[both] != pages[0][both]).any(), "the earlier quad must show through the skipped one"
    assert np.array_equal(host[only_late], pages[0][only_late]), "the skipped quad's own pixels must stay original"
    assert un[cov[late]].all(), "the union mask must still cover the skipped quad"
