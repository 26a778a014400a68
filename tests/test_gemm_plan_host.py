"""The GEMM planner (csrc/gemm_plan.hip) and the launch shape of every tile instance (csrc/gemm_tile.h), pinned without a GPU.

`dmx_test_gemm_plan` runs dmx_conv_gemm's argument checks, the planner and the launch-shape arithmetic for a descriptor on a device of a
given CU count and makes no device call.  tests/golden/gemm_plans.npz holds what the code planned and launched BEFORE the planner was
split out of gemm.hip (recorded through the same entry patched onto that commit), so a change of the instance table, the LDS layout or
the cost model that moves any plan shows here as an exact mismatch.  Adding an instance adds its rows to the golden file (record()).
"""
import ctypes
import itertools
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "gemm_plans.npz")
N_CUS = 256
FIELDS = ("rc", "cfg", "splitk", "kt_per_split", "tiles_n", "persist_blocks", "workspace_bytes", "grid_x", "grid_y", "threads",
          "lds_bytes", "lds_bytes_prefetch", "colstats_ok")

MS = (64, 256, 1024, 4096, 16384)
NS = (4, 64, 320, 640, 1280, 2560, 10240)
KS = (128, 320, 1280, 2880, 5760, 11520)
FLAVOURS = ("plain", "3x3", "stride2", "ups", "ups2", "shortcut")
EPILOGUES = ("none", "geglu", "ln_stats", "rowstats_out", "act", "out_f32", "colstats")
FORCE_TN = tuple(range(17))
FORCE_SPLITK = (0, 1, 3)
OVERRIDES = ((10, 1), (0, 2), (3, 1), (12, 1))          # (cfg, splitk) set on each of the first four tuned rows: 160-column, split, retired, persistent

_buf = ctypes.create_string_buffer(64)                  # what every pointer of a descriptor points at: the planner reads through none of them
_PTR = ctypes.addressof(_buf)


def make_desc(M, N, K, flavour, epilogue):
    """the descriptor of an M x N x K problem, or None where the flavour has no such K (a 3x3 conv needs K = 9 Cin)"""
    from diffute_amd import _cabi
    d = _cabi.GemmDesc()
    d.x0 = d.w = d.out = _PTR
    d.M, d.N, d.K = M, N, K
    d.ksize, d.stride, d.pad = 3, 1, 1
    d.OH, d.OW = 1, M                                   # the plan depends on the grid only through M
    d.IH, d.IW = d.OH, d.OW
    shortcut = 0
    if flavour == "plain":
        d.direct, d.ksize, d.pad, cin = 1, 1, 0, K
    elif flavour == "ups2":                             # the phase-decomposed upsample conv, as dmx_conv_ups2x describes it: K = 4 Cin, M = 4 rows per source pixel
        if M % 4:
            return None
        d.ups, d.ksize, d.pad, cin = 2, 2, 0, K // 4
        d.OW = d.IW = M // 4
    elif flavour == "shortcut":                         # conv3x3 + the 1x1 shortcut of a ResnetBlock2D as a second K segment: K = 9 Cin + Cin
        if K % 10:
            return None
        cin = shortcut = K // 10
        d.s0, d.lds0, d.cs0 = _PTR, cin, cin
    else:
        if K % 9:
            return None
        cin = K // 9
        if flavour == "stride2":
            d.stride, d.IW = 2, 2 * M
        elif flavour == "ups":
            d.ups = 1
    d.Cin = d.cx0 = d.ldx0 = cin
    d.Ktaps = K - shortcut
    d.ldw, d.ldo, d.rows_per_group = K, N, 1
    d.bias = _PTR
    d.cs_rows = M // 4 if flavour == "ups2" else M      # one sample: dmx_conv_gemm_colstats_ok has something to say for every descriptor
    if epilogue == "geglu":
        d.geglu = 1
    elif epilogue == "ln_stats":
        d.ln_stats = d.ln_c1 = d.ln_c2 = _PTR
        d.ln_tiles, d.ln_C, d.ln_eps = 1, K, 1e-5
    elif epilogue == "rowstats_out":
        d.rowstats_out = _PTR
    elif epilogue == "act":
        d.act = 1
    elif epilogue == "out_f32":
        d.out_f32 = 1
    elif epilogue == "colstats":
        d.colstats = _PTR
    return d


def tuned_rows():
    src = open(os.path.join(ROOT, "diffute_amd", "csrc", "gemm_tuned.h")).read()
    rows = [tuple(int(v) for v in m.groups()) for m in re.finditer(r"^\s*\{(\d+), (\d+), (\d+), (\d+), (\d+), (\d+), (\d+), (\d+)\},", src, re.M)]
    assert len(rows) > 150 and rows[0][:3] == (0, 0, 0)
    return rows


def tuned_desc(row):
    M, N, K, _, st, ups, _, _ = row                     # (the table is keyed on M, N, K, stride and ups alone)
    flavour = "ups2" if ups == 2 else "ups" if ups == 1 else "stride2" if st == 2 else "plain"
    return make_desc(M, N, K, flavour, "none")


def plan_all(lib):
    """every descriptor of the set, in a fixed order -> int64 [rows][len(FIELDS)]"""
    out, row = [], (ctypes.c_longlong * 12)()

    def plan(d):
        rc = lib.dmx_test_gemm_plan(ctypes.byref(d), N_CUS, row)
        out.append((rc,) + tuple(row))

    rows = tuned_rows()
    for r in rows:
        plan(tuned_desc(r))
    for M, N, K, fl, ep in itertools.product(MS, NS, KS, FLAVOURS, EPILOGUES):
        d = make_desc(M, N, K, fl, ep)
        if d is None:
            continue
        for d.force_tn, d.force_splitk in itertools.product(FORCE_TN, FORCE_SPLITK):
            plan(d)
    try:
        for r in [r for r in rows if r[0]][:4]:
            d = tuned_desc(r)
            for cfg, sk in OVERRIDES:
                lib.dmx_gemm_plan_override(r[0], r[1], r[2], r[4], r[5], cfg, sk)
                plan(d)
            lib.dmx_gemm_plan_override(0, 0, 0, 0, 0, -1, 0)
            plan(d)
    finally:
        lib.dmx_gemm_plan_override(0, 0, 0, 0, 0, -1, 0)
    return np.array(out, dtype=np.int64)


def record(path=GOLDEN):
    """(re)write the golden file from the loaded library: one array per field, in its smallest integer type"""
    from diffute_amd import _cabi
    got = plan_all(_cabi.lib())
    cols = {}
    for i, f in enumerate(FIELDS):
        c = got[:, i]
        cols[f] = c.astype(next(t for t in (np.int8, np.int16, np.int32, np.int64) if np.array_equal(c.astype(t), c)))
    np.savez_compressed(path, **cols)
    return got.shape[0]


def test_plans_and_launch_shapes_match_the_recorded_ones():
    from diffute_amd import _cabi
    golden = np.load(GOLDEN)
    assert tuple(golden.files) == FIELDS
    got = plan_all(_cabi.lib())
    assert got.shape[0] == golden["rc"].shape[0] > 100000
    for i, f in enumerate(FIELDS):
        bad = np.nonzero(got[:, i] != golden[f].astype(np.int64))[0]
        assert bad.size == 0, f"{f}: {bad.size} of {got.shape[0]} descriptors differ, first at row {bad[0]}: got {got[bad[0]].tolist()}, recorded {[int(golden[g][bad[0]]) for g in FIELDS]}"
    # the set is worth its name: every live instance, split-K and persistent plans, refusals, and statistics both allowed and not
    ok = got[:, 0] == 0
    assert set(np.unique(got[ok, 1])) == {0, 1, 2, 6, 7, 8, 9, 10, 11, 12, 14, 15} and (~ok).any() and set(np.unique(got[~ok, 0])) == {-1}
    assert (got[ok, 2] > 1).any() and (got[ok, 5] > 0).any() and set(np.unique(got[ok, 12])) == {0, 1}
