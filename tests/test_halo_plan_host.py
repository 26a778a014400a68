"""The halo-conv planner (csrc/conv_halo_plan.hip) and the launch shape of every tile instance (csrc/halo_tile.h), pinned without a GPU.

`dmx_test_halo_plan` runs dmx_conv3x3_gn's argument checks and its plan for a descriptor on a device of a given CU count under given settings
of the three switches the plan reads (exclusive device, peers on one XCD, warp-specialised instances) and makes no device call.
tests/golden/halo_plans.npz holds what the code planned and launched BEFORE the planner was split out of conv_halo.hip (recorded through the
same entry patched onto that commit, for the bf16 and the fp16 build: their instance sets differ), so a change of the instance table, the
LDS layout, the cost model or the block decode that moves any plan shows here as an exact mismatch.  Adding an instance adds its rows to the
golden file (record()).
"""
import ast
import ctypes
import itertools
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "halo_plans.npz")
ELEMS = ("bf16", "fp16")
FIELDS = ("rc", "TH", "TW", "bn", "waves", "splits", "blocks", "threads", "lds_bytes", "flag_count", "workspace_bytes", "xcd_tile_major", "peers_local",
          "tiles_x", "tiles_img", "tiles_m", "ncombo", "cpg", "mg_tiles_x", "mg_tiles_img", "mg_tiles_m", "mg_ncombo", "mg_pw", "mg_cpg")
ERR_ARG = -1

BS = (1, 2, 4, 8)
HWS = ((8, 32), (16, 16), (16, 32), (32, 32), (48, 48), (64, 64), (96, 96), (128, 128), (24, 24), (20, 32))   # 48x48: only the 16x16 tile fits; the last two: none
CINS = (64, 128, 320, 640, 1280, 1920, 2560)
CSCS = (0, 64, 320, 640)
NS = (64, 80, 128, 160, 256, 320, 640, 1280, 96)       # 96: no column tile divides it
FORCE_SPLIT = (0, 1, 2, 3, 4, 8, 16)
FORCE_BN = (0, 160, 128, 80, 64, 96)
FORCE_WAVES = (0, 4, 8, 12, 5)
N_CUS = (256, 64)
SWITCHES = tuple(itertools.product((1, 0), repeat=3))   # (exclusive, peers, ws)

_buf = ctypes.create_string_buffer(64)                  # what every pointer of a descriptor points at: the planner reads through none of them
_PTR = ctypes.addressof(_buf)


def make_desc(B, H, W, Cin, N, Csc=0, x_split=0, s_split=0, gn=1):
    """x_split / s_split: 0 = one source, 1 = two sources cut at the multiple of 64 nearest below the middle (at least 64), 2 = cut at 32 (refused);
    gn: 0 = plain conv, 1 = GroupNorm(32) + SiLU in front, 2 = 16 groups (refused)"""
    from diffute_amd import _cabi
    d = _cabi.HaloConvDesc()
    d.x0 = d.w = d.out = d.bias = _PTR
    d.B, d.H, d.W, d.Cin, d.N, d.ldo = B, H, W, Cin, N, N
    d.cx0 = d.ldx0 = Cin
    if x_split:
        d.cx0 = d.ldx0 = 32 if x_split == 2 else max(64, Cin // 128 * 64)
        d.x1, d.ldx1 = _PTR, max(Cin - d.cx0, 8)
    if Csc:
        d.s0, d.Csc, d.cs0, d.lds0 = _PTR, Csc, Csc, Csc
        if s_split:
            d.cs0 = d.lds0 = 32 if s_split == 2 else max(64, Csc // 128 * 64)
            d.s1, d.lds1 = _PTR, max(Csc - d.cs0, 8)
    d.ldw = 9 * Cin + Csc
    if gn:
        d.gn, d.silu, d.groups, d.eps = 1, 1, 32 if gn == 1 else 16, 1e-5
        d.st0 = d.st1 = d.gamma = d.beta = _PTR
    return d


def descriptors():
    """(descriptor, n_cus, exclusive, peers, ws) of the set, in a fixed order.  The full product of the axes above is ~10^11 rows; these are its
    slices: every shape under every environment, every force on the shapes of the UNet / VAE levels, every argument variant on a few shapes."""
    # 1. the plan nobody forces: every shape, both devices, every setting of the switches
    for B, (H, W), Cin, Csc, N in itertools.product(BS, HWS, CINS, (0, 320), NS):
        d = make_desc(B, H, W, Cin, N, Csc)
        for n_cus, (ex, peers, ws) in itertools.product(N_CUS, SWITCHES):
            yield d, n_cus, ex, peers, ws
    # 2. every force, alone and combined, on one shape per level (the first four are the UNet's at 512 px, batch 4) and a 16x16-tile shape
    for (B, (H, W), Cin), N in itertools.product(((4, (64, 64), 320), (4, (32, 32), 640), (4, (16, 16), 1280), (4, (128, 128), 320), (1, (128, 128), 128),
                                                  (2, (48, 48), 640), (8, (16, 32), 1920), (1, (8, 32), 2560)), (128, 160, 320, 640, 1280, 96)):
        d = make_desc(B, H, W, Cin, N)
        for d.force_split, d.force_bn, d.force_waves in itertools.product(FORCE_SPLIT, FORCE_BN, FORCE_WAVES):
            for n_cus, ws in itertools.product(N_CUS, (1, 0)):
                yield d, n_cus, 1, 1, ws
            yield d, 256, 0, 0, 1
    # 3. every argument variant: source splits (a cut at 32 is refused), shortcut widths and their splits, GroupNorm on / off / 16 groups (refused)
    for B, (H, W), Cin, Csc, N in itertools.product((1, 4), ((16, 16), (32, 32), (64, 64), (20, 32)), CINS, CSCS, (160, 640, 1280, 256)):
        for x_split, s_split, gn in itertools.product((0, 1, 2), (0, 1, 2) if Csc else (0,), (0, 1, 2)):
            d = make_desc(B, H, W, Cin, N, Csc, x_split, s_split, gn)
            for d.force_split in (0, 2, 8):
                yield d, 256, 1, 1, 1
    # 4. more blocks x pixel tiles than the kernel's 32-bit block decode divides exactly (2^19 blocks x 2^16 tiles): refused
    yield make_desc(64, 512, 512, 320, 1280), 256, 1, 1, 1


def plan_all(lib):
    """every descriptor of the set -> int64 [rows][len(FIELDS)]"""
    out, row = [], (ctypes.c_longlong * (len(FIELDS) - 1))()
    fn = lib.dmx_test_halo_plan
    for d, n_cus, ex, peers, ws in descriptors():
        rc = fn(ctypes.byref(d), n_cus, ex, peers, ws, row)
        out.append((rc,) + tuple(row))
    return np.array(out, dtype=np.int64)


def record(libs, path=GOLDEN):
    """(re)write the golden file from {element type: loaded library}: one array per build and field, in its smallest integer type"""
    cols = {}
    for elem in ELEMS:
        got = plan_all(libs[elem])
        for i, f in enumerate(FIELDS):
            c = got[:, i]
            cols[f"{elem}_{f}"] = c.astype(next(t for t in (np.int8, np.int16, np.int32, np.int64) if np.array_equal(c.astype(t), c)))
    np.savez_compressed(path, **cols)
    return got.shape[0]


def table_rows():
    """(id, bn, waves, builds) of every DMX_HALO_INSTANCES row of halo_tile.h"""
    src = open(os.path.join(ROOT, "diffute_amd", "csrc", "halo_tile.h")).read()
    rows = [(int(m[1]), int(m[2]), int(m[3]), m[4]) for m in re.finditer(r"^\s*ROW\((\d+), (\d+), (\d+), \d+, \d+, \d+, (?:true|false), (\w+),", src, re.M)]
    assert [r[0] for r in rows] == list(range(len(rows))) and len(rows) >= 8
    return rows


@pytest.mark.parametrize("elem", ELEMS)
def test_plans_and_launch_shapes_match_the_recorded_ones(elem):
    from diffute_amd import _cabi
    golden = np.load(GOLDEN)
    assert tuple(golden.files) == tuple(f"{e}_{f}" for e in ELEMS for f in FIELDS)
    got = plan_all(_cabi.lib(elem))
    assert got.shape[0] == golden[f"{elem}_rc"].shape[0] > 100000
    for i, f in enumerate(FIELDS):
        bad = np.nonzero(got[:, i] != golden[f"{elem}_{f}"].astype(np.int64))[0]
        assert bad.size == 0, (f"{f}: {bad.size} of {got.shape[0]} descriptors differ, first at row {bad[0]}: got {got[bad[0]].tolist()}, "
                               f"recorded {[int(golden[f'{elem}_{g}'][bad[0]]) for g in FIELDS]}")
    # the set is worth its name: every instance this build has, every split, both exchanges, both dealings, refusals
    ok = got[:, 0] == 0
    col = {f: got[:, i] for i, f in enumerate(FIELDS)}
    built = {(bn, waves) for _, bn, waves, builds in table_rows() if builds == "BOTH" or elem == "bf16"}
    assert set(zip(col["bn"][ok].tolist(), col["waves"][ok].tolist())) == built and len(built) == (8 if elem == "bf16" else 4)
    assert set(np.unique(col["splits"][ok])) == {1, 2, 4, 8}
    assert set(np.unique(col["peers_local"][ok])) == {0, 1} and set(np.unique(col["xcd_tile_major"][ok])) == {0, 1}
    assert (~ok).any() and set(np.unique(got[~ok, 0])) == {ERR_ARG} and not got[~ok, 1:].any()
    assert got[-1, 0] == ERR_ARG                       # the problem beyond the 32-bit block decode


def test_forced_instances_of_the_gpu_layout_test_are_rows_of_the_table():
    """tests/test_fwd_layout_gpu.py forces instances by a literal (force_bn, force_waves) list: every pair it names is a row of halo_tile.h, and
    between them they name every warp-specialised row - the instances the plan reaches by itself only where its waves rule takes them (the
    ping-pong rows are what (0, 0) and the forced splits of that test run)"""
    src = open(os.path.join(ROOT, "tests", "test_fwd_layout_gpu.py")).read()
    literal = ast.literal_eval(re.search(r"^HALO_INSTANCES = (\{.*?\})\s*(?:#.*)?$", src, re.M)[1])
    forced = {p for pairs in literal.values() for p in pairs if p != (0, 0)}
    rows = {(bn, waves) for _, bn, waves, _ in table_rows()}
    assert forced <= rows and forced >= {(bn, waves) for bn, waves in rows if waves != 8}
    assert all(bn == N for N, pairs in literal.items() for bn, _ in pairs if bn)
