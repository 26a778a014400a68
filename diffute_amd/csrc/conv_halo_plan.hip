// Plan of the halo 3x3 convolution (conv_halo.hip): which instance of halo_tile.h runs a problem, its pixel tile, column tile and K split,
// the block decode and dealing the kernel is given, the workspace and launch shape that takes.  Host arithmetic only - no HIP call: the
// device and the process enter as a HaloEnv (tests/test_halo_plan_host.py runs without a GPU).  One plan per launch: every caller plans
// once and hands the HaloPlan to dmx_conv_halo_launch.
#include "kernels.h"
#include "halo_tile.h"

namespace {

struct HaloInstance { int id, bn, waves, threads, lds_bytes; bool built; const char* what; };
#define DMX_HALO_ROW_(id, bn, waves, NF, WMW, WNW, WS, builds, what) \
  HaloInstance{id, HaloTile<NF, WMW, WNW, WS>::BN, waves, HaloTile<NF, WMW, WNW, WS>::NT, HaloTile<NF, WMW, WNW, WS>::TOTAL, (0 DMX_HALO_IN_BUILD_##builds(+1)) != 0, what},
constexpr HaloInstance kInst[] = {DMX_HALO_INSTANCES(DMX_HALO_ROW_)};
#undef DMX_HALO_ROW_
#define DMX_HALO_ROW_(i, bn_, waves, NF, WMW, WNW, WS, builds, what) \
  static_assert(kInst[i].id == i && kInst[i].bn == bn_ && (waves == 8) == !WS, "halo_tile.h: a row's id is its position, its bn its tile's, waves = 8 the ping-pong");
DMX_HALO_INSTANCES(DMX_HALO_ROW_)
#undef DMX_HALO_ROW_
static_assert(sizeof(kInst) / sizeof(kInst[0]) == DMX_HALO_NINST, "halo_tile.h: DMX_HALO_NINST");

// the instance of this build with this column tile and force_waves value, or null
const HaloInstance* find_inst(int bn, int waves) {
  for (const HaloInstance& I : kInst)
    if (I.built && I.bn == bn && I.waves == waves) return &I;
  return nullptr;
}

// x / d for x < 2^20, 2 <= d < 2^12 with magic = 2^32 / d + 1; d = 1: magic 0 (device: hb_div of conv_halo.hip)
unsigned halo_magic(int d) { return d <= 1 ? 0u : (unsigned)((1ull << 32) / (unsigned)d + 1); }

int g_halo_peers = 1;
int g_halo_ws = 1;                                     // dmx_set_halo_ws: 0 = the planner never takes the warp-specialised instances (A/B aid)

}  // namespace

// dmx_set_halo_peers: 0 = round-5 dealing and write-through slabs everywhere (A/B and the tests' second opinion); 1 = a tile's K-split peers on one XCD
extern "C" int dmx_set_halo_peers(int on) { const int old = g_halo_peers; g_halo_peers = on ? 1 : 0; dmx_plan_switch(DMX_SW_HALO_PEERS, g_halo_peers); return old; }
extern "C" int dmx_set_halo_ws(int on) { const int old = g_halo_ws; g_halo_ws = on; dmx_plan_switch(DMX_SW_HALO_WS, on); return old; }
HaloEnv dmx_halo_env() { return HaloEnv{n_cus(), dmx_exclusive_device(), g_halo_peers, g_halo_ws}; }

// the pixel tile of an H x W grid (8 x 32, else 16 x 16); false: none fits.  The ONE geometry rule: of the plan and of dmx_conv_halo_wants_stats
static bool halo_geometry(int H, int W, int* TH, int* TW) {
  if (W % 32 == 0 && H % 8 == 0) { *TW = 32; *TH = 8; return true; }
  if (W % 16 == 0 && H % 16 == 0) { *TW = 16; *TH = 16; return true; }
  return false;
}

// ONE place for "could a fused GroupNorm -> conv launch consume statistics records of an H x W tensor": the tile geometries of the plan and the
// level rule of the model executors.  They ask this before they spend a statistics pass / a statistics epilogue on a tensor
// (Exec::ensure_stats, Exec::chain_stats) and before they fuse (Exec::conv_gn); `everywhere` = dmx_set_halo_conv(2): wherever the kernel takes
// the problem.
// The level rule - the fused launch is at least as fast IN SITU as GroupNorm + the implicit-GEMM conv (+ its split-K reduce).
// Measured per shape inside the 50-step pass (B = 4; halo incl. GroupNorm vs conv + reduce + GroupNorm): 64x64 level 61 vs 69, 87 vs 105,
// 119 vs 129 us; 32x32 level 63 vs 66, 89 vs 98, 124 vs 125; 16x16 level 64 vs 61, 85 vs 77, 48 vs 44 - the blocks of the deep levels
// are 8-way K splits whose fp32 slab exchange costs what the fusion saves.
bool dmx_conv_halo_wants_stats(int H, int W, bool everywhere) {
  int th, tw;
  return halo_geometry(H, W, &th, &tw) && (everywhere || (long)H * W >= 1024);
}

// Plan: tile geometry, column width BN (160 / 128: 4 x 2 waves; 80 / 64: 8 x 1 waves) and K split.  A K split costs an exchange of fp32
// slabs through memory ((S - 1) / S x 256 x BN x 4 bytes per block, written and read back) and the co-residency of a tile's blocks, so the
// plan takes the narrow tiles where they make the split unnecessary or smaller; with tiles to spare the wide tile wins (twice the work per
// weight byte and per barrier).  Costs in us, fitted on scripts/attic/halo_probe.py.
HaloPlan dmx_conv_halo_plan(const HaloConvArgs& a, const HaloEnv& env) {
  const HaloPlan refused{};
  // ---- what the kernel takes at all
  if (a.Cin <= 0 || a.Cin % 64 || a.cx0 % 64 || a.cx0 > a.Cin || a.Csc % 64 || (a.Csc && a.cs0 % 64) || a.N % 8 || a.ldo % 8) return refused;
  if (a.ldx0 % 8 || (a.x1 && a.ldx1 % 8) || a.ldw % 8 || (a.res && a.ldres % 8)) return refused;
  if (a.gn && (a.groups != 32 || a.Cin % a.groups)) return refused;
  if (a.force_split && (a.force_split & (a.force_split - 1) || a.force_split > 8)) return refused;
  HaloPlan P{};
  if (!halo_geometry(a.H, a.W, &P.TH, &P.TW)) return refused;
  // ---- column tile and K split: the cheapest (ping-pong row, split) by the cost model
  const long tiles_m = (long)a.B * (a.H / P.TH) * (a.W / P.TW);
  const int T = 9 * (a.Cin / 64) + a.Csc / 64;
  double best = 1e300;
  for (const HaloInstance& I : kInst) {
    const int bn = I.bn;
    if (I.waves != 8 || a.N % bn) continue;
    if (a.force_bn && a.force_bn != bn) continue;
    const long tiles = tiles_m * (a.N / bn);
    for (int s = 1; s <= 8; s *= 2) {
      if (a.force_split && s != a.force_split) continue;
      if (s > 1 && (!env.exclusive || tiles * s > env.n_cu || T / s < 3)) continue;
      const double rounds = (double)((tiles * s + env.n_cu - 1) / env.n_cu);
      const double step = bn >= 128 ? 1.45 : 0.96;                         // us per tap and block (measured, B = 4 64x64x320: K = 2880 / 5760 / 8640)
      double cost = rounds * ((double)((T + s - 1) / s) * step + 13.0);    // + prologue / epilogue of a block
      if (s > 1) cost += 3.5 + 2.0 * (double)(s - 1) * bn / 160.0;         // publish + wait + the peers' slabs
      if (cost < best) { best = cost; P.bn = bn; P.splits = s; }
    }
  }
  if (!P.splits) return refused;
  // ---- the instance of that column tile.  waves: 8 = two-group ping-pong, 4 = warp-specialised (4 compute + 4 loader waves; the wide tiles
  // of the bf16 build only), 12 = forced only.
  // Measured (B = 4, stand-alone incl. GroupNorm, us; ping-pong / 4 + 4 / 8 + 4): 64x64x320 K = 2880 / 5760 / 8640 (two-way splits): 62.2 /
  // 85.3 / 113.1 - 61.0 / 81.7 / 107.0 - 62.6 / 84.2 / 111.1; 32x32x640 K = 5760 (four-way): 59.5 - 64.3 - 66.9; 16x16x1280 K = 11520
  // (eight-way): 58.8 - 70.0 - 77.6: the warp-specialised K loop is ~10 % faster per tap (1.02 vs 1.13 us), its epilogue with four / eight
  // slabs per row in flight has fewer registers to hide them in -> 4 + 4 up to two-way splits, the ping-pong beyond
  P.waves = 8;
  if (find_inst(P.bn, 4) && P.splits <= 2 && env.ws) P.waves = 4;
  if (a.force_waves && find_inst(P.bn, a.force_waves)) P.waves = a.force_waves;
  if (a.force_waves && a.force_waves != P.waves) return refused;
  const HaloInstance& I = *find_inst(P.bn, P.waves);
  P.inst = I.id; P.threads = I.threads; P.lds_bytes = I.lds_bytes;
  // ---- the block decode.  It divides by multiplication (hb_div: magic = 2^32 / d + 1), exact only while x * d < 2^32 for every dividend x
  // (block index, channel, patch row) and divisor d of the decode (larger problems: GroupNorm + the implicit GEMM, whose decode is 64-bit)
  const long tiles_x = a.W / P.TW, tiles_img = tiles_x * (a.H / P.TH), ncombo = (long)(a.N / P.bn) * P.splits, cpg = a.gn ? a.Cin / a.groups : 1;
  const long blocks = tiles_m * (a.N / P.bn) * P.splits;
  long dmax = tiles_m; for (long d : {ncombo, tiles_img, tiles_x, (long)P.TW + 2, cpg}) if (d > dmax) dmax = d;
  long xmax = blocks; for (long x : {(long)a.Cin, (long)(P.TH + 2) * (P.TW + 2) * 8}) if (x > xmax) xmax = x;
  if (!(xmax < (1l << 31) && dmax < (1l << 31) && (unsigned long long)xmax * (unsigned long long)dmax < (1ull << 32))) return refused;
  P.blocks = (int)blocks;
  P.tiles_x = (int)tiles_x; P.tiles_img = (int)tiles_img; P.tiles_m = (int)tiles_m; P.ncombo = (int)ncombo; P.cpg = (int)cpg;
  P.mg_tiles_x = halo_magic(P.tiles_x); P.mg_tiles_img = halo_magic(P.tiles_img); P.mg_tiles_m = halo_magic(P.tiles_m);
  P.mg_ncombo = halo_magic(P.ncombo); P.mg_pw = halo_magic(P.TW + 2); P.mg_cpg = halo_magic(P.cpg);
  // ---- block -> XCD dealing: weights-major when the weight slab is the larger stream of an XCD, pixel-tile-major otherwise
  {
    const double wbytes = 2.0 * a.N * (9.0 * a.Cin + a.Csc), abytes = 2.0 * a.B * a.H * a.W * (double)(a.Cin + a.Csc) * 1.33;
    // weights-major: every XCD reads its combos' weights once, the activations combos / 8 .. combos times; tile-major: the reverse
    P.xcd_tile_major = (abytes * (P.ncombo >= 8 ? P.ncombo / 8.0 : 1.0) + wbytes > abytes + wbytes * 8.0) ? 1 : 0;
  }
  // the S blocks of a tile on one XCD: r is the fastest index of the decode and an XCD's share of the grid (blocks / 8 consecutive Lb) holds whole tiles
  P.peers_local = (env.peers && P.splits > 1 && P.blocks % 8 == 0 && (P.blocks / 8) % P.splits == 0) ? 1 : 0;
  // ---- workspace of a K split: one completion flag + one XCC-id word per block (peers_local), then one fp32 slab of 256 x bn per block
  if (P.splits > 1) {
    P.flag_count = 2 * P.blocks;
    P.flag_bytes = align_up((size_t)P.flag_count * sizeof(int), 256);
    P.workspace_bytes = P.flag_bytes + (size_t)P.blocks * 256 * P.bn * sizeof(float);
  }
  P.ok = true;
  return P;
}

int dmx_conv_halo_check(const HaloConvArgs& a, const HaloPlan& P) {
  DMX_REQUIRE(a.x0 && a.w && a.out, "conv_halo: null argument");
  DMX_REQUIRE(P.ok, "conv_halo: unsupported problem (H=%d W=%d Cin=%d cx0=%d Csc=%d N=%d split=%d bn=%d)", a.H, a.W, a.Cin, a.cx0, a.Csc, a.N, a.force_split, a.force_bn);
  if (a.gn) DMX_REQUIRE(a.st0 && a.gamma && a.beta && (a.cx0 == a.Cin || a.st1), "conv_halo: the fused GroupNorm needs statistics records, gamma and beta");
  if (a.Csc) DMX_REQUIRE(a.s0 && (a.cs0 == a.Csc || a.s1), "conv_halo: the shortcut segment needs its source tensor(s)");
  DMX_REQUIRE(a.ldw >= 9 * a.Cin + a.Csc, "conv_halo: weight rows shorter than K");
  return DMX_OK;
}

int dmx_conv_halo_check_and_plan(const HaloConvArgs& a, const HaloEnv& env, HaloPlan* plan) {
  *plan = dmx_conv_halo_plan(a, env);
  return dmx_conv_halo_check(a, *plan);
}
