// Tile / split-K plan of the implicit-GEMM kernel (gemm.hip): which instance of gemm_tile.h runs a problem, how K is split, the workspace and
// launch shape that takes.  Host arithmetic only - no HIP call, the device enters as its CU count (tests/test_gemm_plan_host.py runs without a
// GPU).  The UNet's GEMMs are small next to 256 CUs (M = 256..16384 rows), so the plan trades tile efficiency against filling the CUs, with
// split-K (fp32 partials + a reduce pass) when tiles alone leave CUs idle.
#include "kernels.h"
#include "gemm_tile.h"

struct GemmInstance {
  int bm, bn, bk, threads;                             // derived from the GemmTile arguments; bm = 0: no such instance (`what` says why)
  bool persistent, col160, cs_twin, announced;
  int (*lds_bytes)(bool ln, bool pf); int (*pf_dump_off)(bool ln);
  int slots; double per_ktile, fixed; bool geglu160, search;
  const char* what;
};
template <class L> static constexpr GemmInstance live(int slots, double per_ktile, double fixed, bool geglu160, bool search, const char* what) {
  return {L::BM, L::BN, L::BK, L::NT, L::PERSISTENT, L::COL160, L::CS_TWIN, false, &L::lds_bytes, &L::pf_dump_off, slots, per_ktile, fixed, geglu160, search, what};
}
#define DMX_LIVE_(id, name, slots, pk, fx, geglu160, search, what, ...) live<GemmTile<__VA_ARGS__>>(slots, pk, fx, geglu160, search, what),
#define DMX_GONE_(id, name, announced, why) GemmInstance{0, 0, 0, 0, false, false, false, announced, nullptr, nullptr, 0, 0.0, 0.0, false, false, why},
static const GemmInstance kInst[DMX_GEMM_NCFG] = {DMX_GEMM_INSTANCES(DMX_LIVE_, DMX_GONE_)};

// force_tn <-> plan id: 1 <-> 128x64, 2 <-> 128x128, n >= 3 <-> n - 1
int dmx_gemm_cfg_of_force(int force_tn) { return force_tn == 1 ? CFG_128x64 : force_tn == 2 ? CFG_128x128 : force_tn - 1; }
int dmx_gemm_force_of_cfg(int c) { return c == CFG_128x64 ? 1 : c == CFG_128x128 ? 2 : c + 1; }
static long n_tiles(const GemmArgs& a, const GemmInstance& T) { return (long)(a.ups2 ? 4 * cdiv(a.M4, T.bm) : cdiv(a.M, T.bm)) * cdiv(a.N, T.bn); }

// number of blocks of a persistent launch: one per CU, fewer when the iteration space is small (>= 4 K-tiles per block),
// a multiple of 8 so the XCD-contiguous remap applies
static int persist_grid(const GemmArgs& a, const GemmInstance& T, int n_cu) {
  const long total = n_tiles(a, T) * (a.K / T.bk);
  long g = total / 4; if (g > n_cu) g = n_cu; if (g < 1) g = 1;
  if (g >= 8) g &= ~7L;
  return (int)g;
}
// what an instance can run: K-tile alignment of every K segment, and what its epilogue covers
static bool cfg_applicable(const GemmArgs& a, int c) {
  if (c < 0 || c >= DMX_GEMM_NCFG || !kInst[c].bm) return false;
  const GemmInstance& T = kInst[c];
  if (a.K % T.bk != 0 || a.Cin % T.bk != 0 || a.cx0 % T.bk != 0 || a.Ktaps % T.bk != 0 || (a.Ktaps < a.K && a.cs0 % T.bk != 0)) return false;
  // the 160 / 320-column epilogue: bias | folded LayerNorm, row bias, residual (+ GEGLU where the instance says so)
  if (T.col160 && (a.rowstats_out || a.act || a.out_f32 || (a.N & 7) || (!T.geglu160 && a.geglu))) return false;
  if (T.persistent && ((a.N & 7) || a.out_f32)) return false;   // stream-K owners finish through the coalesced bf16 epilogue
  return true;
}

// costs in units of one 128x128x32 K-tile step of one block
static double plan_cost(const GemmArgs& a, const GemmInstance& T, int sk, int n_cu) {
  const int nkt = a.K / T.bk;
  const long tiles = (long)cdiv(a.M, T.bm) * cdiv(a.N, T.bn);
  if (T.persistent) {                                          // every block gets total / grid K-tiles; ~2 tile boundaries per block
    const int g = persist_grid(a, T, n_cu);
    return (double)cdiv((int)(tiles * nkt), g) * T.per_ktile + T.fixed * (1.0 + (double)tiles / g);
  }
  const long nb = tiles * sk;
  const double t_block = cdiv(nkt, sk) * T.per_ktile + T.fixed;
  const int per_round = 256;                                   // CUs
  double rounds = (double)((nb + per_round - 1) / per_round);
  if (T.slots == 512 && nb <= 256) rounds = 1.2;               // two co-resident blocks overlap each other's stalls
  double t = rounds * t_block;
  if (sk > 1) t += 12.0 + ((double)a.M * a.N * 4.0 * (sk + 1) / 5.0e12) / 0.45e-6;   // reduce pass: ~5 us + traffic
  return t;
}

#include "gemm_tuned.h"

// Tuning aid (scripts/tune_in_situ.py): plan overrides set at run time take precedence over the compiled table, so a
// candidate plan can be timed inside the real UNet pass - with the shape's real epilogue, neighbours and cache state.
static std::vector<TunedPlan> g_plan_overrides;
void dmx_gemm_plan_override_set(int M, int N, int K, int st, int ups, int cfg, int sk) {
  dmx_plan_epoch_bump();
  if (cfg < 0) { g_plan_overrides.clear(); return; }
  for (TunedPlan& tp : g_plan_overrides)
    if (tp.M == M && tp.N == N && tp.K == K && tp.st == st && tp.ups == ups) { tp.cfg = cfg; tp.sk = sk; return; }
  g_plan_overrides.push_back(TunedPlan{M, N, K, 0, st, ups, cfg, sk});
}

// (instance, split) of a problem: override, tuned table, else the cheapest searchable instance by plan_cost
static void choose(const GemmArgs& a, int n_cu, GemmPlan& P) {
  const bool no_split = a.rowstats_out || a.ln_stats || a.geglu || a.act || (a.N % 4) != 0;   // those epilogues live in the GEMM kernel
  auto take = [&](int c, int sk) -> bool {
    if (!cfg_applicable(a, c)) return false;
    const int nkt = a.K / kInst[c].bk;
    if (kInst[c].persistent) { P.cfg = c; P.splitk = 1; P.kt_per_split = nkt; return true; }
    if (sk < 1 || (sk > 1 && (no_split || nkt / sk < 4))) return false;
    P.cfg = c; P.kt_per_split = cdiv(nkt, sk); P.splitk = cdiv(nkt, P.kt_per_split);
    return true;
  };
  if (!a.force_tn && !a.force_splitk && (a.N % 4) == 0) {
    // keyed on the GEMM view (M, N, K) + gather flavour; tap structure does not matter
    auto match = [&](const TunedPlan& tp) { return tp.M == a.M && tp.N == a.N && tp.K == a.K && tp.st == a.stride && tp.ups == (a.ups2 ? 2 : a.ups); };
    for (const TunedPlan& tp : g_plan_overrides)
      if (match(tp)) {
        if (take(tp.cfg, tp.sk)) return;
        break;                                                 // not applicable: normal plan
      }
    for (const TunedPlan& tp : kTuned)
      if (match(tp) && take(tp.cfg, tp.sk)) return;
  }
  int best_c = CFG_128x128, best_sk = 1; double best = 1e300;
  for (int c = 0; c < DMX_GEMM_NCFG; ++c) {
    const GemmInstance& T = kInst[c];
    if (!cfg_applicable(a, c)) continue;
    if (a.force_tn) { if (c != dmx_gemm_cfg_of_force(a.force_tn)) continue; }
    else {
      if (!T.search) continue;                            // eight-wave / 160-column / persistent instances: tuned table or force_tn only
      if (c != CFG_128x64 && a.N <= 64) continue;
      if ((c == CFG_256x128 || c == CFG_256x128_WS) && ((long)a.M * a.N < 256L * 128 * 96)) continue;     // big tiles only for big outputs
      // 3x3 convolutions over <= 128 input channels (the 512^2 / 256^2 levels of the autoencoder, K = 1152): the weight operand is
      // as large as the activation operand per tile, so the 256-row tile's reuse buys nothing and its longer prologue / epilogue
      // shows - measured at batch 32 (scripts/attic/vae_conv_probe.py): 128->128 3.54 vs 3.79 ms, 128->256 1.61 vs 1.76 ms
      if (c == CFG_256x128 && a.ksize == 3 && !a.direct && a.Cin <= 128 && a.Ktaps == a.K) continue;
    }
    const int nkt = a.K / T.bk;
    const int max_sk = (no_split || T.persistent) ? 1 : 16;
    for (int sk = 1; sk <= max_sk; ++sk) {
      if (a.force_splitk && sk != a.force_splitk && !T.persistent) continue;
      if (sk > 1 && nkt / sk < (T.bk == 64 ? 4 : 8)) break;
      if (c == CFG_256x128_WS && !a.force_tn && nkt / sk < 40) break;      // the warp-specialised loop pays off from ~2.5k of K per block
      const double cst = plan_cost(a, T, sk, n_cu);
      if (cst < best) { best = cst; best_c = c; best_sk = sk; }
    }
  }
  const int nkt = a.K / kInst[best_c].bk;
  P.cfg = best_c; P.kt_per_split = cdiv(nkt, best_sk); P.splitk = cdiv(nkt, P.kt_per_split);
}

GemmPlan dmx_gemm_plan(const GemmArgs& a, int n_cu) {
  GemmPlan P{};
  choose(a, n_cu, P);
  const GemmInstance& T = kInst[P.cfg];
  P.tiles_n = cdiv(a.N, T.bn);
  // workspace.  split-K: sk fp32 planes of the output.  Persistent stream-K: 256 bytes of flags per 64 blocks, then one accumulator slab per block
  if (T.persistent) {
    P.persist_blocks = persist_grid(a, T, n_cu);
    P.flag_bytes = align_up((size_t)P.persist_blocks * sizeof(int), 256);
    P.workspace_bytes = P.flag_bytes + (size_t)P.persist_blocks * T.bm * T.bn * sizeof(float);
  } else if (P.splitk > 1) {
    P.workspace_bytes = (size_t)P.splitk * a.M * a.N * sizeof(float);
  }
  // column statistics: bf16 coalesced epilogue, no reduce pass behind the kernel, an instance with a statistics twin, tiles inside one sample
  const int rows = a.ups2 ? a.M4 : a.M;
  P.colstats_ok = !(a.out_f32 || a.geglu || (a.N & 7) || (a.ldo & 7) || (a.res && (a.ldres & 7)) || a.cs_rows <= 0) && P.splitk == 1 && T.cs_twin &&
                  a.cs_rows % T.bm == 0 && rows % a.cs_rows == 0;
  return P;
}

GemmLaunchShape dmx_gemm_launch_shape(const GemmArgs& a, const GemmPlan& P) {
  const GemmInstance& T = kInst[P.cfg];
  const bool ln = a.ln_stats != nullptr, pf = a.pf_bytes[0] > 0;
  return {P.persist_blocks ? P.persist_blocks : (int)n_tiles(a, T), P.splitk, T.threads, T.lds_bytes(ln, pf), pf ? T.pf_dump_off(ln) : 0};
}

int dmx_gemm_check_and_plan(const GemmArgs& a, int n_cu, GemmPlan* plan) {
  DMX_REQUIRE(a.M > 0 && a.N > 0 && a.K > 0, "gemm: empty problem M=%d N=%d K=%d", a.M, a.N, a.K);
  DMX_REQUIRE(a.K % 32 == 0, "gemm: K=%d must be a multiple of 32", a.K);
  DMX_REQUIRE(a.ldw % 8 == 0 && a.ldx0 % 8 == 0, "gemm: leading dimensions must be multiples of 8 (ldw=%d ldx0=%d)", a.ldw, a.ldx0);
  DMX_REQUIRE(a.cx0 % 32 == 0 && a.Cin % 32 == 0, "gemm: channel splits must be multiples of 32 (Cin=%d cx0=%d)", a.Cin, a.cx0);
  DMX_REQUIRE(a.Ktaps % 32 == 0 && a.Ktaps <= a.K, "gemm: bad Ktaps=%d K=%d", a.Ktaps, a.K);
  if (a.Ktaps < a.K) DMX_REQUIRE(a.s0 != nullptr && a.cs0 % 32 == 0, "gemm: shortcut segment needs s0 and aligned cs0");
  if (a.ln_stats) DMX_REQUIRE(a.ln_c1 && a.ln_c2 && a.ln_tiles > 0 && a.ln_C > 0 && !a.out_f32 && a.N % 8 == 0 && a.ldo % 8 == 0, "gemm: folded LayerNorm needs c1/c2, bf16 output and N %% 8 == 0");
  if (a.rowstats_out) DMX_REQUIRE(!a.out_f32 && a.N % 8 == 0 && a.ldo % 8 == 0 && !a.geglu, "gemm: row statistics need the bf16 coalesced epilogue");
  if (a.act) DMX_REQUIRE(a.act == 1 && !a.out_f32 && !a.geglu && a.N % 8 == 0 && a.ldo % 8 == 0 && (a.res == nullptr || a.ldres % 8 == 0), "gemm: the GELU epilogue needs the bf16 coalesced path (N %% 8 == 0)");
  if (a.geglu) DMX_REQUIRE((a.bias || a.ln_stats) && a.N % 128 == 0 && !a.out_f32 && !a.res && !a.rowbias && a.ldo % 8 == 0, "gemm: GEGLU needs bias, N%%128==0, bf16 out");
  if (a.ups2) {
    DMX_REQUIRE(a.ksize == 2 && !a.direct && !a.ups && a.stride == 1 && a.OH == a.IH && a.OW == a.IW && a.M4 > 0 && a.M == 4 * a.M4 &&
                a.Ktaps == a.K && a.K == 4 * a.Cin && a.w_phase_stride > 0, "gemm: inconsistent phase-decomposed upsample conv arguments");
    DMX_REQUIRE(!a.res && !a.rowbias && !a.geglu && !a.act && !a.ln_stats && !a.rowstats_out, "gemm: the phase-decomposed upsample conv takes a bias only");
  }
  const int fc = dmx_gemm_cfg_of_force(a.force_tn);
  DMX_REQUIRE(!a.force_tn || fc < 0 || fc >= DMX_GEMM_NCFG || !kInst[fc].announced, "gemm: tile instance %d was retired", a.force_tn);
  *plan = dmx_gemm_plan(a, n_cu);
  if (a.colstats) DMX_REQUIRE(plan->colstats_ok, "gemm: this plan cannot emit column statistics (split-K, fp32 / GEGLU output or tiles straddling samples)");
  if (a.force_tn) DMX_REQUIRE(cfg_applicable(a, fc), "gemm: tile instance %d cannot run this problem (K-tile alignment / epilogue)", a.force_tn);
  return DMX_OK;
}
