// The tile instances of the implicit-GEMM kernel (gemm.hip), described once.  GemmTile<...> derives from the kernel's template arguments
// what the kernel, its launcher and the planner (gemm_plan.hip) all need - tile shape, block size, the dynamic-LDS layout, capabilities -
// and DMX_GEMM_INSTANCES lists the instances, one row per plan id.  Host-only arithmetic: nothing here touches the device.
#pragma once
constexpr int DMX_GEMM_LDS_MAX = 163840;   // LDS of a CU: what one block may ask for

// WM x NWN MFMA waves (along m x along n), each a (MF TM) x (MF TN) wave tile of MF x MF fragments; NP extra waves that only issue LDS-DMA
// (warp specialisation); BKT deep K-tiles in an NSTAGE ring; PS = persistent stream-K work loop
template <int WM, int TN, int BKT, int NSTAGE, int TM = 2, int NP = 0, int NWN = 2, bool PS = false, int MF = 32> struct GemmTile {
  static constexpr int BM = MF * TM * WM, BN = MF * TN * NWN, BK = BKT;
  static constexpr int NC = NWN * WM;                  // consumer (MFMA) waves
  static constexpr int NT = 64 * (NC + NP);            // block threads
  static constexpr bool COL160 = TN == 5;              // 160 / 320-column tiles: their own coalesced epilogue (bias | folded LayerNorm, row bias, residual)
  static constexpr bool WARP_SPEC = NP > 0;            // separate loader and MFMA wave loops
  static constexpr bool PERSISTENT = PS;               // one block per CU walks (tile, K-range) items, fix-up in the kernel, no reduce pass
  static constexpr bool PINGPONG = PS && BM >= 256;    // two-group ping-pong K loop (persistent big tiles)
  // a second instantiation that also emits GroupNorm column statistics (GemmArgs.colstats).  The warp-specialised instance has none; on the
  // persistent 160-column instances the statistics cost the producer as much as the consumer saves (in situ: 53.8 -> 59.1 us)
  static constexpr bool CS_TWIN = !WARP_SPEC && !(PS && COL160);
  // second argument of __launch_bounds__, which HIP reads as waves per SIMD, i.e. the register budget per lane: 4 (128 registers) for the
  // eight-wave tiles of 32x32 / 32x64 wave tiles, so that two blocks (16 waves) share a CU; 1 (no bound beyond the block size) for the
  // eight-wave 160-column tiles of two wave columns, one block per CU; 2 (256 registers) for everything else
  static constexpr int MIN_WAVES = (COL160 && NWN == 2) ? 1 : ((WM == 4 && TM == 1 && TN <= 2 && NP == 0 && NWN == 2) ? 4 : 2);
  // ---- dynamic LDS: [ring | epilogue staging (the ring is free by then)] [LayerNorm (mean, rstd) per row] [column vectors] [prefetch dump]
  static constexpr int STAGE = (BM + BN) * BKT * 2;    // one ring stage: activation tile + weight tile, [rows][BKT] 16-bit
  static constexpr int RING = NSTAGE * STAGE;
  static constexpr int EPI_BYTES = BM * (BN + 4) * 4;  // whole-tile fp32 staging of the coalesced epilogue
  // passes: the 160 / 320-column tiles stage half their rows at a time; a tile that does not fit beside 8 KB for the areas behind it (256x256) one wave row
  static constexpr int EPI_PASSES = COL160 ? 2 : (EPI_BYTES <= DMX_GEMM_LDS_MAX - 8192 ? 1 : WM);
  static constexpr int EPI_PASS = EPI_BYTES / EPI_PASSES;
  static constexpr int LN_OFF = RING > EPI_PASS ? RING : EPI_PASS;      // [BM][2] floats; allocated with GemmArgs.ln_stats or COL160
  static constexpr int COLV_OFF = LN_OFF + BM * 2 * 4;                  // COL160: [3][BN] floats (bias | c2, c1, row bias)
  static constexpr int lds_base(bool ln) { return (ln || COL160) ? COLV_OFF + (COL160 ? 3 * BN * 4 : 0) : LN_OFF; }
  // the 1 KB the weight prefetch (GemmArgs.pf) lands in sits behind everything else where it fits (0: no slot, no prefetch); persistent instances: none
  static constexpr int pf_dump_off(bool ln) { return (!PS && lds_base(ln) + 1024 <= DMX_GEMM_LDS_MAX) ? lds_base(ln) : 0; }
  static constexpr int lds_bytes(bool ln, bool pf) { return (pf && pf_dump_off(ln)) ? pf_dump_off(ln) + 1024 : lds_base(ln); }
  static constexpr int LDS_OPT_IN = lds_bytes(true, true);              // hipFuncAttributeMaxDynamicSharedMemorySize: the largest layout
  static_assert(lds_base(true) % 16 == 0 && LDS_OPT_IN <= DMX_GEMM_LDS_MAX, "LDS budget");
};

// One row per plan id (ProfClass 10 + id, `cfg` of gemm_tuned.h and dmx_gemm_plan_override; force_tn: dmx_gemm_force_of_cfg).
//   LIVE(id, name, slots, per_ktile, fixed, geglu160, search, what it is for, GemmTile arguments...)
//     slots = blocks the chip holds (512: two per CU); per_ktile / fixed = cost of a K-tile step / of prologue + epilogue per block, in
//     units of one 128x128x32 K-tile step (~0.45 us; fitted on scripts/tune_gemm.py measurements); geglu160 = the 160-column epilogue
//     of this instance does GEGLU; search = the cost model may pick it (the others: tuned table, override or force_tn only)
//   GONE(id, name, announced, why) - measured, not adopted (EXPERIMENTS.md), never instantiated; the id stays so the numbering is stable.
//     announced = its force_tn value was public once and is refused by name
#define DMX_GEMM_INSTANCES(LIVE, GONE)                                                                                                      \
  LIVE(0, CFG_128x128, 512, 1.00, 9.0, false, true, "128x128x32, 4 waves, 64 KB ring, 2 blocks/CU: mid-size GEMMs, split-K convolutions", 2, 2, 32, 4) \
  LIVE(1, CFG_128x64, 512, 0.78, 6.0, false, true, "128x64x32, 4 waves, 48 KB: N <= 64", 2, 1, 32, 4)                                      \
  LIVE(2, CFG_256x128, 256, 2.35, 10.0, false, true, "256x128x64, 8 waves, 144 KB, 1 block/CU: large GEMMs (128-byte DMA rows, 85 FLOP/B)", 4, 2, 64, 3) \
  GONE(3, CFG_128x64_2STAGE, true, "two-stage 128x64x64")                                                                                   \
  GONE(4, CFG_128x128_DEEP, true, "deep-ring 128x128x64")                                                                                   \
  GONE(5, CFG_256x256, true, "256x256x32, 128 FLOP/B")                                                                                      \
  LIVE(6, CFG_256x128_WS, 256, 1.90, 11.0, false, true, "warp-specialised 256x128x64, 4 MFMA waves (128x64) + 4 DMA waves: large K", 2, 2, 64, 3, 4, 4) \
  LIVE(7, CFG_128x64_8W, 512, 0.55, 5.0, false, false, "128x64x64, EIGHT waves (32x32): small grids are bound by the per-CU LDS-DMA fill rate, which doubles with 8 issuing waves", 4, 1, 64, 3, 1) \
  LIVE(8, CFG_128x128_8W, 512, 1.00, 8.0, false, false, "128x128x32, eight waves (32x64), 4-stage ring", 4, 2, 32, 4, 1)                   \
  LIVE(9, CFG_128x128x64_8W, 256, 1.00, 8.0, false, false, "128x128x64, eight waves, 3-stage ring (96 KB)", 4, 2, 64, 3, 1)                \
  LIVE(10, CFG_128x160, 512, 1.10, 8.0, false, false, "128x160x64, four waves in one column (32x160), 2-buffer ring (72 KB, 2 blocks/CU): 160 divides every channel count of the UNet (320 k)", 4, 5, 64, 2, 1, 0, 1) \
  LIVE(11, CFG_128x320, 256, 2.00, 10.0, true, false, "128x320x64, eight waves (4 x 2) of 32x160, 2-buffer ring (112 KB, 1 block/CU): five whole GEGLU groups per tile, the FF1 GEMMs (N = 8C) in one full round", 4, 5, 64, 2, 1, 0, 2) \
  LIVE(12, CFG_P256x160, 256, 1.6, 8.0, false, false, "persistent 256x160x64, eight waves in one column (32x160), 3-stage ring (156 KB)", 8, 5, 64, 3, 1, 0, 1, true) \
  GONE(13, CFG_P256x256, false, "persistent 256x256x32: 128 accumulators + the ping-pong loop spill")                                       \
  LIVE(14, CFG_P256x128, 256, 1.3, 7.0, false, false, "persistent 256x128x64, eight waves in one column (32x128), 3-stage ring (144 KB)", 8, 4, 64, 3, 1, 0, 1, true) \
  LIVE(15, CFG_P256x160_MF16, 256, 1.4, 8.0, false, false, "persistent 256x160x64 with 16x16x32 MFMAs, eight waves (4 x 2) of 64x80: 25 % fewer LDS fragment bytes per FLOP", 4, 5, 64, 3, 4, 0, 2, true, 16)

#define DMX_GEMM_ID_(id, name, ...) name = id,
enum GemmCfgId { DMX_GEMM_INSTANCES(DMX_GEMM_ID_, DMX_GEMM_ID_) DMX_GEMM_NCFG };
#undef DMX_GEMM_ID_
