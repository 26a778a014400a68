// The tile instances of the halo 3x3 convolution (conv_halo.hip), described once.  HaloTile<...> derives from the kernel's template arguments
// what the kernel, its launcher and the planner (conv_halo_plan.hip) all need - block size, wave roles, column width, the dynamic-LDS
// layout - and DMX_HALO_INSTANCES lists the instances, one row per instance id.  Host-only arithmetic: nothing here touches the device.
#pragma once

constexpr int HB_PATCH = 44032;            // patch buffer: 2752 pieces of 16 B (340 rows of 128 B, rounded up to whole 1-KB DMA instructions)

// A block is 256 output pixels x BN output channels.  WMW x WNW compute waves (along the pixels x along the channels), each a
// (256 / WMW)-pixel x 16 NF-channel wave tile of 16x16x32 MFMAs; WS = warp-specialised: four more waves that only load.  The instances:
//   * 8-wave ping-pong, WIDE tiles (WMW x WNW = 4 x 2, 64-pixel x 16 NF-channel wave tiles, BN = 160 / 128): two groups of four waves run
//     the same stream one barrier apart, so on every SIMD one wave issues MFMAs while its partner issues LDS-DMA and normalises
//   * 8-wave ping-pong, NARROW tiles (8 x 1, 32-pixel wave tiles, BN = 80 / 64) with TWO taps per pipeline step: twice the tiles - the
//     levels where the wide tile would need a K split, i.e. an exchange of fp32 slabs through memory
//   * 4 + 4 warp-specialised (4 x 1 compute waves of 64-pixel x 160 / 128-column tiles + four LOADER waves): the compute waves only read
//     fragments and issue MFMAs, the loaders issue every LDS-DMA instruction and normalise the patches - one barrier per tap.  What bounds a
//     ping-pong step is the DMA phase of a group (each LDS-DMA instruction holds its wave ~100 cycles; 6-7 per wave and tap plus the
//     normalisation is longer than the partner's 640 cycles of MFMAs), and the 64 x 80 wave tiles read 144 KB of fragments per tap (88 % of
//     the LDS bandwidth under the MFMAs); here the loaders have the whole tap for the same DMA work and the fragment reads are 112 KB
//   * 4 x 2 + 4 warp-specialised: the wide tile's eight compute waves + four loader waves (force_waves = 12 only)
// (16-wave lock-step instances of the wide tiles were built, measured slower than the ping-pong and removed: EXPERIMENTS.md round 4.)
template <int NF, int WMW, int WNW, bool WS_ = false> struct HaloTile {
  static constexpr bool WS = WS_;
  static constexpr int NCW = WMW * WNW;               // compute waves
  static constexpr int NT = 64 * NCW + (WS ? 256 : 0);   // threads (WS: + four loader waves)
  static constexpr int DNT = WS ? 256 : NT;           // threads that issue DMA / normalise (WS: the last 256 threads of the block)
  static constexpr bool PP = !WS && (NCW == 8);       // two-group ping-pong (8 waves)
  static constexpr int BN = WNW * 16 * NF;
  static constexpr int MFR = 16 / WMW;                // 16-pixel fragments per wave
  // TPS = taps per pipeline step: the narrow tiles have the LDS for TWO weight tiles per ring stage (2 x 10 KB = one stage of the
  // 160-column tile): per step the same DMA / MFMA work as the wide tile with half the barriers, DMA-phase overheads and
  // normalisation slots per FLOP - and twice the tiles, i.e. no K split (no fp32 slab exchange) at the 64 x 64 level
  static constexpr int TPS = (WMW == 8 && WNW == 1) ? 2 : 1;
  static constexpr int WTILE = BN * 128;              // one tap's [BN][64] weight tile
  static constexpr int WSTAGE = TPS * WTILE;
  // weight ring: 3 stages = prefetch distance 1 under the two-group ping-pong (stage (s - 1) % 3 is the partner's, s % 3 this wave's next).
  // A 4-stage ring / distance 2 with a counted vmcnt was built for the tiles that have the LDS for it and measured SLOWER (64x64x320,
  // 80 columns: 72 vs 62 us): what bounds a step is each wave's serial non-MFMA work, not the landing time of the tile (EXPERIMENTS.md)
  static constexpr int NSTG = 3;
  static constexpr int PATCH0 = NSTG * WSTAGE, PATCH1 = PATCH0 + HB_PATCH;
  static constexpr int GB = PATCH1 + HB_PATCH;        // gamma | beta of a chunk, two 1-KB slots (lanes 32..63 of the DMA land in the second half)
  static constexpr int COEF = GB + 2048;              // (a, s) of the 64 channels of a chunk, 512 B
  static constexpr int GST = COEF + 512;              // (mean, rstd) of the 32 groups, 256 B (+ 256 spare)
  static constexpr int DUMP = GST + 512;              // 1 KB the weight prefetch for the NEXT launches lands in (HaloConvArgs.pf)
  static constexpr int TOTAL = DUMP + 1024;
  // epilogue: fp32 staging of 128 rows + the statistics fold
  static constexpr int LDT = BN + 4;
  static constexpr int EPI_FOLD = 128 * LDT * 4;
  static constexpr int OCP = BN / 8, RL = NT / OCP;
  static constexpr int EPI_TOTAL = EPI_FOLD + RL * BN * 8;
  static_assert(EPI_TOTAL <= TOTAL && TOTAL <= 163840, "LDS budget");
};

// One row per instance:  ROW(id, bn, waves, NF, WMW, WNW, WS, builds, what it is for)
//   bn = output columns per block (HaloConvArgs.force_bn), waves = the HaloConvArgs.force_waves value that selects the instance among
//   those of its bn.  The waves = 8 rows, in this order, are the candidates of the planner's cost search (every bn has one; a tie goes to
//   the earlier row); its waves rule then chooses among the instances of the bn it took.  The launcher instantiates the kernels in row
//   order, which is their order in the code object.
//   builds = BOTH | BF16_ONLY.  The warp-specialised instances are NOT instantiated under -DDMX_F16: in the fp16 build the compiler spills
//   an accumulator of the 160-column instance INSIDE the tap loop, which the asm MFMAs make a correctness bug - non-deterministic results
//   at 768 px, EXPERIMENTS.md round 4 item 1b; tests/test_build_cpu.py checks the ISA of both builds.
#define DMX_HALO_INSTANCES(ROW)                                                                                                             \
  ROW(0, 160, 4, 10, 4, 1, true, BF16_ONLY, "4 + 4 warp-specialised 256x160: ~10 % faster per tap, up to two-way splits")                  \
  ROW(1, 128, 4, 8, 4, 1, true, BF16_ONLY, "4 + 4 warp-specialised 256x128")                                                               \
  ROW(2, 160, 12, 5, 4, 2, true, BF16_ONLY, "4 x 2 + 4 warp-specialised 256x160: forced only (measured between the other two)")            \
  ROW(3, 128, 12, 4, 4, 2, true, BF16_ONLY, "4 x 2 + 4 warp-specialised 256x128: forced only")                                             \
  ROW(4, 160, 8, 5, 4, 2, false, BOTH, "ping-pong 256x160: tiles to spare (twice the work per weight byte and per barrier of the narrow tiles)") \
  ROW(5, 128, 8, 4, 4, 2, false, BOTH, "ping-pong 256x128: channel counts 160 does not divide")                                            \
  ROW(6, 80, 8, 5, 8, 1, false, BOTH, "ping-pong 256x80, two taps per step: where the wide tile would need a K split, or a deeper one")    \
  ROW(7, 64, 8, 4, 8, 1, false, BOTH, "ping-pong 256x64, two taps per step")
constexpr int DMX_HALO_NINST = 8;

// DMX_HALO_IN_BUILD_<builds>(code): `code` where this build has the instance, nothing where it has not
#define DMX_HALO_IN_BUILD_BOTH(...) __VA_ARGS__
#ifdef DMX_F16
#define DMX_HALO_IN_BUILD_BF16_ONLY(...)
#else
#define DMX_HALO_IN_BUILD_BF16_ONLY(...) __VA_ARGS__
#endif
