// Test support (include/diffute_hip.h "test support"): extern "C" entries that reach the small training kernels which have no
// operator-level entry of their own - train_small.hip's transposes, add, pointwise 1x1 and small-linear backward, norm.hip's row
// softmax and vae_train.hip's casts (tests/test_train_small_gpu.py) - and the two weight-preparation kernels that only the model
// executors launch: gemm.hip's folded-LayerNorm weights and elementwise.hip's padded context cast (tests/test_weight_pack_gpu.py); fold.hip's
// composition and the folded block tail on the executor (tests/test_ff_fold_gpu.py); gemm_plan.hip's and conv_halo_plan.hip's planners
// (tests/test_gemm_plan_host.py, tests/test_halo_plan_host.py).
// Each entry checks its arguments and forwards to the *_launch function / executor op the graphs call; none does arithmetic of its own.
#include "exec.h"

#define ST(s) ((hipStream_t)(s))

extern "C" int dmx_test_transpose_bf16(const void* in, int ldin, void* out, int ldout, int R, int C, dmx_stream_t stream) {
  DMX_REQUIRE(in && out && R > 0 && C > 0 && ldin >= C && ldout >= R, "test_transpose_bf16: bad argument");
  return dmx_transpose_bf16_launch((const bf16*)in, ldin, (bf16*)out, ldout, R, C, ST(stream));
}

// The jobs are recorded through a TrBatch exactly as *_train_prepare records them (kernels.h) and run as one launch.  `table` is the
// caller's device buffer for the job table; the host-side copy of what was uploaded last stays alive between calls, so a repeated
// batch takes the "table unchanged" path.  njobs = 0, or another table pointer, forgets that copy.
extern "C" int dmx_test_transpose_batch(const dmx_test_tr_job* h_jobs, int njobs, void* table, size_t table_bytes, dmx_stream_t stream) {
  static std::vector<TrJob> cache;
  static void* cache_table = nullptr;
  if (njobs == 0) { cache.clear(); cache_table = nullptr; return DMX_OK; }
  DMX_REQUIRE(h_jobs && njobs > 0 && table, "test_transpose_batch: null argument");
  DMX_REQUIRE((size_t)njobs * sizeof(TrJob) <= table_bytes && table_bytes <= DMX_TR_TABLE_BYTES, "test_transpose_batch: %d jobs, table of %zu bytes", njobs, table_bytes);
  for (int i = 0; i < njobs; ++i)
    DMX_REQUIRE(h_jobs[i].in && h_jobs[i].out && h_jobs[i].R > 0 && h_jobs[i].C > 0 && h_jobs[i].ldin >= h_jobs[i].C && h_jobs[i].ldout >= h_jobs[i].R,
                "test_transpose_batch: bad job %d", i);
  if (table != cache_table) { cache.clear(); cache_table = table; }
  TrBatch batch;
  for (int i = 0; i < njobs; ++i) {
    const int rc = dmx_transpose_bf16_launch((const bf16*)h_jobs[i].in, h_jobs[i].ldin, (bf16*)h_jobs[i].out, h_jobs[i].ldout, h_jobs[i].R, h_jobs[i].C, ST(stream));
    if (rc) return rc;
  }
  return batch.run(table, table_bytes, cache, ST(stream));
}

extern "C" int dmx_test_add_bf16(const void* a, int lda, const void* b, int ldb, void* out, int ldo, int rows, int C, dmx_stream_t stream) {
  DMX_REQUIRE(a && b && out && rows > 0 && C > 0 && lda >= C && ldb >= C && ldo >= C, "test_add_bf16: bad argument");
  return dmx_add_bf16_launch((const bf16*)a, lda, (const bf16*)b, ldb, (bf16*)out, ldo, rows, C, ST(stream));
}

extern "C" int dmx_test_softmax_rows(const float* s, int lds, void* p, int ldp, int rows, int n, float scale, dmx_stream_t stream) {
  DMX_REQUIRE(s && p && rows > 0 && n > 0 && lds >= n && ldp >= n, "test_softmax_rows: bad argument");
  return dmx_softmax_rows_launch(s, lds, (bf16*)p, ldp, rows, n, scale, ST(stream));
}
extern "C" int dmx_test_softmax_bwd_rows(const void* p, int ldp, const float* dp, int lddp, void* ds, int ldds, int rows, int n, float scale, dmx_stream_t stream) {
  DMX_REQUIRE(p && dp && ds && rows > 0 && n > 0 && ldp >= n && lddp >= n && ldds >= n, "test_softmax_bwd_rows: bad argument");
  return dmx_softmax_bwd_rows_launch((const bf16*)p, ldp, dp, lddp, (bf16*)ds, ldds, rows, n, scale, ST(stream));
}

extern "C" int dmx_test_pointwise_small_fwd(const void* x, int ldx, const void* w, int ldw, const float* bias, void* y, int ldy, int M, int Cin, int Cout,
                                            int out_f32, dmx_stream_t stream) {
  DMX_REQUIRE(x && w && y && M > 0 && ldx >= Cin && ldw >= Cin && ldy >= Cout, "test_pointwise_small_fwd: bad argument");
  return dmx_pointwise_small_fwd_launch((const bf16*)x, ldx, (const bf16*)w, ldw, bias, y, ldy, M, Cin, Cout, out_f32, ST(stream));
}
extern "C" size_t dmx_test_pointwise_small_bwd_workspace_bytes(int M, int Cin, int Cout) { return dmx_pointwise_small_bwd_ws_bytes(M, Cin, Cout); }
extern "C" int dmx_test_pointwise_small_bwd(const void* x, int ldx, const float* dy, int lddy, const void* w, int ldw, void* dx, int lddx,
                                            float* dw, int lddw, float* db, int M, int Cin, int Cout, void* workspace, size_t workspace_bytes, dmx_stream_t stream) {
  DMX_REQUIRE(x && dy && w && dw && db && M > 0 && ldx >= Cin && lddy >= Cout && ldw >= Cin && lddw >= Cin && (!dx || lddx >= Cin), "test_pointwise_small_bwd: bad argument");
  return dmx_pointwise_small_bwd_launch((const bf16*)x, ldx, dy, lddy, (const bf16*)w, ldw, (bf16*)dx, lddx, dw, lddw, db, M, Cin, Cout, workspace, workspace_bytes, ST(stream));
}

extern "C" int dmx_test_linear_small_bwd(const float* x, int ldx, const float* dy, int lddy, const void* w, int ldw, float* dw, int lddw, float* db, int db_stride,
                                         float* dx, int lddx, int B, int N, int K, int silu_in, int accumulate, dmx_stream_t stream) {
  DMX_REQUIRE(dy && B > 0 && N > 0 && K > 0 && lddy >= N && (dw || dx), "test_linear_small_bwd: bad argument");
  DMX_REQUIRE(!dw || (x && ldx >= K && lddw >= K && (!db || db_stride >= 1)), "test_linear_small_bwd: dw wants x, lddw >= K, db_stride >= 1");
  DMX_REQUIRE(!dx || (w && ldw >= K && lddx >= K && (!silu_in || (x && ldx >= K))), "test_linear_small_bwd: dx wants w, lddx >= K (and x with silu_in)");
  DMX_REQUIRE(dw || !db, "test_linear_small_bwd: db is written by the dw kernel");
  return dmx_linear_small_bwd_launch(x, ldx, dy, lddy, (const bf16*)w, ldw, dw, lddw, db, db_stride, dx, lddx, B, N, K, silu_in, accumulate, ST(stream));
}

extern "C" int dmx_test_slice_cast(const float* in, int ldin, void* out, int ldo, int M, int C, dmx_stream_t stream) {
  DMX_REQUIRE(in && out && M > 0 && C > 0 && ldin >= C && ldo >= C, "test_slice_cast: bad argument");
  return dmx_slice_cast_launch(in, ldin, (bf16*)out, ldo, M, C, ST(stream));
}
extern "C" int dmx_test_mode_bwd(const void* dz, int lddz, float* dmom, int M, int C, dmx_stream_t stream) {
  DMX_REQUIRE(dz && dmom && M > 0 && C > 0 && lddz >= C, "test_mode_bwd: bad argument");
  return dmx_mode_bwd_launch((const bf16*)dz, lddz, dmom, M, C, ST(stream));
}
extern "C" int dmx_test_bf16_to_f32_rows(const void* in, int ldin, float* out, int M, int C, dmx_stream_t stream) {
  DMX_REQUIRE(in && out && M > 0 && C > 0 && ldin >= C, "test_bf16_to_f32_rows: bad argument");
  return dmx_bf16_to_f32_rows_launch((const bf16*)in, ldin, out, M, C, ST(stream));
}

// The GEMM planner without a device (tests/test_gemm_plan_host.py): what dmx_conv_gemm(d) would check, plan and launch on n_cus compute units
extern "C" int dmx_test_gemm_plan(const dmx_gemm_desc* d, int n_cus, long long* out) {
  DMX_REQUIRE(d && out && n_cus > 0, "test_gemm_plan: bad argument");
  for (int i = 0; i < 12; ++i) out[i] = 0;
  GemmArgs a = dmx_gemm_args(d);
  if (d->ups == 2) { a.ups = 0; a.ups2 = 1; a.M4 = a.M / 4; a.w_phase_stride = (long long)a.N * a.K; }   // the phase-decomposed upsample conv of dmx_conv_ups2x
  GemmPlan P;
  if (const int rc = dmx_gemm_check_and_plan(a, n_cus, &P)) return rc;
  a.pf_bytes[0] = 0;    const GemmLaunchShape s = dmx_gemm_launch_shape(a, P);        // without / with weight-prefetch ranges (Exec::peek)
  a.pf_bytes[0] = 4096; const GemmLaunchShape spf = dmx_gemm_launch_shape(a, P);
  const long long v[12] = {P.cfg, P.splitk, P.kt_per_split, P.tiles_n, P.persist_blocks, (long long)P.workspace_bytes, s.grid_x, s.grid_y, s.threads, s.lds_bytes, spf.lds_bytes, P.colstats_ok ? 1 : 0};
  for (int i = 0; i < 12; ++i) out[i] = v[i];
  return DMX_OK;
}

// The halo-conv planner without a device (tests/test_halo_plan_host.py): what dmx_conv3x3_gn(d) would check and plan on n_cus compute units under
// the given settings of dmx_set_exclusive_device / dmx_set_halo_peers / dmx_set_halo_ws
extern "C" int dmx_test_halo_plan(const dmx_halo_conv_desc* d, int n_cus, int exclusive, int peers, int ws, long long* out) {
  DMX_REQUIRE(d && out && n_cus > 0, "test_halo_plan: bad argument");
  for (int i = 0; i < 23; ++i) out[i] = 0;
  HaloPlan P;
  if (const int rc = dmx_conv_halo_check_and_plan(dmx_halo_args(d), HaloEnv{n_cus, exclusive, peers, ws}, &P)) return rc;
  const long long v[23] = {P.TH, P.TW, P.bn, P.waves, P.splits, P.blocks, P.threads, P.lds_bytes, P.flag_count, (long long)P.workspace_bytes, P.xcd_tile_major, P.peers_local,
                           P.tiles_x, P.tiles_img, P.tiles_m, P.ncombo, P.cpg, P.mg_tiles_x, P.mg_tiles_img, P.mg_tiles_m, P.mg_ncombo, P.mg_pw, P.mg_cpg};
  for (int i = 0; i < 23; ++i) out[i] = v[i];
  return DMX_OK;
}

// W' (16) [N][K] = round16(w_raw * gamma), c1[n] = sum_k W'[n][k], c2[n] = sum_k beta[k] w_raw[n][k] (+ bias[n]); all dense, K a multiple of 8
extern "C" int dmx_test_ln_fold(const void* w_raw, void* w_out, const float* gamma, const float* beta, const float* bias, float* c1, float* c2,
                                int N, int K, dmx_stream_t stream) {
  DMX_REQUIRE(w_raw && w_out && gamma && beta && c1 && c2 && N > 0 && K > 0, "test_ln_fold: bad argument");
  return dmx_ln_fold_launch((const bf16*)w_raw, (bf16*)w_out, gamma, beta, bias, c1, c2, N, K, ST(stream));
}
// w_out (16) [C][K + C] = [ round16(wpo [C][C] . wf2 [C][K]) | wpo ], b_out [C] = bpo + wpo . bf2; all dense, any C and K
extern "C" int dmx_test_compose_linear(const void* wpo, const void* wf2, const float* bf2, const float* bpo, void* w_out, float* b_out, int C, int K, dmx_stream_t stream) {
  DMX_REQUIRE(wpo && wf2 && bf2 && bpo && w_out && b_out && C > 0 && K > 0, "test_compose_linear: bad argument");
  return dmx_compose_linear_launch((const bf16*)wpo, (const bf16*)wf2, bf2, bpo, (bf16*)w_out, b_out, C, K, ST(stream));
}
// The folded tail of a transformer block as the UNet walk runs it (unet.hip Fwd::xformer + the GroupNorm behind the block), on the executor:
//   y = [g | h3] wfpo^T + bfpo + x  (Exec::conv, two K segments; g [B*HW][4C], h3 / x [B*HW][C], wfpo [C][5C]),  t = GroupNorm(y; groups, eps 1e-5, no activation)
// mode 0: the GEMM completes y itself;  1: ConvOpts.defer - a split-K plan leaves its reduce pass to the GroupNorm, x (the residual that pass
// adds) is dropped after it;  2: the same, but x is dropped BEFORE the GroupNorm (Exec::drop completes y first).  y and t are copied out dense.
static int folded_tail_gn(Exec& ex, const void* g, const void* h3, const void* x, const void* wfpo, const float* bfpo, const float* gamma, const float* beta,
                          int B, int HW, int C, int groups, int mode, void* y_out, void* t_out) {
  auto ext = [&](const void* p, int c) { Tn t; t.p = (bf16*)p; t.B = B; t.H = 1; t.W = HW; t.C = c; t.ld = c; return t; };      // (not workspace memory: drop only runs the pending-reduce rule)
  const Tn tg = ext(g, 4 * C), th3 = ext(h3, C), tx = ext(x, C);
  ConvOpts o; o.ksize = 1; o.pad = 0; o.bias = bfpo; o.res = &tx; o.defer = mode ? 2 : 0;
  Tn y = ex.conv(tg, &th3, (const bf16*)wfpo, C, o);
  if (mode == 2) ex.drop(tx);
  Tn t = ex.groupnorm(y, nullptr, gamma, beta, groups, 1e-5f, false);
  if (mode != 2) ex.drop(tx);
  if (!ex.dry && !ex.rc) {
    const size_t nb = (size_t)B * HW * C * sizeof(bf16);
    DMX_HIP(hipMemcpyAsync(y_out, y.p, nb, hipMemcpyDeviceToDevice, ex.stream));
    DMX_HIP(hipMemcpyAsync(t_out, t.p, nb, hipMemcpyDeviceToDevice, ex.stream));
  }
  ex.drop(t); ex.drop(y);
  return ex.rc;
}
extern "C" size_t dmx_test_folded_tail_gn_workspace_bytes(int B, int HW, int C, int groups, int mode) {
  Exec ex = Exec::dry_run();
  folded_tail_gn(ex, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, B, HW, C, groups, mode, nullptr, nullptr);
  return ex.ws.peak() + 4096;
}
extern "C" int dmx_test_folded_tail_gn(const void* g, const void* h3, const void* x, const void* wfpo, const float* bfpo, const float* gamma, const float* beta,
                                       int B, int HW, int C, int groups, int mode, void* y_out, void* t_out, void* workspace, size_t workspace_bytes, dmx_stream_t stream) {
  DMX_REQUIRE(g && h3 && x && wfpo && bfpo && gamma && beta && y_out && t_out && workspace, "test_folded_tail_gn: null argument");
  DMX_REQUIRE(B > 0 && HW > 0 && C > 0 && C % 64 == 0 && groups > 0 && C % groups == 0 && mode >= 0 && mode <= 2, "test_folded_tail_gn: bad shape or mode");
  Exec ex = Exec::on(ST(stream), workspace, workspace_bytes);
  return folded_tail_gn(ex, g, h3, x, wfpo, bfpo, gamma, beta, B, HW, C, groups, mode, y_out, t_out);
}
// out (16) [B][Spad][C] = in (fp32, or 16-bit with in_is_16) [B][S][C], rows >= S zero
extern "C" int dmx_test_cast_pad_rows(const void* in, int in_is_16, void* out, int B, int S, int Spad, int C, dmx_stream_t stream) {
  DMX_REQUIRE(in && out && B > 0 && S > 0 && Spad >= S && C > 0, "test_cast_pad_rows: bad argument");
  return dmx_cast_pad_rows_launch(in, in_is_16, (bf16*)out, B, S, Spad, C, ST(stream));
}
