// UNet2DConditionModel executor (SD2-inpainting layout): the graph behind
// `unet(sample, timestep, encoder_hidden_states).sample` (reference call sites
// app.ipynb:814, train_diffute_v1.py:913; module structure SURVEY.md Appendix A.1).
//
// The graph is walked on the host and every op is one of the hand-written gfx950 kernels.
// Fusions relative to the eager diffusers graph:
//   - torch.cat([latents, mask, masked_latents]) + NCHW->NHWC + fp32->bf16 + conv_in im2col: one kernel
//   - skip-connection torch.cat: never materialised (GroupNorm and the shortcut read two sources)
//   - conv1 + bias + time-embedding broadcast add: one launch
//   - conv2 + 1x1 conv_shortcut + residual add: one launch (shortcut appended as extra K)
//   - nearest x2 upsample: folded into the following conv's gather
//   - to_q|to_k|to_v one GEMM (N = 3C); the attention kernel reads V row-major through LDS transpose reads
//   - GEGLU: Linear(C,8C) + a*gelu(b) in one launch; every Linear bias / residual in the GEMM epilogue
//   - all 22 time_emb_proj Linear layers: one GEMV launch
//   - cross-attention K / V^T of the glyph context computed once per image (set_context)
#include <stdlib.h>
#include <math.h>
#include "unet_model.h"

namespace {

void build_resnet(dmx_unet* u, ResW& r, const std::string& p, int cin, int cout, bool temb) {
  resnet_build(u->pt, r, p, cin, cout);
  if (temb) { r.temb_off = u->tproj_total; u->tproj_total += cout; }   // rows of the batched time_emb_proj matrix
}

void build_xf(dmx_unet* u, XfW& x, const std::string& p, int C, int heads) {
  ParamTable& pt = u->pt;
  const int ctx = u->cfg.cross_attention_dim;
  x.C = C; x.heads = heads;
  x.ng = pt.f32(p + "norm.weight", C); x.nb = pt.f32(p + "norm.bias", C);
  x.wpi = pt.linear(p + "proj_in.weight", C, C); x.bpi = pt.f32(p + "proj_in.bias", C);
  const std::string t = p + "transformer_blocks.0.";
  x.l1g = pt.f32(t + "norm1.weight", C); x.l1b = pt.f32(t + "norm1.bias", C);
  x.wqkv_raw = pt.reserve((size_t)3 * C * C * 2);                  // to_q | to_k | to_v stacked: one GEMM, N = 3C
  pt.linear_at(t + "attn1.to_q.weight", C, C, x.wqkv_raw, C);
  pt.linear_at(t + "attn1.to_k.weight", C, C, x.wqkv_raw + (size_t)C * C * 2, C);
  pt.linear_at(t + "attn1.to_v.weight", C, C, x.wqkv_raw + (size_t)2 * C * C * 2, C);
  x.wqkv = pt.reserve((size_t)3 * C * C * 2);                      // norm1's gamma folded in (finalize)
  x.c1_qkv = pt.reserve((size_t)3 * C * 4); x.c2_qkv = pt.reserve((size_t)3 * C * 4);
  x.wo1 = pt.linear(t + "attn1.to_out.0.weight", C, C); x.bo1 = pt.f32(t + "attn1.to_out.0.bias", C);
  x.l2g = pt.f32(t + "norm2.weight", C); x.l2b = pt.f32(t + "norm2.bias", C);
  x.wq2_raw = pt.linear(t + "attn2.to_q.weight", C, C);
  x.wq2 = pt.reserve((size_t)C * C * 2); x.c1_q2 = pt.reserve((size_t)C * 4); x.c2_q2 = pt.reserve((size_t)C * 4);
  x.wkv2 = pt.reserve((size_t)2 * C * ctx * 2);                    // to_k | to_v stacked (context projections)
  pt.linear_at(t + "attn2.to_k.weight", C, ctx, x.wkv2, ctx);
  pt.linear_at(t + "attn2.to_v.weight", C, ctx, x.wkv2 + (size_t)C * ctx * 2, ctx);
  x.wo2 = pt.linear(t + "attn2.to_out.0.weight", C, C); x.bo2 = pt.f32(t + "attn2.to_out.0.bias", C);
  x.l3g = pt.f32(t + "norm3.weight", C); x.l3b = pt.f32(t + "norm3.bias", C);
  { PackRule r; r.kind = PackRule::GEGLU_W; r.dst = pt.reserve((size_t)8 * C * C * 2); r.rows = 8 * C; r.cols = C; r.ld = C;
    pt.add(t + "ff.net.0.proj.weight", {8 * C, C}, r); x.wf1_raw = r.dst; }
  x.wf1 = pt.reserve((size_t)8 * C * C * 2); x.c1_f1 = pt.reserve((size_t)8 * C * 4); x.c2_f1 = pt.reserve((size_t)8 * C * 4);
  { PackRule r; r.kind = PackRule::GEGLU_B; r.dst = pt.reserve((size_t)8 * C * 4); r.rows = 8 * C;
    pt.add(t + "ff.net.0.proj.bias", {8 * C}, r); x.bf1 = r.dst; }
  x.wf2 = pt.linear(t + "ff.net.2.weight", C, 4 * C); x.bf2 = pt.f32(t + "ff.net.2.bias", C);
  x.wpo = pt.linear(p + "proj_out.weight", C, C); x.bpo = pt.f32(p + "proj_out.bias", C);
  x.wfpo = pt.reserve((size_t)C * 5 * C * 2); x.bfpo = pt.reserve((size_t)C * 4);      // derived: [Wpo Wf2 | Wpo], bpo + Wpo bf2 (fold_ready)
}

}  // namespace

extern "C" dmx_unet* dmx_unet_create(const dmx_unet_config* cfg) {
  if (!cfg) { dmx_set_error("unet_create: null config"); return nullptr; }
  for (int i = 0; i < 4; ++i) {
    const int c = cfg->block_out_channels[i];
    if (c % 64 != 0 || c % cfg->norm_num_groups != 0 || (cfg->heads[i] > 0 && c / cfg->heads[i] != 64)) {
      dmx_set_error("unet_create: block_out_channels[%d]=%d must be a multiple of 64 with head dim 64", i, c);
      return nullptr;
    }
  }
  if (cfg->cross_attention_dim % 64 != 0) { dmx_set_error("unet_create: cross_attention_dim must be a multiple of 64"); return nullptr; }
  auto u = std::make_unique<dmx_unet>();
  u->cfg = *cfg;
  ParamTable& pt = u->pt;
  const int* boc = cfg->block_out_channels; const int L = cfg->layers_per_block;
  const int temb = boc[0] * 4; u->temb_dim = temb;
  u->te_w1 = pt.linear("time_embedding.linear_1.weight", temb, boc[0]); u->te_b1 = pt.f32("time_embedding.linear_1.bias", temb);
  u->te_w2 = pt.linear("time_embedding.linear_2.weight", temb, temb); u->te_b2 = pt.f32("time_embedding.linear_2.bias", temb);
  u->freq = pt.reserve((size_t)(boc[0] / 2) * 4);
  u->ci_kpad = (int)align_up((size_t)9 * cfg->in_channels, 64);
  u->ci_w = pt.reserve((size_t)boc[0] * u->ci_kpad * 2);
  pt.conv_at("conv_in.weight", boc[0], cfg->in_channels, 3, u->ci_w, u->ci_kpad, 0);
  u->ci_b = pt.f32("conv_in.bias", boc[0]);
  std::vector<int> skips; skips.push_back(boc[0]);
  int cprev = boc[0];
  for (int i = 0; i < 4; ++i) {
    const int c = boc[i];
    u->down_res[i].resize(L); if (cfg->down_has_attn[i]) u->down_xf[i].resize(L);
    for (int j = 0; j < L; ++j) {
      const std::string p = "down_blocks." + std::to_string(i);
      build_resnet(u.get(), u->down_res[i][j], p + ".resnets." + std::to_string(j) + ".", cprev, c, true);
      if (cfg->down_has_attn[i]) build_xf(u.get(), u->down_xf[i][j], p + ".attentions." + std::to_string(j) + ".", c, cfg->heads[i]);
      cprev = c; skips.push_back(c);
    }
    if (i < 3) {
      const std::string p = "down_blocks." + std::to_string(i) + ".downsamplers.0.conv.";
      u->down_ds[i].c = c; u->down_ds[i].w = pt.reserve((size_t)c * 9 * c * 2);
      pt.conv_at(p + "weight", c, c, 3, u->down_ds[i].w, 9 * c, 0);
      u->down_ds[i].b = pt.f32(p + "bias", c);
      skips.push_back(c);
    }
  }
  build_resnet(u.get(), u->mid_res[0], "mid_block.resnets.0.", cprev, cprev, true);
  build_xf(u.get(), u->mid_xf, "mid_block.attentions.0.", cprev, cfg->heads[3]);
  build_resnet(u.get(), u->mid_res[1], "mid_block.resnets.1.", cprev, cprev, true);
  for (int i = 0; i < 4; ++i) {
    const int c = boc[3 - i];
    u->up_res[i].resize(L + 1); if (cfg->up_has_attn[i]) u->up_xf[i].resize(L + 1);
    for (int j = 0; j < L + 1; ++j) {
      const int cs = skips.back(); skips.pop_back();
      const std::string p = "up_blocks." + std::to_string(i);
      build_resnet(u.get(), u->up_res[i][j], p + ".resnets." + std::to_string(j) + ".", cprev + cs, c, true);
      if (cfg->up_has_attn[i]) build_xf(u.get(), u->up_xf[i][j], p + ".attentions." + std::to_string(j) + ".", c, cfg->heads[3 - i]);
      cprev = c;
    }
    if (i < 3) {
      const std::string p = "up_blocks." + std::to_string(i) + ".upsamplers.0.conv.";
      u->up_us[i].c = c; u->up_us[i].w = pt.reserve((size_t)c * 9 * c * 2);
      pt.conv_at(p + "weight", c, c, 3, u->up_us[i].w, 9 * c, 0);
      u->up_us[i].b = pt.f32(p + "bias", c);
      u->up_us[i].wp = pt.reserve((size_t)4 * c * 4 * c * 2);      // derived: phase weights of the upsample conv (refresh_derived)
    }
  }
  u->cno_g = pt.f32("conv_norm_out.weight", boc[0]); u->cno_b = pt.f32("conv_norm_out.bias", boc[0]);
  u->co_w = pt.reserve((size_t)cfg->out_channels * 9 * boc[0] * 2);
  pt.conv_at("conv_out.weight", cfg->out_channels, boc[0], 3, u->co_w, 9 * boc[0], 0);
  u->co_b = pt.f32("conv_out.bias", cfg->out_channels);

  // time_emb_proj of every resnet: rows of one [tproj_total][temb] matrix (+ bias vector)
  u->tp_w = pt.reserve((size_t)u->tproj_total * temb * 2);
  u->tp_b = pt.reserve((size_t)u->tproj_total * 4);
  auto reg_tp = [&](const ResW& r, const std::string& p) {
    pt.linear_at(p + "time_emb_proj.weight", r.cout, temb, u->tp_w + (size_t)r.temb_off * temb * 2, temb);
    pt.f32_at(p + "time_emb_proj.bias", r.cout, u->tp_b + (size_t)r.temb_off * 4);
  };
  for (int i = 0; i < 4; ++i)
    for (int j = 0; j < L; ++j) reg_tp(u->down_res[i][j], "down_blocks." + std::to_string(i) + ".resnets." + std::to_string(j) + ".");
  reg_tp(u->mid_res[0], "mid_block.resnets.0."); reg_tp(u->mid_res[1], "mid_block.resnets.1.");
  for (int i = 0; i < 4; ++i)
    for (int j = 0; j < L + 1; ++j) reg_tp(u->up_res[i][j], "up_blocks." + std::to_string(i) + ".resnets." + std::to_string(j) + ".");

  // cross-attention context slots in graph order
  for (int i = 0; i < 4; ++i) for (auto& x : u->down_xf[i]) u->xf_all.push_back(&x);
  u->xf_all.push_back(&u->mid_xf);
  for (int i = 0; i < 4; ++i) for (auto& x : u->up_xf[i]) u->xf_all.push_back(&x);
  for (size_t s = 0; s < u->xf_all.size(); ++s) u->xf_all[s]->ctx_slot = (int)s;
  return u.release();
}

DMX_MODEL_ABI(dmx_unet, unet)

// Recompute everything derived from the raw weights in the arena (folded shortcut biases, LayerNorm-folded GEMM
// weights and their c1 / c2 vectors) after the raw weights changed in place (fused optimizer); asynchronous.
static int refresh_derived(dmx_unet* u, hipStream_t s) {
  u->fold_stale = true;                                // (the composed ff.net.2 / proj_out weights follow at the next inference entry: fold_ready)
  int rc = for_each_resnet(u, [&](const ResW& r) { return resnet_finalize(r, u->arena, s); });
  for (int i = 0; i < 3 && !rc; ++i)
    rc = dmx_ups_phase_weights_launch(u->at<bf16>(u->up_us[i].w), 9 * u->up_us[i].c, u->at<bf16>(u->up_us[i].wp), u->up_us[i].c, u->up_us[i].c, s);
  // fold norm1/2/3 of every BasicTransformerBlock into the GEMM that consumes it (W' = W*gamma, c1, c2)
  for (const XfW* x : u->xf_all) {
    const int C = x->C;
    if (!rc) rc = dmx_ln_fold_launch(u->at<bf16>(x->wqkv_raw), u->at<bf16>(x->wqkv), u->at<float>(x->l1g), u->at<float>(x->l1b), nullptr,
                                     u->at<float>(x->c1_qkv), u->at<float>(x->c2_qkv), 3 * C, C, s);
    if (!rc) rc = dmx_ln_fold_launch(u->at<bf16>(x->wq2_raw), u->at<bf16>(x->wq2), u->at<float>(x->l2g), u->at<float>(x->l2b), nullptr,
                                     u->at<float>(x->c1_q2), u->at<float>(x->c2_q2), C, C, s);
    if (!rc) rc = dmx_ln_fold_launch(u->at<bf16>(x->wf1_raw), u->at<bf16>(x->wf1), u->at<float>(x->l3g), u->at<float>(x->l3b), u->at<float>(x->bf1),
                                     u->at<float>(x->c1_f1), u->at<float>(x->c2_f1), 8 * C, C, s);
  }
  return rc;
}
// The composed weights of dmx_set_ff_fold, once per weights change, at the entry of an inference call: on the call's stream, in front of its
// launches and - every caller asks before its own hipStreamBeginCapture - outside the library's graph capture.  Where the CALLER is capturing
// the stream, the two launches per block become nodes of the caller's graph and the weights stay marked stale: nothing has run yet.
// Two things follow from composing lazily, both the caller's to order (include/diffute_hip.h dmx_set_ff_fold):
//   - the mark is cleared when the launches are ENQUEUED on `s`: an inference call on another stream right afterwards is not ordered behind
//     them (dmx_unet_refresh_derived's own launches have the same contract with the stream they were given);
//   - a graph the CALLER captured around an inference call while the fold was fresh holds no composition: replayed after a weights change it
//     reads composed weights that are stale until some inference entry of the library has run on the new weights (they are rebuilt in place).
static int fold_ready(dmx_unet* u, hipStream_t s) {
  if (!u->fold_stale || !dmx_ff_fold_enabled()) return DMX_OK;
  hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
  if (s != nullptr && hipStreamIsCapturing(s, &cs) != hipSuccess) { (void)hipGetLastError(); cs = hipStreamCaptureStatusNone; }
  for (const XfW* x : u->xf_all)
    if (const int rc = dmx_compose_linear_launch(u->at<bf16>(x->wpo), u->at<bf16>(x->wf2), u->at<float>(x->bf2), u->at<float>(x->bpo),
                                                 u->at<bf16>(x->wfpo), u->at<float>(x->bfpo), x->C, 4 * x->C, s)) return rc;
  if (cs == hipStreamCaptureStatusNone) u->fold_stale = false;
  return DMX_OK;
}
extern "C" int dmx_unet_refresh_derived(dmx_unet* u, dmx_stream_t stream) {
  DMX_REQUIRE(u && u->arena && u->finalized, "unet_refresh_derived: weights not finalized");
  u->drop_graphs();
  return refresh_derived(u, (hipStream_t)stream);
}

int dmx_unet::derive(hipStream_t s) {
  drop_graphs();
  int rc = refresh_derived(this, s);
  const bf16* zp = nullptr;
  if (!rc) rc = dmx_zero_page(&zp);                  // allocate the padding page now, never inside a stream capture
  return rc;
}
extern "C" int dmx_unet_finalize(dmx_unet* u, const float* h_freq, dmx_stream_t stream) {
  DMX_REQUIRE(u && u->arena, "unet_finalize: arena not bound");
  DMX_REQUIRE(h_freq != nullptr, "unet_finalize: null frequency table");
  DMX_HIP(hipMemcpyAsync(u->arena + u->freq, h_freq, (size_t)(u->cfg.block_out_channels[0] / 2) * 4, hipMemcpyHostToDevice, (hipStream_t)stream));
  return model_finalize(u, "unet", (hipStream_t)stream);
}

// ----------------------------------------------------------------------------- context
static int ctx_pad(int ctx_len) { return dmx_ctx_pad(ctx_len); }

extern "C" size_t dmx_unet_context_bytes(const dmx_unet* u, int B, int ctx_len) {
  if (!u) return 0;
  size_t tot = 0;
  const int sp = ctx_pad(ctx_len);
  for (const XfW* x : u->xf_all) tot += align_up((size_t)B * sp * 2 * x->C * 2, 256);
  return tot;
}
// context cache slot of one cross-attention layer: [B*sp][2C] bf16, columns [0,C) = K, [C,2C) = V
static const bf16* ctx_slot_ptr(const dmx_unet* u, const void* cache, int B, int ctx_len, int slot) {
  size_t off = 0; const int sp = ctx_pad(ctx_len);
  for (int s = 0; s < slot; ++s) off += align_up((size_t)B * sp * 2 * u->xf_all[s]->C * 2, 256);
  return (const bf16*)((const char*)cache + off);
}

// The K / V projection of n context rows (ctx [n][ctx_len][D]) into rows [row0, row0 + n) of a cache laid out for B rows: row b of every
// layer's [B*sp][2C] slab is the contiguous [sp][2C] block at b*sp, so the GEMM's M is n*sp and its output starts at row row0*sp - rows
// outside are not touched.  On a dry Exec (the workspace query) nothing is launched.
static int project_context(const dmx_unet* u, Exec& ex, const void* ctx, int ctx_is_bf16, int row0, int n, int B, int ctx_len, void* cache) {
  const int D = u->cfg.cross_attention_dim, sp = ctx_pad(ctx_len);
  bf16* cp = (bf16*)ex.raw((size_t)n * sp * D * 2);
  if (ex.rc) return ex.rc;
  if (!ex.dry) ex.rc = dmx_cast_pad_rows_launch(ctx, ctx_is_bf16, cp, n, ctx_len, sp, D, ex.stream);
  if (ex.rc) return ex.rc;
  for (const XfW* x : u->xf_all) {
    // [K | V][b*sp + s][2C] = ctx [W_k ; W_v]^T   (padded context rows are zero -> finite K/V rows)
    const bf16* kv = ex.dry ? nullptr : ctx_slot_ptr(u, cache, B, ctx_len, x->ctx_slot) + (size_t)row0 * sp * 2 * x->C;
    ex.gemm_raw(cp, D, n * sp, ex.dry ? nullptr : u->at<bf16>(x->wkv2), D, 2 * x->C, D, nullptr, (void*)kv, 2 * x->C, 0);
    if (ex.rc) return ex.rc;
  }
  return ex.rc;
}

extern "C" int dmx_unet_set_context(dmx_unet* u, const void* ctx, int ctx_is_bf16, int B, int ctx_len,
                                    void* cache, size_t cache_bytes, void* workspace, size_t workspace_bytes, dmx_stream_t stream) {
  DMX_REQUIRE(u && u->finalized, "unet_set_context: weights not finalized");
  DMX_REQUIRE(ctx && cache && cache_bytes >= dmx_unet_context_bytes(u, B, ctx_len), "unet_set_context: context cache too small");
  Exec ex = Exec::on((hipStream_t)stream, workspace, workspace_bytes);
  return project_context(u, ex, ctx, ctx_is_bf16, 0, B, B, ctx_len, cache);
}
extern "C" int dmx_unet_set_context_rows(dmx_unet* u, const void* ctx, int ctx_is_bf16, int row0, int n, int B, int ctx_len,
                                         void* cache, size_t cache_bytes, void* workspace, size_t workspace_bytes, dmx_stream_t stream) {
  DMX_REQUIRE(u && u->finalized, "unet_set_context_rows: weights not finalized");
  DMX_REQUIRE(B >= 1 && n >= 1 && row0 >= 0 && row0 <= B - n, "unet_set_context_rows: rows [%d, %d) of a cache of %d rows", row0, row0 + n, B);
  DMX_REQUIRE(ctx_len >= 1, "unet_set_context_rows: ctx_len %d", ctx_len);
  DMX_REQUIRE(ctx && cache && cache_bytes >= dmx_unet_context_bytes(u, B, ctx_len), "unet_set_context_rows: context cache too small");
  Exec ex = Exec::on((hipStream_t)stream, workspace, workspace_bytes);
  return project_context(u, ex, ctx, ctx_is_bf16, row0, n, B, ctx_len, cache);
}

// ----------------------------------------------------------------------------- forward
namespace {

struct Fwd {
  dmx_unet* u; Exec& ex; int B; const float* tproj; int tp_ld; const void* cache; int ctx_len;
  Exec::Weights wt;                 // the packed bf16 arena or, in fp32 validation mode, the fp32 master arena
  template <typename T> const T* W(size_t off) const { return wt.at<T>(off); }

  Tn resnet(const ResW& r, const Tn& x0, const Tn* x1) {
    return resnet_run(ex, u->arena, r, x0, x1, u->cfg.norm_num_groups, 1e-5f, tproj, tp_ld);
  }

  // fp32 validation mode: the same block with explicit LayerNorms on the RAW weights (the folded copies are derived data of
  // the bf16 path) and the context K / V projected in place (`cache` is the fp32 context [B*ctx_len][cross_attention_dim])
  Tn xformer_f32(const XfW& w, const Tn& x) {
    const int G = u->cfg.norm_num_groups, C = w.C, S = x.H * x.W, D = u->cfg.cross_attention_dim;
    auto F = [&](size_t off) { return W<float>(off); };
    auto H = [&](size_t off) { return W<bf16>(off); };
    Tn t = ex.groupnorm(x, nullptr, F(w.ng), F(w.nb), G, 1e-6f, false);
    Tn h = ex.linear(t, H(w.wpi), C, F(w.bpi), nullptr, false); ex.drop(t);
    Tn n = ex.layernorm(h, F(w.l1g), F(w.l1b), 1e-5f);
    Tn qkv = ex.linear(n, H(w.wqkv_raw), 3 * C, nullptr, nullptr, false); ex.drop(n);
    Tn a = ex.make(x.B, x.H, x.W, C);
    ex.attention(qkv.p, 3 * C, ex.col(qkv, C), 3 * C, ex.col(qkv, 2 * C), 3 * C, S, a.p, C, x.B, w.heads, S, S, 0.125f);
    ex.drop(qkv);
    Tn h2 = ex.linear(a, H(w.wo1), C, F(w.bo1), &h, false); ex.drop(a); ex.drop(h);
    n = ex.layernorm(h2, F(w.l2g), F(w.l2b), 1e-5f);
    Tn q = ex.linear(n, H(w.wq2_raw), C, nullptr, nullptr, false); ex.drop(n);
    Tn cx; cx.p = (bf16*)cache; cx.B = x.B; cx.H = 1; cx.W = ctx_len; cx.C = D; cx.ld = D;
    Tn kv = ex.linear(cx, H(w.wkv2), 2 * C, nullptr, nullptr, false);
    a = ex.make(x.B, x.H, x.W, C);
    ex.attention(q.p, C, kv.p, 2 * C, ex.col(kv, C), 2 * C, ctx_len, a.p, C, x.B, w.heads, S, ctx_len, 0.125f);
    ex.drop(q); ex.drop(kv);
    Tn h3 = ex.linear(a, H(w.wo2), C, F(w.bo2), &h2, false); ex.drop(a); ex.drop(h2);
    n = ex.layernorm(h3, F(w.l3g), F(w.l3b), 1e-5f);
    Tn g = ex.linear(n, H(w.wf1_raw), 8 * C, F(w.bf1), nullptr, true); ex.drop(n);
    Tn h4 = ex.linear(g, H(w.wf2), C, F(w.bf2), &h3, false); ex.drop(g); ex.drop(h3);
    Tn y = ex.linear(h4, H(w.wpo), C, F(w.bpo), &x, false); ex.drop(h4);
    return y;
  }

  Tn xformer(const XfW& w, const Tn& x) {
    if (ex.f32) return xformer_f32(w, x);
    const int G = u->cfg.norm_num_groups, C = w.C, S = x.H * x.W;
    const bool chain = ex.chain_ok(x);     // C = 320 levels: the per-row GEMM chains around the two attention cores are three kernels (xf_chain.hip)
    // the entry GroupNorm rides in the first chain's operand load when x came with its statistics records (xf_chain.hip mode 2)
    const bool gn_fold = chain && ex.chain_gn_fold(x);
    if (gn_fold) ex.flush(x);                // (the chains read x through raw pointers; the GroupNorm below completes a pending x itself)
    Tn t = gn_fold ? x : ex.groupnorm(x, nullptr, u->at<float>(w.ng), u->at<float>(w.nb), G, 1e-6f, false);
    // LayerNorms are folded: each residual-stream producer also emits per-row (sum, sumsq) partials and the
    // consuming GEMM multiplies the raw rows by W*gamma and normalises in its epilogue - no LN kernels, no LN tensors.
    Exec::RowStats st1, st2, st3;
    Tn h, qkv;
    if (chain) {
      // [proj_in -> LN1 -> to_q | to_k | to_v]
      h = ex.make(x.B, x.H, x.W, C); qkv = ex.make(x.B, x.H, x.W, 3 * C);
      XfChainArgs c{};
      c.M = x.rows(); c.C = C; c.eps = 1e-5f;
      c.x = t.p; c.ldx = t.ld; c.w0 = u->at<bf16>(w.wpi); c.b0 = u->at<float>(w.bpi); c.h_out = h.p; c.ldh = h.ld;
      c.w1 = u->at<bf16>(w.wqkv); c.c1 = u->at<float>(w.c1_qkv); c.c2 = u->at<float>(w.c2_qkv); c.y = qkv.p; c.ldy = qkv.ld;
      if (gn_fold) { c.gn_st = x.cst; c.gn_gamma = u->at<float>(w.ng); c.gn_beta = u->at<float>(w.nb); c.gn_groups = G; c.gn_rows = S; c.gn_eps = 1e-6f; }
      ex.xf_chain(2, c);
      if (!gn_fold) ex.drop(t);
    } else {
      h = ex.linear(t, u->at<bf16>(w.wpi), C, u->at<float>(w.bpi), nullptr, false, &st1);
      ex.drop(t);
      // ---- self attention
      Exec::LnIn ln1; ln1.stats = st1.buf; ln1.tiles = st1.tiles; ln1.c1 = u->at<float>(w.c1_qkv); ln1.c2 = u->at<float>(w.c2_qkv);
      qkv = ex.linear(h, u->at<bf16>(w.wqkv), 3 * C, nullptr, nullptr, false, nullptr, &ln1);
      ex.drop(st1.buf);
    }
    Tn a = ex.make(x.B, x.H, x.W, C);
    ex.attention(qkv.p, 3 * C, qkv.p + C, 3 * C, qkv.p + 2 * C, 3 * C, S, a.p, C, x.B, w.heads, S, S, 0.125f);
    ex.drop(qkv);
    const int sp = ctx_pad(ctx_len);
    const bf16* kvc = ctx_slot_ptr(u, cache, x.B, ctx_len, w.ctx_slot);
    if (chain) {
      // [to_out + res -> LN2 -> to_q] and [to_out + res -> LN3 -> FF1 / GEGLU -> FF2 + res -> proj_out + res] around the cross-attention
      XfChainArgs c{};
      c.M = x.rows(); c.C = C; c.eps = 1e-5f;
      Tn h2 = ex.make(x.B, x.H, x.W, C), q = ex.make(x.B, x.H, x.W, C);
      c.x = a.p; c.ldx = a.ld; c.res = h.p; c.ldres = h.ld; c.w0 = u->at<bf16>(w.wo1); c.b0 = u->at<float>(w.bo1);
      c.h_out = h2.p; c.ldh = h2.ld; c.w1 = u->at<bf16>(w.wq2); c.c1 = u->at<float>(w.c1_q2); c.c2 = u->at<float>(w.c2_q2);
      c.y = q.p; c.ldy = q.ld;
      ex.xf_chain(0, c);
      ex.drop(a); ex.drop(h);
      a = ex.make(x.B, x.H, x.W, C);
      ex.attention(q.p, C, kvc, 2 * C, kvc + C, 2 * C, sp, a.p, C, x.B, w.heads, S, ctx_len, 0.125f, true);
      ex.drop(q);
      Tn h3 = ex.make(x.B, x.H, x.W, C), y = ex.make(x.B, x.H, x.W, C);
      XfChainArgs d{};
      d.M = x.rows(); d.C = C; d.eps = 1e-5f;
      d.x = a.p; d.ldx = a.ld; d.res = h2.p; d.ldres = h2.ld; d.w0 = u->at<bf16>(w.wo2); d.b0 = u->at<float>(w.bo2);
      d.h_out = h3.p; d.ldh = h3.ld; d.c1 = u->at<float>(w.c1_f1); d.c2 = u->at<float>(w.c2_f1);
      d.wf1 = u->at<bf16>(w.wf1); d.wf2 = u->at<bf16>(w.wf2); d.bf2 = u->at<float>(w.bf2);
      d.wpo = u->at<bf16>(w.wpo); d.bpo = u->at<float>(w.bpo); d.xres = x.p; d.ldxres = x.ld;
      d.y = y.p; d.ldy = y.ld;
      ex.chain_stats(d, y);                            // (statistics records of y for the GroupNorm -> conv launch that reads it next)
      ex.xf_chain(1, d);
      ex.drop(a); ex.drop(h2); ex.drop(h3);
      return y;
    }
    Tn h2 = ex.linear(a, u->at<bf16>(w.wo1), C, u->at<float>(w.bo1), &h, false, &st2);
    ex.drop(a); ex.drop(h);
    // ---- cross attention over the cached glyph-context K / V
    Exec::LnIn ln2; ln2.stats = st2.buf; ln2.tiles = st2.tiles; ln2.c1 = u->at<float>(w.c1_q2); ln2.c2 = u->at<float>(w.c2_q2);
    Tn q = ex.linear(h2, u->at<bf16>(w.wq2), C, nullptr, nullptr, false, nullptr, &ln2);
    ex.drop(st2.buf);
    a = ex.make(x.B, x.H, x.W, C);
    ex.attention(q.p, C, kvc, 2 * C, kvc + C, 2 * C, sp, a.p, C, x.B, w.heads, S, ctx_len, 0.125f, true);
    ex.drop(q);
    Tn h3 = ex.linear(a, u->at<bf16>(w.wo2), C, u->at<float>(w.bo2), &h2, false, &st3);
    ex.drop(a); ex.drop(h2);
    // ---- GEGLU feed-forward
    Exec::LnIn ln3; ln3.stats = st3.buf; ln3.tiles = st3.tiles; ln3.c1 = u->at<float>(w.c1_f1); ln3.c2 = u->at<float>(w.c2_f1);
    Tn g = ex.linear(h3, u->at<bf16>(w.wf1), 8 * C, nullptr, nullptr, true, nullptr, &ln3);
    ex.drop(st3.buf);
    if (ex.ff_fold) {
      // ff.net.2 + residual and proj_out + block residual as ONE GEMM with two K segments: y = [g | h3] [Wpo Wf2 | Wpo]^T + (Wpo bf2 + bpo) + x.
      // It is the block's last op and a GroupNorm reads y next, so a split-K plan leaves its reduce pass to that GroupNorm (defer = 2, like a
      // resnet's conv2): the caller keeps x - the residual that pass adds - alive until then (Exec::drop of x would complete y first).
      ConvOpts o; o.ksize = 1; o.pad = 0; o.bias = u->at<float>(w.bfpo); o.res = &x; o.stats = 1; o.defer = 2;
      Tn y = ex.conv(g, &h3, u->at<bf16>(w.wfpo), C, o);
      ex.drop(g); ex.drop(h3);
      return y;
    }
    Tn h4 = ex.linear(g, u->at<bf16>(w.wf2), C, u->at<float>(w.bf2), &h3, false);
    ex.drop(g); ex.drop(h3);
    Tn y = ex.linear(h4, u->at<bf16>(w.wpo), C, u->at<float>(w.bpo), &x, false, nullptr, nullptr, true);   // (+ GroupNorm statistics for the next block)
    ex.drop(h4);
    return y;
  }
};

// a row of the precomputed time-embedding projection table -> the buffer every resnet's conv1 reads its row bias from.  Grid (chunks, 1):
// the scalar form, row index[0] into row 0 (every image reads it with row stride 0).  Grid (chunks, B) with a plan: image b fetches row
// max(index[b], 0) (an idle row reads row 0: finite, ignored) and the first thread of each image's first block writes that plan row's
// timestep into the forward's timesteps buffer.
__global__ __launch_bounds__(256) void dmx_temb_fetch_kernel(const float* table, const int* index, const dmx_sched_row_rec* plan, float* out,
                                                             long long* timesteps, int n) {
  const int b = blockIdx.y;
  int idx = index[b]; if (plan && idx < 0) idx = 0;
  const float* src = table + (size_t)idx * n;
  float* dst = out + (size_t)b * n;
  for (int i = blockIdx.x * 256 + threadIdx.x; i < n; i += gridDim.x * 256) dst[i] = src[i];
  if (plan && blockIdx.x == 0 && threadIdx.x == 0) timesteps[b] = (long long)plan[idx].timestep;
}

// Step cache hand-off (FILL): the tensor and, where it has them, its statistics records -> the caller's buffer, one launch behind the
// producer (the statistics pool is zeroed per forward and the producers ADD into it, so the records are final only after it).  16-byte units.
__global__ __launch_bounds__(256) void dmx_step_cache_store_kernel(const u32x4* t, u32x4* ct, size_t nt, const u32x4* st, u32x4* cs, size_t ns) {
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < nt + ns; i += (size_t)gridDim.x * blockDim.x) {
    if (i < nt) ct[i] = t[i];
    else cs[i - nt] = st[i - nt];
  }
}

}  // namespace

// layout of a step cache: the tensor [B*H*W][C1] (H, W: the forward's latent grid, where up-block 3 runs), then its [B][C1][4] records
static size_t step_cache_tensor_bytes(const dmx_unet* u, int B, int H, int W) { return (size_t)B * H * W * u->cfg.block_out_channels[1] * sizeof(bf16); }
static size_t step_cache_stat_bytes(const dmx_unet* u, int B) { return (size_t)B * u->cfg.block_out_channels[1] * DMX_STAT_WORDS * sizeof(long long); }
extern "C" size_t dmx_unet_step_cache_bytes(dmx_unet* u, int B, int H, int W) {
  if (!u || B <= 0 || H <= 0 || W <= 0) return 0;
  return align_up(step_cache_tensor_bytes(u, B, H, W), 256) + align_up(step_cache_stat_bytes(u, B), 256);
}

int temb_rows(const dmx_unet* u, Exec& ex, const long long* timesteps, int t_count, int rows, const TembBufs& b, float* tproj) {
  const int c0 = u->cfg.block_out_channels[0], temb = u->temb_dim;
  if (ex.dry || ex.rc) return ex.rc;
  ex.rc = dmx_timestep_embedding_launch(timesteps, t_count, u->at<float>(u->freq), rows, c0, b.sinus, ex.stream);
  if (!ex.rc) ex.rc = dmx_linear_small_launch(b.sinus, c0, u->at<bf16>(u->te_w1), c0, u->at<float>(u->te_b1), b.e1, temb, rows, temb, c0, 0, ex.stream);
  if (!ex.rc) ex.rc = dmx_linear_small_launch(b.e1, temb, u->at<bf16>(u->te_w2), temb, u->at<float>(u->te_b2), b.emb, temb, rows, temb, temb, 1, ex.stream);
  if (!ex.rc) ex.rc = dmx_linear_small_launch(b.emb, temb, u->at<bf16>(u->tp_w), temb, u->at<float>(u->tp_b), tproj, u->tproj_total, rows, u->tproj_total, temb, 1, ex.stream);
  return ex.rc;
}
// the projections of all T timesteps of a denoise loop in one batched pass (each row is computed exactly as the per-step path computes its single row)
static int temb_table_run(dmx_unet* u, Exec& ex, const long long* timesteps, int T, float* table) {
  const TembBufs b(u, ex, T);
  temb_rows(u, ex, timesteps, T, T, b, table);
  b.drop(ex);
  return ex.rc;
}
extern "C" size_t dmx_unet_temb_table_floats(dmx_unet* u, int T) { return u ? (size_t)T * u->tproj_total : 0; }
extern "C" size_t dmx_unet_temb_table_workspace_bytes(dmx_unet* u, int T) {
  if (!u) return 0;
  Exec ex = Exec::dry_run();
  temb_table_run(u, ex, nullptr, T, nullptr);
  return ex.ws.peak() + 4096;
}
extern "C" int dmx_unet_temb_table(dmx_unet* u, const int64_t* timesteps, int T, float* table, void* workspace, size_t workspace_bytes, dmx_stream_t stream) {
  DMX_REQUIRE(u && u->finalized, "unet_temb_table: weights not finalized");
  DMX_REQUIRE(timesteps && table && workspace && T > 0, "unet_temb_table: null argument");
  Exec ex = Exec::on((hipStream_t)stream, workspace, workspace_bytes);
  return temb_table_run(u, ex, (const long long*)timesteps, T, table);
}
// each setter fills the one source; its all-NULL call clears it only while it holds that setter's own form
extern "C" int dmx_unet_use_temb_table(dmx_unet* u, const float* table, const int* step_index) {
  DMX_REQUIRE(u != nullptr, "unet_use_temb_table: null handle");
  DMX_REQUIRE((table == nullptr) == (step_index == nullptr), "unet_use_temb_table: table and step index go together");
  if (table || !u->temb.plan) u->temb = {table, step_index, nullptr};
  return DMX_OK;
}
extern "C" int dmx_unet_use_temb_table_rows(dmx_unet* u, const float* table, const dmx_sched_row_rec* plan, const int* row_index) {
  DMX_REQUIRE(u != nullptr, "unet_use_temb_table_rows: null handle");
  DMX_REQUIRE((table == nullptr) == (row_index == nullptr) && (table == nullptr) == (plan == nullptr), "unet_use_temb_table_rows: table, plan and row index go together");
  if (table || u->temb.plan) u->temb = {table, row_index, plan};
  return DMX_OK;
}

int unet_check_call(const dmx_unet* u, const UNetCall& c, const void* workspace, const char* who) {
  DMX_REQUIRE(u && u->finalized, "%s: weights not finalized (bind_arena, load_param*, finalize)", who);
  DMX_REQUIRE(c.f0 && c.out && c.timesteps && c.ctx && workspace, "%s: null argument", who);
  DMX_REQUIRE(c.c0 + c.c1 + c.c2 == u->cfg.in_channels, "%s: c0+c1+c2=%d != in_channels=%d", who, c.c0 + c.c1 + c.c2, u->cfg.in_channels);
  DMX_REQUIRE(c.B > 0 && c.H > 0 && c.W > 0 && c.H % 8 == 0 && c.W % 8 == 0, "%s: H=%d W=%d must be positive multiples of 8", who, c.H, c.W);
  return DMX_OK;
}

namespace {

// One walk for the three forms of a step: sc.mode 0 / FILL run every layer (FILL also leaves the tensor that enters up-block 3 in the
// step cache), USE runs what lies around that tensor - conv_in, down-block 0 (for its three skips; its stride-2 conv has no reader),
// up-block 3 on the kept tensor, conv_norm_out, conv_out.
int unet_run(dmx_unet* u, Exec& ex, const UNetCall& c, StepCache& sc) {
  const int B = c.B, H = c.H, W = c.W, t_count = c.t_count;
  const bool shallow = sc.mode == DMX_STEP_CACHE_USE;
  bf16* const sc_t = (bf16*)sc.buf;
  long long* const sc_st = sc.buf ? (long long*)((char*)sc.buf + align_up(step_cache_tensor_bytes(u, B, H, W), 256)) : nullptr;
  const dmx_unet_config& cfg = u->cfg;
  const int* boc = cfg.block_out_channels; const int L = cfg.layers_per_block; const int temb = u->temb_dim;
  // ---- time embedding (fp32, bf16 weights).  A scalar timestep (the denoise loop) is embedded once and every image reads
  // row 0 of the projections (row stride 0); per-sample timesteps (training) get one row each.
  const int Bt = (t_count == 1) ? 1 : B;
  const int tp_ld = (t_count == 1) ? 0 : u->tproj_total;
  const TembBufs te(u, ex, B);                                        // sized for B rows either way (workspace query)
  float* const sinus = te.sinus; float* const e1 = te.e1; float* const emb = te.emb;
  float* tproj = (float*)ex.raw((size_t)B * u->tproj_total * 4);
  Fwd f{u, ex, B, tproj, tp_ld, c.ctx, c.ctx_len, ex.weights(u->arena)};
  Tn h;
  if (ex.f32) {
    // fp32 validation mode: same layers on the fp32 masters through the generic fp32 GEMM (SiLU as its own tiny pass)
    auto small = [&](float* x, int K, size_t w, size_t b, int N, float* y) {
      if (ex.dry || ex.rc) return;
      GemmF32Args a{}; a.x0 = a.x1 = x; a.ldx0 = a.ldx1 = K; a.cx0 = a.Cin = K; a.direct = 1; a.ksize = 1; a.stride = 1; a.Ktaps = a.K = K;
      a.w = f.W<float>(w); a.ldw = K; a.M = Bt; a.N = N; a.bias = f.W<float>(b); a.rows_per_group = 1; a.out = y; a.ldo = N;
      ex.rc = dmx_gemm_f32_launch(a, ex.stream);
    };
    if (!ex.dry && !ex.rc) ex.rc = dmx_timestep_embedding_launch(c.timesteps, t_count, (const float*)(u->arena + u->freq), Bt, boc[0], sinus, ex.stream);
    small(sinus, boc[0], u->te_w1, u->te_b1, temb, e1);
    if (!ex.dry && !ex.rc) ex.rc = dmx_silu_f32_launch(e1, (size_t)Bt * temb, ex.stream);
    small(e1, temb, u->te_w2, u->te_b2, temb, emb);
    if (!ex.dry && !ex.rc) ex.rc = dmx_silu_f32_launch(emb, (size_t)Bt * temb, ex.stream);
    // the 22 time_emb_proj biases are separate fp32 entries: in the master arena entry k sits at byte 2*dst_k, so (unlike the
    // stacked bf16 weight rows) they are not one contiguous vector there - gather them into one
    float* tpb = (float*)ex.raw((size_t)u->tproj_total * 4);
    if (!ex.dry && !ex.rc) {
      for_each_resnet(u, [&](const ResW& r) {
        if (r.temb_off >= 0 &&
            hipMemcpyAsync(tpb + r.temb_off, f.W<float>(u->tp_b + (size_t)r.temb_off * 4), (size_t)r.cout * 4, hipMemcpyDeviceToDevice, ex.stream) != hipSuccess) {
          dmx_set_error("unet_forward_f32: bias gather failed"); ex.rc = DMX_ERR_HIP;
        }
        return ex.rc;
      });
    }
    if (!ex.dry && !ex.rc) {
      GemmF32Args a{}; a.x0 = a.x1 = emb; a.ldx0 = a.ldx1 = temb; a.cx0 = a.Cin = temb; a.direct = 1; a.ksize = 1; a.stride = 1; a.Ktaps = a.K = temb;
      a.w = f.W<float>(u->tp_w); a.ldw = temb; a.M = Bt; a.N = u->tproj_total; a.bias = tpb; a.rows_per_group = 1; a.out = tproj; a.ldo = u->tproj_total;
      ex.rc = dmx_gemm_f32_launch(a, ex.stream);
    }
    ex.drop(tpb);
    te.drop(ex);
    Tn x9 = ex.make(B, H, W, cfg.in_channels);
    if (!ex.dry && !ex.rc) ex.rc = dmx_concat_nchw_to_nhwc_f32_launch(c.f0, c.c0, c.f1, c.c1, c.f2, c.c2, (float*)x9.p, B, H * W, ex.stream);
    ConvOpts oi; oi.bias = f.W<float>(u->ci_b); oi.ldw = u->ci_kpad;
    h = ex.conv(x9, nullptr, f.W<bf16>(u->ci_w), boc[0], oi);
    ex.drop(x9);
  } else {
    if (!ex.dry && !ex.rc) {
      // a table of the loop's timesteps (dmx_unet_temb_table): the per-row form serves per-image timesteps (in-flight batching: every image
      // on its own step, timesteps[b] from the plan), the scalar form a scalar timestep; any other call computes its rows
      const dmx_unet::TembSource& ts = u->temb;
      if (ts.table && t_count == (ts.plan ? B : 1)) {
        hipLaunchKernelGGL(dmx_temb_fetch_kernel, dim3(cdiv(u->tproj_total, 1024), ts.plan ? B : 1), dim3(256), 0, ex.stream, ts.table, ts.index,
                           ts.plan, tproj, const_cast<long long*>(c.timesteps), u->tproj_total);
        ex.rc = dmx_check_launch("dmx_temb_fetch_kernel");
      } else {
        temb_rows(u, ex, c.timesteps, t_count, Bt, te, tproj);
      }
    }
    te.drop(ex);
    // ---- conv_in: cat + layout + im2col, then GEMM
    Tn col = ex.make(B, H, W, u->ci_kpad);
    if (!ex.dry && !ex.rc) {
      Im2colArgs a{}; a.f0 = c.f0; a.c0 = c.c0; a.f1 = c.f1; a.c1 = c.c1; a.f2 = c.f2; a.c2 = c.c2; a.C = cfg.in_channels;
      a.B = B; a.IH = a.OH = H; a.IW = a.OW = W; a.ksize = 3; a.stride = 1; a.pad = 1; a.out = col.p; a.Kpad = u->ci_kpad;
      ex.rc = dmx_im2col_small_launch(a, ex.stream);
    }
    h = ex.linear(col, u->at<bf16>(u->ci_w), boc[0], u->at<float>(u->ci_b), nullptr, false, nullptr, nullptr, true);
    ex.drop(col);
  }
  ex.tap(h);                                           // "conv_in"
  ex.ensure_stats(h);
  std::vector<Tn> skips; skips.push_back(h);
  // The input of a transformer block whose folded last GEMM (dmx_set_ff_fold) left its split-K reduce pass to the GroupNorm that reads the block's
  // output next: it is the residual that pass adds, so it lives until the op after the block has run (like mid_in below).  Dropping it then is
  // right whatever that op was: one that is no GroupNorm has completed the output itself (Exec::flush), and Exec::drop completes it otherwise.
  Tn held;
  auto xf = [&](const XfW& w, Tn& y) {
    Tn z = f.xformer(w, y);
    if (z.pend >= 0) held = y; else ex.drop(y);
    y = z;
  };
  auto drop_held = [&]() { if (held.p) { ex.drop(held); held = Tn(); } };
  for (int i = 0; i < (shallow ? 1 : 4); ++i) {
    for (int j = 0; j < L; ++j) {
#ifdef DMX_PROBES
      static const bool fine = getenv("DMX_TAPS_FINE") != nullptr;      // debugging aid: also tap every resnet / transformer output of the down path
#else
      constexpr bool fine = false;
#endif
      Tn y = f.resnet(u->down_res[i][j], h, nullptr);
      drop_held();
      if (fine) ex.tap(y);
      if (cfg.down_has_attn[i]) { xf(u->down_xf[i][j], y); if (fine) ex.tap(y); }
      ex.ensure_stats(y);                             // (two GroupNorms read it: the next block's and the up path's concat)
      h = y; skips.push_back(h);                      // previous h stays alive as a skip
    }
    if (i < 3 && !shallow) {
      ConvOpts o; o.stride = 2; o.pad = 1; o.bias = f.W<float>(u->down_ds[i].b); o.stats = 1;
      h = ex.conv(h, nullptr, f.W<bf16>(u->down_ds[i].w), boc[i], o);
      drop_held();
      ex.ensure_stats(h);
      skips.push_back(h);
    }
    ex.tap(h);                                         // "down{i}"
  }
  if (shallow) drop_held();                              // (a shallow walk leaves the down path here)
  Tn mid_in;
  if (!shallow) {
    Tn z = f.resnet(u->mid_res[0], h, nullptr);          // h is also skips.back(): keep it
    drop_held();
    xf(u->mid_xf, z);
    ex.ensure_stats(z);
    h = f.resnet(u->mid_res[1], z, nullptr); mid_in = z;
    drop_held();
    ex.tap(h);                                         // "mid"
  } else {
    // the kept tensor in h's place: memory of the caller, not of the workspace (never dropped), complete (no pending reduce pass)
    h = Tn(); h.p = sc_t; h.B = B; h.H = H; h.W = W; h.C = boc[1]; h.ld = boc[1];
    h.cst = sc.has_stats ? (ex.dry ? (const long long*)8 : sc_st) : nullptr;      // (dry walk: no addresses - any non-null value asks the same question)
  }
  for (int i = shallow ? 3 : 0; i < 4; ++i) {
    for (int j = 0; j < L + 1; ++j) {
      Tn s = skips.back(); skips.pop_back();
      Tn y = f.resnet(u->up_res[i][j], h, &s);
      drop_held();
      // (z is the residual of mid_res[1]'s conv2: where that conv left its split-K reduce to the GroupNorm that has just run, z had to live until here)
      if (i == 0 && j == 0) ex.drop(mid_in);
      if (!(shallow && j == 0)) ex.drop(h);
      ex.drop(s);
      if (cfg.up_has_attn[i]) xf(u->up_xf[i][j], y);
      ex.ensure_stats(y);
      h = y;
    }
    if (i < 3) {
      // nearest x2 + conv3x3 as four 2x2 phase convolutions on the source grid (pre-summed taps): 4/9 of the multiply-adds
      const bool direct = ex.f32;                                          // (the phase weights are derived data of the bf16 path)
      ConvOpts o; o.ups = 1; o.ups2 = direct ? 0 : 1; o.bias = f.W<float>(u->up_us[i].b); o.stats = 1;
      Tn y = ex.conv(h, nullptr, direct ? f.W<bf16>(u->up_us[i].w) : u->at<bf16>(u->up_us[i].wp), boc[3 - i], o);
      drop_held();
      ex.ensure_stats(y);
      ex.drop(h); h = y;
      if (i == 2 && sc.mode == DMX_STEP_CACHE_FILL) {
        ex.flush(h);
        sc.has_stats = h.cst != nullptr;
        if (!ex.dry && !ex.rc) {
          const size_t nt = step_cache_tensor_bytes(u, B, H, W) / 16, ns = sc.has_stats ? step_cache_stat_bytes(u, B) / 16 : 0;
          ProfScope ps(PROF_OTHER, ex.stream, 0.0, 32.0 * (double)(nt + ns), "step cache store");
          const size_t blocks = (nt + ns + 255) / 256;
          hipLaunchKernelGGL(dmx_step_cache_store_kernel, dim3((unsigned)(blocks < 2048 ? blocks : 2048)), dim3(256), 0, ex.stream,
                             (const u32x4*)h.p, (u32x4*)sc_t, nt, (const u32x4*)h.cst, (u32x4*)sc_st, ns);
          ex.rc = dmx_check_launch("dmx_step_cache_store_kernel");
        }
      }
    }
    ex.tap(h);                                         // "up{i}"
  }
  Tn t = ex.groupnorm(h, nullptr, f.W<float>(u->cno_g), f.W<float>(u->cno_b), cfg.norm_num_groups, 1e-5f, true);
  drop_held();
  ex.drop(h);
  float* eps_nhwc = (float*)ex.raw((size_t)B * H * W * cfg.out_channels * 4);
  ConvOpts oo; oo.bias = f.W<float>(u->co_b); oo.out_f32 = 1;
  ex.conv(t, nullptr, f.W<bf16>(u->co_w), cfg.out_channels, oo, eps_nhwc);
  ex.drop(t);
  if (!ex.dry && !ex.rc) ex.rc = dmx_nhwc_to_nchw_f32_launch(eps_nhwc, cfg.out_channels, c.out, B, cfg.out_channels, H * W, ex.stream);
  ex.drop(eps_nhwc); ex.drop(tproj);
  return ex.rc;
}

// the product walk with the weight prefetch plan (Exec::note / peek): a dry walk of the same graph lists the weight ranges in launch
// order, the real walk hands every launch the ranges of the launches that follow it
int unet_run_planned(dmx_unet* u, Exec& ex, const UNetCall& c, StepCache& sc) {
  Exec::PfPlan plan;
  {
    Exec dr = Exec::dry_run(); dr.plan = &plan; dr.plan_rec = true;
    UNetCall d = c; d.f0 = d.f1 = d.f2 = nullptr; d.timesteps = nullptr; d.out = nullptr;
    StepCache dsc = sc; dsc.buf = nullptr;
    unet_run(u, dr, d, dsc);
  }
  ex.plan = &plan; ex.plan_rec = false; ex.plan_bad = false; ex.plan_i = 0;
  int rc = unet_run(u, ex, c, sc);
  if (!rc && (ex.plan_bad || ex.plan_i != (int)plan.w.size())) { dmx_set_error("unet: the prefetch plan of the dry walk (%d launches) does not match the real walk (%d)", (int)plan.w.size(), ex.plan_i); rc = DMX_ERR_ARG; }
  ex.plan = nullptr;
  return rc;
}

// the call record of a workspace query: shapes only
UNetCall dry_call(int t_count, int ctx_len, int B, int H, int W) {
  UNetCall c; c.t_count = t_count; c.ctx_len = ctx_len; c.B = B; c.H = H; c.W = W;
  return c;
}
// the call record of the C ABI's argument list (the one place that list is spelled out)
#define UNET_CALL_PARAMS const float* f0, int c0, const float* f1, int c1, const float* f2, int c2, const int64_t* timesteps, int t_count, \
                         const void* ctx, int ctx_len, float* out, int B, int H, int W
#define UNET_CALL_RECORD UNetCall{f0, f1, f2, c0, c1, c2, (const long long*)timesteps, t_count, ctx, ctx_len, out, B, H, W}

int forward_eager(dmx_unet* u, const UNetCall& c, StepCache sc, void* workspace, size_t workspace_bytes, hipStream_t stream) {
  if (const int rc = fold_ready(u, stream)) return rc;
  Exec ex = Exec::on(stream, workspace, workspace_bytes);
  return unet_run_planned(u, ex, c, sc);
}

// whether the tensor a FILL walk of this shape keeps carries statistics records: asked of a dry FILL walk once per shape and plan epoch
bool step_cache_has_stats(dmx_unet* u, const UNetCall& c) {
  const auto key = std::make_tuple(c.B, c.H, c.W, dmx_plan_epoch());
  auto it = u->step_cache_stats.find(key);
  if (it != u->step_cache_stats.end()) return it->second;
  Exec ex = Exec::dry_run();
  StepCache sc; sc.mode = DMX_STEP_CACHE_FILL;
  unet_run(u, ex, dry_call(c.t_count, c.ctx_len, c.B, c.H, c.W), sc);
  if (u->step_cache_stats.size() > 256) u->step_cache_stats.clear();
  return u->step_cache_stats[key] = sc.has_stats;
}

// the step-cache record of a cached forward, checked (house style: DMX_REQUIRE)
int step_cache_record(dmx_unet* u, const UNetCall& c, void* cache, size_t cache_bytes, int mode, const char* who, StepCache* sc) {
  DMX_REQUIRE(mode == DMX_STEP_CACHE_FILL || mode == DMX_STEP_CACHE_USE, "%s: unknown step cache mode %d", who, mode);
  DMX_REQUIRE(cache != nullptr, "%s: null step cache", who);
  DMX_REQUIRE(((size_t)cache & 15) == 0, "%s: the step cache must be 16-byte aligned", who);
  DMX_REQUIRE(cache_bytes >= dmx_unet_step_cache_bytes(u, c.B, c.H, c.W), "%s: step cache too small (%zu bytes, needs %zu)", who, cache_bytes,
              dmx_unet_step_cache_bytes(u, c.B, c.H, c.W));
  sc->mode = mode; sc->buf = cache;
  sc->has_stats = mode == DMX_STEP_CACHE_USE && step_cache_has_stats(u, c);
  return DMX_OK;
}

}  // namespace

// peak of a dry walk under BOTH settings of dmx_set_ff_fold (a first-fit peak is not monotone in the op list: either may be the larger), so that
// a workspace sized once serves the walk whichever way the switch stands and is never smaller than what the two-launch walk asked for
static size_t walk_peak(dmx_unet* u, const UNetCall& c, const StepCache& sc) {
  size_t need = 0;
  for (int k = 0; k < 2; ++k) {
    Exec ex = Exec::dry_run();
    if (k) ex.ff_fold = !ex.ff_fold;
    StepCache s = sc;
    unet_run(u, ex, c, s);
    if (ex.ws.peak() > need) need = ex.ws.peak();
  }
  return need;
}

extern "C" size_t dmx_unet_workspace_bytes(dmx_unet* u, int B, int H, int W, int ctx_len) {
  if (!u) return 0;
  size_t need = walk_peak(u, dry_call(1, ctx_len, B, H, W), StepCache());
  // set_context needs the padded context + split-K scratch
  Exec e2 = Exec::dry_run();
  project_context(u, e2, nullptr, 0, 0, B, B, ctx_len, nullptr);
  if (e2.ws.peak() > need) need = e2.ws.peak();
  return need + 4096;
}

extern "C" int dmx_unet_forward(dmx_unet* u, UNET_CALL_PARAMS, void* workspace, size_t workspace_bytes, dmx_stream_t stream) {
  const UNetCall c = UNET_CALL_RECORD;
  if (const int rc = unet_check_call(u, c, workspace, "unet_forward")) return rc;
  return forward_eager(u, c, StepCache(), workspace, workspace_bytes, (hipStream_t)stream);
}

// dmx_unet_forward + debug taps: the block outputs conv_in, down0..3, mid, up0..3 (the oracle's tap points) are copied out as
// NCHW fp32, back to back, into `taps`; shapes (B, C, H, W) land in tap_shapes[i*4..], the count in *n_taps.
extern "C" int dmx_unet_forward_taps(dmx_unet* u, UNET_CALL_PARAMS, void* workspace, size_t workspace_bytes,
                                     float* taps, size_t tap_floats, int* tap_shapes, int* n_taps, dmx_stream_t stream) {
  const UNetCall c = UNET_CALL_RECORD;
  if (const int rc = unet_check_call(u, c, workspace, "unet_forward_taps")) return rc;
  DMX_REQUIRE(taps && tap_shapes && n_taps, "unet_forward_taps: null argument");
  if (const int rc = fold_ready(u, (hipStream_t)stream)) return rc;
  TapSink sink; sink.buf = taps; sink.cap = tap_floats;
  Exec ex = Exec::on((hipStream_t)stream, workspace, workspace_bytes); ex.taps = &sink;
  StepCache off;
  const int rc = unet_run(u, ex, c, off);
  write_taps(sink, tap_shapes, n_taps);
  return rc;
}

// fp32 VALIDATION forward (tests): the same graph walker on fp32 activations, the fp32 master copy of the parameters
// (`masters`: dmx_unet_grad_bytes(u) bytes filled by dmx_unet_master_import for every parameter) and the plain fp32 kernels of
// ref_f32.hip.  `ctx` is the raw glyph context [B][ctx_len][cross_attention_dim] fp32 (its K / V are projected in the call).
// taps / tap_shapes / n_taps may be NULL.  Never used by the product path.
extern "C" size_t dmx_unet_workspace_bytes_f32(dmx_unet* u, int B, int H, int W, int ctx_len) {
  if (!u) return 0;
  Exec ex = Exec::dry_run(true);
  StepCache off;
  unet_run(u, ex, dry_call(B, ctx_len, B, H, W), off);
  return ex.ws.peak() + 4096;
}
extern "C" int dmx_unet_forward_f32(dmx_unet* u, const void* masters, const float* f0, int c0, const float* f1, int c1, const float* f2, int c2,
                                    const int64_t* timesteps, int t_count, const float* ctx, int ctx_len, float* out, int B, int H, int W,
                                    void* workspace, size_t workspace_bytes, float* taps, size_t tap_floats, int* tap_shapes, int* n_taps, dmx_stream_t stream) {
  const UNetCall c = UNET_CALL_RECORD;
  if (const int rc = unet_check_call(u, c, workspace, "unet_forward_f32")) return rc;
  DMX_REQUIRE(masters != nullptr, "unet_forward_f32: no master arena");
  TapSink sink; sink.buf = taps; sink.cap = tap_floats;
  Exec ex = Exec::on((hipStream_t)stream, workspace, workspace_bytes, true); ex.masters = (const char*)masters;
  if (taps) ex.taps = &sink;
  StepCache off;
  const int rc = unet_run(u, ex, c, off);
  write_taps(sink, tap_shapes, n_taps);
  return rc;
}

// Same contract as dmx_unet_forward, but the launch sequence (~600 kernels) is captured into a hipGraph the second
// time an identical call is seen and replayed afterwards (one hipGraphLaunch per UNet step).  Needs a
// non-default stream (the legacy NULL stream cannot be captured); falls back to eager launches otherwise or while
// the profiler is recording.
bool dmx_profile_active();
static int forward_graph(dmx_unet* u, const UNetCall& c, StepCache sc, void* workspace, size_t workspace_bytes, hipStream_t s) {
  if (s == nullptr || dmx_profile_active()) return forward_eager(u, c, sc, workspace, workspace_bytes, s);
  if (const int rc = fold_ready(u, s)) return rc;      // (in front of a replay as well as of the capture below: never inside it)
  const dmx_unet::GraphKey key = u->graph_key(c, workspace, sc);
  dmx_unet::GraphEntry& e = u->graphs[key];
  if (e.exec) { DMX_HIP(hipGraphLaunch(e.exec, s)); return dmx_poll_device_error(); }      // (what an earlier replay raised: common.h)
  if (e.seen++ == 0)        // first sight: eager (also runs every one-time hipFuncSetAttribute outside a capture)
    return forward_eager(u, c, sc, workspace, workspace_bytes, s);
  if (u->graphs.size() > 64) { u->graphs.erase(key); u->drop_graphs(); }
  DMX_HIP(hipStreamBeginCapture(s, hipStreamCaptureModeThreadLocal));
  Exec ex = Exec::on(s, workspace, workspace_bytes);
  const int rc = unet_run_planned(u, ex, c, sc);
  hipGraph_t g = nullptr;
  const hipError_t ce = hipStreamEndCapture(s, &g);
  if (rc) { if (g) (void)hipGraphDestroy(g); return rc; }
  if (ce != hipSuccess || !g) { dmx_set_error("hipStreamEndCapture failed: %s", hipGetErrorString(ce)); return DMX_ERR_HIP; }
  hipGraphExec_t exec = nullptr;
  const hipError_t ie = hipGraphInstantiate(&exec, g, nullptr, nullptr, 0);
  (void)hipGraphDestroy(g);
  if (ie != hipSuccess) { dmx_set_error("hipGraphInstantiate failed: %s", hipGetErrorString(ie)); return DMX_ERR_HIP; }
  u->graphs[key].exec = exec;
  DMX_HIP(hipGraphLaunch(exec, s));
  return DMX_OK;
}
extern "C" int dmx_unet_forward_graph(dmx_unet* u, UNET_CALL_PARAMS, void* workspace, size_t workspace_bytes, dmx_stream_t stream) {
  const UNetCall c = UNET_CALL_RECORD;
  if (const int rc = unet_check_call(u, c, workspace, "unet_forward_graph")) return rc;
  return forward_graph(u, c, StepCache(), workspace, workspace_bytes, (hipStream_t)stream);
}

// ----------------------------------------------------------------------------- step cache (DeepCache-style reuse of the deep features)
// dmx_unet_forward / _graph with a step cache: FILL is the same forward (bit-equal `out`) that also leaves the tensor entering the last
// up-block, with its statistics records, in `cache`; USE computes `out` from the cache and the layers around it only.
extern "C" size_t dmx_unet_workspace_bytes_cached(dmx_unet* u, int B, int H, int W, int ctx_len) {
  if (!u) return 0;
  size_t need = dmx_unet_workspace_bytes(u, B, H, W, ctx_len);      // (the FILL walk allocates what the plain walk allocates)
  // a first-fit peak is not monotone in the op list: the shallow walk is asked on its own
  const UNetCall c = dry_call(1, ctx_len, B, H, W);
  StepCache sc; sc.mode = DMX_STEP_CACHE_USE; sc.has_stats = step_cache_has_stats(u, c);
  const size_t shallow = walk_peak(u, c, sc);
  if (shallow + 4096 > need) need = shallow + 4096;
  return need;
}
extern "C" int dmx_unet_forward_cached(dmx_unet* u, UNET_CALL_PARAMS, void* cache, size_t cache_bytes, int mode,
                                       void* workspace, size_t workspace_bytes, dmx_stream_t stream) {
  const UNetCall c = UNET_CALL_RECORD;
  if (const int rc = unet_check_call(u, c, workspace, "unet_forward_cached")) return rc;
  StepCache sc;
  if (const int rc = step_cache_record(u, c, cache, cache_bytes, mode, "unet_forward_cached", &sc)) return rc;
  return forward_eager(u, c, sc, workspace, workspace_bytes, (hipStream_t)stream);
}
extern "C" int dmx_unet_forward_cached_graph(dmx_unet* u, UNET_CALL_PARAMS, void* cache, size_t cache_bytes, int mode,
                                             void* workspace, size_t workspace_bytes, dmx_stream_t stream) {
  const UNetCall c = UNET_CALL_RECORD;
  if (const int rc = unet_check_call(u, c, workspace, "unet_forward_cached_graph")) return rc;
  StepCache sc;
  if (const int rc = step_cache_record(u, c, cache, cache_bytes, mode, "unet_forward_cached_graph", &sc)) return rc;
  return forward_graph(u, c, sc, workspace, workspace_bytes, (hipStream_t)stream);
}
