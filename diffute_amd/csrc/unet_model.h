// Model description shared by the inference graph (unet.hip) and the training graph (unet_train.hip): where every
// parameter of the SD2-inpainting UNet lives in the packed weights arena.
#pragma once
#include <map>
#include <memory>
#include <tuple>
#include <vector>
#include "exec.h"

struct XfW {
  int C = 0, heads = 0, ctx_slot = -1;
  size_t ng, nb, wpi, bpi, l1g, l1b, l2g, l2b, l3g, l3b;
  size_t wqkv, wo1, bo1, wq2, wkv2, wo2, bo2, wf1, bf1, wf2, bf2, wpo, bpo;
  // folded LayerNorm: raw (as loaded) copies of the three LN-consuming weights + the derived c1 / c2 vectors
  size_t wqkv_raw, wq2_raw, wf1_raw, c1_qkv, c2_qkv, c1_q2, c2_q2, c1_f1, c2_f1;
  // ff.net.2 and proj_out composed into one linear over [g | h3] (fold.hip): wfpo [C][5C] = [Wpo Wf2 | Wpo], bfpo [C] = bpo + Wpo bf2
  size_t wfpo, bfpo;
};
struct ConvW { size_t w, b; int c; size_t wp = 0; /* upsamplers: derived [4][c][4c] phase weights */ };

// One forward call of the UNet as the C ABI describes it: the three channel groups of the input (NCHW fp32; cat order), the timesteps,
// the cross-attention context (product path: the K / V cache of dmx_unet_set_context; fp32 validation and training: the raw context) and
// the output (NCHW fp32)
struct UNetCall {
  const float *f0 = nullptr, *f1 = nullptr, *f2 = nullptr; int c0 = 0, c1 = 0, c2 = 0;
  const long long* timesteps = nullptr; int t_count = 1;
  const void* ctx = nullptr; int ctx_len = 0;
  float* out = nullptr; int B = 0, H = 0, W = 0;
};

// Step cache of a denoise loop (dmx_unet_forward_cached): the tensor that enters the last up-block - the output of up_us[2]'s phase
// convolution, tap "up2", [B*H*W][block_out_channels[1]] in the compute element type - and its GroupNorm statistics records ([B][C][4]
// DmxStat), in a caller-owned buffer outside the workspace.  FILL: the whole walk, which leaves both there; USE: only the layers
// around them (conv_in, down-block 0, up-block 3, conv_norm_out, conv_out) run, on the kept tensor.
struct StepCache {
  int mode = 0;                     // 0 = off, DMX_STEP_CACHE_FILL, DMX_STEP_CACHE_USE
  void* buf = nullptr;              // null in a dry walk
  // whether the full walk's tensor carries statistics records (a property of the shape and the plan switches): FILL notes it, USE must be
  // told (step_cache_has_stats) - with them the consumers run their apply-only forms, without them they compute their own
  bool has_stats = false;
};

struct dmx_unet : ModelBase {
  dmx_unet_config cfg;
  int temb_dim = 0, tproj_total = 0;
  size_t te_w1, te_b1, te_w2, te_b2, tp_w, tp_b, freq;
  size_t ci_w, ci_b; int ci_kpad = 0;
  size_t co_w, co_b, cno_g, cno_b;
  std::vector<ResW> down_res[4], up_res[4]; std::vector<XfW> down_xf[4], up_xf[4];
  ConvW down_ds[4], up_us[4];
  ResW mid_res[2]; XfW mid_xf;
  std::vector<XfW*> xf_all;          // cross-attention layers in graph order (context cache slots)
  std::vector<TrJob> tr_cache;       // the transpose job table dmx_unet_train_prepare uploaded last (kernels.h TrBatch)
  std::shared_ptr<void> train_state;   // live training pass (unet_train.hip)
  // optional source of the time-embedding projections: rows of a table computed for all timesteps of a loop in one batched pass, instead of
  // four small launches per step.  Scalar form (dmx_unet_use_temb_table; plan == nullptr): row index[0] for every image.  Per-row form
  // (dmx_unet_use_temb_table_rows): row index[b] for image b, timesteps[b] from the plan record.
  struct TembSource { const float* table = nullptr; const int* index = nullptr; const dmx_sched_row_rec* plan = nullptr; } temb;
  // hipGraph cache: one captured UNet step per distinct call (pointers are baked into the nodes).  The key is everything the captured
  // launches depend on: the call record, the workspace, the time-embedding source (its plan pointer tells the two forms apart) and
  // dmx_plan_epoch() (every dmx_set_* switch changes the plans baked into the graph)
  struct GraphKey {
    const void *f0, *f1, *f2, *timesteps, *ctx, *out, *workspace; int c0, c1, c2, t_count, ctx_len, B, H, W;
    const void *temb_table, *temb_index, *temb_plan; int plan_epoch;
    const void* step_cache; int step_mode;      // (a cached loop replays two graphs: its full step and its shallow step)
    auto tie() const { return std::tie(f0, f1, f2, timesteps, ctx, out, workspace, c0, c1, c2, t_count, ctx_len, B, H, W, temb_table, temb_index, temb_plan, plan_epoch, step_cache, step_mode); }
    bool operator<(const GraphKey& o) const { return tie() < o.tie(); }
  };
  GraphKey graph_key(const UNetCall& c, const void* workspace, const StepCache& sc) const {
    return GraphKey{c.f0, c.f1, c.f2, c.timesteps, c.ctx, c.out, workspace, c.c0, c.c1, c.c2, c.t_count, c.ctx_len, c.B, c.H, c.W,
                    temb.table, temb.index, temb.plan, dmx_plan_epoch(), sc.buf, sc.mode};
  }
  // memo of StepCache::has_stats per (B, H, W, plan epoch), from a dry FILL walk (unet.hip step_cache_has_stats)
  std::map<std::tuple<int, int, int, int>, bool> step_cache_stats;
  struct GraphEntry { hipGraphExec_t exec = nullptr; int seen = 0; };
  std::map<GraphKey, GraphEntry> graphs;
  // the composed ff.net.2 / proj_out weights (XfW::wfpo / bfpo) lag the raw weights: derive() and dmx_unet_refresh_derived only set this, the
  // next inference entry composes (unet.hip fold_ready) - a training step launches nothing for them
  bool fold_stale = true;
  void drop_graphs() { for (auto& kv : graphs) if (kv.second.exec) (void)hipGraphExecDestroy(kv.second.exec); graphs.clear(); }
  ~dmx_unet() override { drop_graphs(); }
  void rebound() override { drop_graphs(); }
  int derive(hipStream_t s) override;     // unet.hip: folded biases / LayerNorm-folded weights / phase weights, the zero page; drops the graphs
};

// every ResnetBlock2D of the UNet, level by level (down_res[i], up_res[i]), then the two of the mid block; stops at the first non-zero
// return of fn(ResW&) and returns it.  (NOT the order the parameter table registers time_emb_proj in - down, mid, up: dmx_unet_create
// spells that one out.)
template <typename F> int for_each_resnet(dmx_unet* u, F&& fn) {
  for (int i = 0; i < 4; ++i) {
    for (auto& r : u->down_res[i]) if (const int rc = fn(r)) return rc;
    for (auto& r : u->up_res[i]) if (const int rc = fn(r)) return rc;
  }
  for (auto& r : u->mid_res) if (const int rc = fn(r)) return rc;
  return 0;
}

// the common argument checks of the forward entry points (`who` names the entry point in the error string)
int unet_check_call(const dmx_unet* u, const UNetCall& c, const void* workspace, const char* who);

// The time-embedding MLP and the stacked time_emb_proj of every resnet (product path: fp32 math, bf16 weights), four launches:
// sinusoid of `t_count` timesteps broadcast to `rows` rows, linear_1, linear_2, time_emb_proj -> tproj[rows][tproj_total].  The per-step
// path, the batched table of a denoise loop and the training forward (which keeps the intermediates for its backward) all run this
// one, so a row is the same bits wherever it was computed.  The caller owns the buffers (their place in the allocation order is part
// of the workspace contract).
struct TembBufs {
  float *sinus = nullptr, *e1 = nullptr, *emb = nullptr;
  TembBufs() {}
  TembBufs(const dmx_unet* u, Exec& ex, int rows)
      : sinus((float*)ex.raw((size_t)rows * u->cfg.block_out_channels[0] * 4)), e1((float*)ex.raw((size_t)rows * u->temb_dim * 4)),
        emb((float*)ex.raw((size_t)rows * u->temb_dim * 4)) {}
  void drop(Exec& ex) const { ex.drop(sinus); ex.drop(e1); ex.drop(emb); }
};
int temb_rows(const dmx_unet* u, Exec& ex, const long long* timesteps, int t_count, int rows, const TembBufs& b, float* tproj);

static inline int dmx_ctx_pad(int ctx_len) { return (int)align_up((size_t)ctx_len, 64); }
