// Model description shared by the inference graphs (vae.hip) and the training graph (vae_train.hip) of the AutoencoderKL.
#pragma once
#include <memory>
#include <vector>
#include "exec.h"

struct AttnW { int C = 0; size_t gg, gb, wq, bq, wk, bk, wv, bv, wo, bo; };
struct CW { size_t w = 0, b = 0; int cin = 0, cout = 0, kpad = 0; size_t wp = 0; /* decoder upsamplers: derived [4][cout][4*cin] phase weights */ };

struct dmx_vae : ModelBase {
  dmx_vae_config cfg;
  // encoder
  CW e_in, e_out, quant; std::vector<ResW> e_res[4]; CW e_ds[4]; ResW e_mid[2]; AttnW e_attn; size_t e_ng, e_nb;
  // decoder
  CW pquant, d_in, d_out; ResW d_mid[2]; AttnW d_attn; std::vector<ResW> d_res[4]; CW d_us[4]; size_t d_ng, d_nb;
  std::shared_ptr<void> train_state;   // live training pass (vae_train.hip)
  int derive(hipStream_t s) override;  // vae.hip: folded shortcut biases, phase weights of the decoder's upsample convs
};

// every ResnetBlock2D of the autoencoder: level by level (e_res[i], d_res[i]), then the mid blocks (e_mid[k], d_mid[k]); stops at the
// first non-zero return of fn(ResW&) and returns it
template <typename F> int for_each_resnet(dmx_vae* v, F&& fn) {
  for (int i = 0; i < 4; ++i) {
    for (auto& r : v->e_res[i]) if (const int rc = fn(r)) return rc;
    for (auto& r : v->d_res[i]) if (const int rc = fn(r)) return rc;
  }
  for (int k = 0; k < 2; ++k) { if (const int rc = fn(v->e_mid[k])) return rc; if (const int rc = fn(v->d_mid[k])) return rc; }
  return 0;
}
