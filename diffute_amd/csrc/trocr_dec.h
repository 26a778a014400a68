// The TrOCR text decoder's model handle: shared by the step path (trocr_dec.hip) and the teacher-forced prefill (trocr_prefill.hip)
#pragma once
#include <vector>
#include "exec.h"
#include "../../include/diffute_hip.h"

// byte offsets of one layer's parameters in the weights arena
struct DecLayer { size_t wqkv, bqkv, wo, bo, l1g, l1b, wcq, bcq, wco, bco, l2g, l2b, w1, b1, w2, b2, l3g, l3b; };

struct dmx_trocr_dec : ModelBase {
  dmx_trocr_dec_config cfg;
  size_t emb, posw, leg = 0, leb = 0, wckv, bckv, lm;
  int npos = 0, kdim = 0, cnt_slice = 0;
  std::vector<DecLayer> layers;
};
