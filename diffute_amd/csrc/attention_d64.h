// Vector types of the LDS transpose reads (ds_read_b64_tr_b16) that the head-dim-64 attention forward kernels share: attention.hip, attention_sk.hip.
#pragma once

typedef __attribute__((ext_vector_type(4))) short s16x4;
typedef __attribute__((ext_vector_type(8))) short s16x8;
typedef __attribute__((address_space(3))) s16x4* lds_s16x4;
