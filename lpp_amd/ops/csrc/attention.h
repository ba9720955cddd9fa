// Host interface of the attention kernels: the launches defined next to the
// kernels (attention_fwd.hip, attention_bwd.hip) and what attention_api.cpp
// shares with them.
#pragma once

#include <cmath>

#include "attn_order.h"
#include "attn_tile.h"  // ATTN_D

namespace lpp {

// Softmax scale 1/sqrt(D) and c = scale*log2(e), the factor of the exp2-domain
// scores the kernels work in.
struct AttnScale {
  float scale, c;
};
inline AttnScale attn_scale() {
  const float scale = 1.0f / std::sqrt((float)ATTN_D);
  return {scale, scale * 1.4426950408889634f};
}

// Process-wide order mode (LPP_ATTN_ORDER, default 1; attention_api.cpp).
int attn_order_mode();

// q [B,S,H,128], k/v [B,S,HKV,128], bf16, contiguous, H a multiple of HKV.
void attn_check_qkv(const at::Tensor& q, const at::Tensor& k, const at::Tensor& v,
                    const char* who);
// A document tensor of q's rows: int32, contiguous, [B,S], on q's device.
void attn_check_docs(const at::Tensor& q, const at::Tensor& d, const char* who,
                     const char* name);

// order_G <= 0 (fwd, dQ, dK/dV): heads per group = ATTN_GROUP_WAVES resident
// waves of workgroups per XCD (32 CUs x one workgroup per CU) over nblk; the
// factor is the measured winner of the G sweep, not a residency
// (profiles/README.md, Round 4).
// doc_start / doc_end (packed rows, int32 [B,S], checked by attn_check_docs):
// nullptr launches the plain causal kernel, a tensor the DOCS instantiation.
void launch_attn_fwd(const at::Tensor& q, const at::Tensor& k, const at::Tensor& v,
                     at::Tensor& o, at::Tensor& lse2, int order_mode, int order_G,
                     const at::Tensor* doc_start = nullptr);
void launch_attn_bwd_delta(const at::Tensor& dO, const at::Tensor& o, at::Tensor& delta);
void launch_attn_bwd_dq(const at::Tensor& dO, const at::Tensor& q, const at::Tensor& k,
                        const at::Tensor& v, const at::Tensor& lse2,
                        const at::Tensor& delta, at::Tensor& dq, int order_mode,
                        int order_G, const at::Tensor* doc_start = nullptr);
void launch_attn_bwd_dkdv(const at::Tensor& dO, const at::Tensor& q, const at::Tensor& k,
                          const at::Tensor& v, const at::Tensor& lse2,
                          const at::Tensor& delta, at::Tensor& dk, at::Tensor& dv,
                          int order_mode, int order_G,
                          const at::Tensor* doc_end = nullptr);

}  // namespace lpp
