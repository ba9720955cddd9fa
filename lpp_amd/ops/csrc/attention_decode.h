// What the two single-token decode kernels share (attention_decode.hip: vector
// ALU, every group size up to 8; attention_decode_mfma.hip: MFMA, groups of 8
// and 16): the launch geometry, the row metadata, the workspace layout of the
// per-chunk partials and the combine kernel that finishes them.
#pragma once

#include "attention.h"
#include "common.h"

namespace lpp {

constexpr int kDecodeChunk = 256;   // C: keys per workgroup (profiles/README.md, Round 6)
constexpr int kDecodeThreads = 256;
constexpr int kDecodeWaves = kDecodeThreads / kWave;
constexpr int kDecodeWs = ATTN_D + 4;  // fp32 partial: acc[128], m, l, pad to 16 B
constexpr float kDecodeMinM = -1e30f;  // running max of an empty state (finite: no inf - inf)
// Which kernel a group of 8 heads gets when the caller does not say (16 has the
// MFMA kernel only).  By group size alone: a row's bits must not depend on N or
// max_len.  Decided by measurement (profiles/README.md, Round 12): MFMA is
// 1.5x to 1.9x faster at all six 64/8 points, spread below 1 us.
constexpr bool kDecodeMfmaDefault8 = true;

__device__ __forceinline__ uint32_t bf16_bits(float x) {
  return (uint32_t)__builtin_bit_cast(unsigned short, __float2bfloat16(x));
}

// Row metadata shared by both kernels.  A row whose cache row or position is
// out of range is skipped (nothing read, nothing written, o = 0).
struct DecodeRow {
  int64_t r;
  int p;
  bool ok;
};
__device__ __forceinline__ DecodeRow decode_row(const int64_t* positions, const int64_t* rows,
                                                int n, int uniform_pos, int slots,
                                                int max_len) {
  const int64_t p = positions ? positions[n] : (int64_t)uniform_pos;
  const int64_t r = rows ? rows[n] : (int64_t)n;
  DecodeRow d;
  d.ok = r >= 0 && r < slots && p >= 0 && p < max_len;
  d.r = r;
  d.p = (int)p;
  return d;
}

// o[n,h,:] = sum_j acc_j 2^(m_j - M) / sum_j l_j 2^(m_j - M) over the row's
// ceil((p+1)/C) chunks, in chunk order.  One chunk takes the same path.
template <int C>
__global__ __launch_bounds__(ATTN_D) void attn_decode_combine_kernel(
    const float* __restrict__ ws, const int64_t* __restrict__ positions,
    const int64_t* __restrict__ rows, __hip_bfloat16* __restrict__ o, int uniform_pos,
    int max_len, int slots, int H, int J) {
  const int h = blockIdx.x, n = blockIdx.y, d = threadIdx.x;
  const DecodeRow row = decode_row(positions, rows, n, uniform_pos, slots, max_len);
  __hip_bfloat16* on = o + ((int64_t)n * H + h) * ATTN_D;
  if (!row.ok) {
    on[d] = __float2bfloat16(0.f);
    return;
  }
  const int nj = row.p / C + 1;                // <= J: p < max_len <= J*C
  const float* w = ws + ((int64_t)n * H + h) * J * kDecodeWs;
  float mx = kDecodeMinM, lv = 0.f, a = 0.f;
  for (int jj = 0; jj < nj; ++jj) {
    const float* wj = w + (int64_t)jj * kDecodeWs;
    const float mj = wj[ATTN_D];
    const float mn = fmaxf(mx, mj);
    const float f0 = exp2f(mx - mn), f1 = exp2f(mj - mn);
    a = a * f0 + wj[d] * f1;
    lv = lv * f0 + wj[ATTN_D + 1] * f1;
    mx = mn;
  }
  on[d] = __float2bfloat16(a / lv);
}

template <int C>
static void launch_decode_combine(const at::Tensor& ws, const int64_t* positions,
                                  const int64_t* rows, at::Tensor& o, int uniform_pos,
                                  int max_len, int slots, int N, int H, int J) {
  hipLaunchKernelGGL((attn_decode_combine_kernel<C>), dim3(H, N), dim3(ATTN_D), 0,
                     current_stream(), ws.data_ptr<float>(), positions, rows,
                     (__hip_bfloat16*)o.data_ptr(), uniform_pos, max_len, slots, H, J);
  LPP_CHECK_HIP(hipGetLastError());
}

// The MFMA kernel's launch (attention_decode_mfma.hip): rep 8 or 16, chunk
// 128 / 256 / 512; the arguments are the ones attention_decode() has checked.
void launch_decode_mfma(int rep, int chunk, const at::Tensor& q, const at::Tensor& k_new,
                        const at::Tensor& v_new, at::Tensor& k_cache, at::Tensor& v_cache,
                        const at::Tensor& cos_t, const at::Tensor& sin_t,
                        const int64_t* positions, const int64_t* rows, int64_t* lengths,
                        at::Tensor& o, int uniform_pos, int max_len);

}  // namespace lpp
