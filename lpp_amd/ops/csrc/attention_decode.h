// What the two single-token decode kernels share (attention_decode.hip: vector
// ALU, every group size up to 8; attention_decode_mfma.hip: MFMA, groups of 8
// and 16): the launch geometry, the row metadata, the workspace layout of the
// per-chunk partials and the combine kernel that finishes them.
#pragma once

#include "attention.h"
#include "attn_paged.h"
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

// What a launch needs of an optional block table (decode_check_args): the
// device view (table null: slot layout) and how many rows `rows` may name -
// the table's rows, or the cache's slots.
struct DecodeTable {
  PageTable pt;
  int rows;
};

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

// ---- shared by the two MFMA kernels (attention_decode_mfma.hip, _fp8.hip) ----

// max over the lanes l, l^16, l^32, l^48, in every lane.  Swapping a register
// with itself leaves rows (0,0,2,2) and (1,1,3,3), then halves (lo,lo), (hi,hi).
__device__ __forceinline__ float max_across_rows(float x) {
  const int2v a = __builtin_amdgcn_permlane16_swap(as_i(x), as_i(x), false, false);
  x = fmaxf(as_f(a[0]), as_f(a[1]));
  const int2v b = __builtin_amdgcn_permlane32_swap(as_i(x), as_i(x), false, false);
  return fmaxf(as_f(b[0]), as_f(b[1]));
}
__device__ __forceinline__ float sum_across_rows(float x) {
  const int2v a = __builtin_amdgcn_permlane16_swap(as_i(x), as_i(x), false, false);
  x = as_f(a[0]) + as_f(a[1]);
  const int2v b = __builtin_amdgcn_permlane32_swap(as_i(x), as_i(x), false, false);
  return as_f(b[0]) + as_f(b[1]);
}

// Byte offset of 16-byte chunk ch of staged key row r (32 rows of 256 bytes).
__device__ __forceinline__ int vstage_off(int r, int ch) {
  return 256 * r + 16 * (ch ^ ((r & 7) << 1));
}

constexpr int kMfmaStep = 32;                       // keys per wave step
constexpr int kVStageBytes = kMfmaStep * ATTN_D * 2;  // one wave's V staging

template <int REP>
constexpr int decode_mfma_lds() {
  // the 4-wave merge reuses the staging after the loop
  constexpr int st = kDecodeWaves * REP * kDecodeWs * (int)sizeof(float);
  constexpr int vs = kDecodeWaves * kVStageBytes;
  return st > vs ? st : vs;
}

// The MFMA kernel's launch (attention_decode_mfma.hip): rep 8 or 16, chunk
// 128 / 256 / 512; the arguments are the ones attention_decode() has checked.
void launch_decode_mfma(int rep, int chunk, const at::Tensor& q, const at::Tensor& k_new,
                        const at::Tensor& v_new, at::Tensor& k_cache, at::Tensor& v_cache,
                        const at::Tensor& cos_t, const at::Tensor& sin_t,
                        const int64_t* positions, const int64_t* rows, int64_t* lengths,
                        at::Tensor& o, const DecodeTable& bt, int uniform_pos, int max_len);

// The argument checks of attention_decode and attention_decode_fp8
// (attention_decode.hip); with the scales given the caches must be e4m3, with
// block_table they are a paged pool.
DecodeTable decode_check_args(const char* who, const at::Tensor& q, const at::Tensor& k_new,
                       const at::Tensor& v_new, const at::Tensor& k_cache,
                       const at::Tensor& v_cache, const at::Tensor& cos_t,
                       const at::Tensor& sin_t, const c10::optional<at::Tensor>& positions,
                       const c10::optional<at::Tensor>& rows,
                       const c10::optional<at::Tensor>& lengths, int64_t uniform_pos,
                       int64_t max_len, const at::Tensor* k_scale, const at::Tensor* v_scale,
                       const c10::optional<at::Tensor>& block_table);

}  // namespace lpp
