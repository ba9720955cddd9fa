// RoPE (rotate_half convention) forward + backward for gfx950.
//
// x: [B, S, H, D] (D contiguous). cos/sin: [Smax, D/2] fp32, precomputed on
// host (guide Appendix B: on-device trig makes this VALU-bound; table loads
// keep it at the HBM roofline). Backward = rotation by -theta (sin negated),
// same kernel.
//
// Thread mapping: one thread handles 4 rotation pairs — 8-byte load from the
// first half (x[d..d+3]) + 8-byte load from the second half (x[d+D/2..]),
// two 8-byte stores. D is a multiple of 8 for every LLaMA geometry (128).
//
// Reference op: SURVEY.md §2.7 "RoPE apply"; position_ids threading at
// models/llama_ds_mp_wrap.py:25,37,148. Oracle: lpp_amd.ops.apply_rope_ref.
#include "common.h"
#include "transpose_tile.h"

namespace lpp {

template <typename T, bool BWD>
__global__ void rope_kernel(const T* __restrict__ x, const float* __restrict__ cos_t,
                            const float* __restrict__ sin_t, T* __restrict__ y,
                            int64_t total_pairs4,  // B*S*H*(D/2/4)
                            int S, int H, int D, int pos_offset) {
  const int half = D / 2;
  const int pair4_per_head = half / 4;
  for (int64_t idx = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; idx < total_pairs4;
       idx += (int64_t)gridDim.x * blockDim.x) {
    const int p4 = idx % pair4_per_head;           // which 4-pair group in the head
    const int64_t bsh = idx / pair4_per_head;      // flattened (b, s, h)
    const int s = (int)((bsh / H) % S);
    const int d0 = p4 * 4;
    const int64_t base = bsh * D + d0;

    using P4 = Pack<T, 4>;
    P4 x1 = *reinterpret_cast<const P4*>(x + base);
    P4 x2 = *reinterpret_cast<const P4*>(x + base + half);
    P4 y1, y2;
    const float* cr = cos_t + (int64_t)(pos_offset + s) * half + d0;
    const float* sr = sin_t + (int64_t)(pos_offset + s) * half + d0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      float c = cr[k];
      float sn = BWD ? -sr[k] : sr[k];
      float a = to_f32(x1.v[k]);
      float b = to_f32(x2.v[k]);
      y1.v[k] = from_f32<T>(a * c - b * sn);
      y2.v[k] = from_f32<T>(b * c + a * sn);
    }
    *reinterpret_cast<P4*>(y + base) = y1;
    *reinterpret_cast<P4*>(y + base + half) = y2;
  }
}

// Backward rotation that also writes dx^T for the wgrad GEMM of q_proj /
// k_proj: x viewed as [T = B*S, H*D] with D = 128, one workgroup per 64-token
// x one-head tile (the pair (d, d + 64) of a head sits inside the tile).  A
// thread holds eight bf16 of one half; the partner half lives in lane ^ 8 of
// the same row.  The rotation is rope_kernel<T, true>'s expressions; the
// natural store is unchanged and the tile also goes out transposed
// (transpose_tile.h).  Requires T % 64 == 0.
__global__ __launch_bounds__(256) void rope_bwd_t_kernel(
    const __hip_bfloat16* __restrict__ x, const float* __restrict__ cos_t,
    const float* __restrict__ sin_t, __hip_bfloat16* __restrict__ y,
    short* __restrict__ yT, int T, int S, int C /* H*128 */, int pos_offset) {
  __shared__ __attribute__((aligned(16))) char img[kTTImgBytes];
  using T_ = __hip_bfloat16;
  using PV = Pack<T_, 8>;
  constexpr int half = 64;

  const int r0 = blockIdx.y * 64;
  const int c0 = blockIdx.x * 128;
  const int col = tt_col();
  const bool first = col < half;
  const int d0 = col & (half - 1);

#pragma unroll
  for (int pass = 0; pass < 4; ++pass) {
    const int row = r0 + tt_row(pass);
    const int s = row % S;
    const int64_t off = (int64_t)row * C + c0 + col;
    PV own = *reinterpret_cast<const PV*>(x + off);
    PV oth;
#pragma unroll
    for (int k = 0; k < 4; ++k)
      reinterpret_cast<int*>(&oth)[k] = __shfl_xor(reinterpret_cast<const int*>(&own)[k], 8);
    const float* cr = cos_t + (int64_t)(pos_offset + s) * half + d0;
    const float* sr = sin_t + (int64_t)(pos_offset + s) * half + d0;
    PV out;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      float c = cr[k];
      float sn = -sr[k];
      float a = to_f32(first ? own.v[k] : oth.v[k]);
      float b = to_f32(first ? oth.v[k] : own.v[k]);
      T_ y1 = from_f32<T_>(a * c - b * sn);
      T_ y2 = from_f32<T_>(b * c + a * sn);
      out.v[k] = first ? y1 : y2;
    }
    *reinterpret_cast<PV*>(y + off) = out;
    tt_stage(img, *reinterpret_cast<const bf16x8_t*>(&out), pass);
  }
  __syncthreads();
  tt_store(img, yT, T, r0, c0);
}

template <bool BWD>
at::Tensor rope_launch(at::Tensor x, at::Tensor cos_t, at::Tensor sin_t, int64_t pos_offset) {
  TORCH_CHECK(x.is_cuda() && x.is_contiguous() && x.dim() == 4, "rope: x must be [B,S,H,D]");
  const int B = x.size(0), S = x.size(1), H = x.size(2), D = x.size(3);
  TORCH_CHECK(D % 8 == 0, "rope: head_dim must be a multiple of 8");
  TORCH_CHECK(cos_t.is_contiguous() && sin_t.is_contiguous());
  TORCH_CHECK(cos_t.size(0) >= pos_offset + S, "rope cache too short");
  auto y = at::empty_like(x);
  const int64_t total = (int64_t)B * S * H * (D / 8);
  auto stream = lpp::current_stream();
  const int grid = lpp::grid_for(total, 256);
  LPP_DISPATCH_FLOAT(x.scalar_type(), "rope", [&] {
    hipLaunchKernelGGL((lpp::rope_kernel<scalar_t, BWD>), dim3(grid), dim3(256), 0, stream,
                       (const scalar_t*)x.data_ptr(), cos_t.data_ptr<float>(),
                       sin_t.data_ptr<float>(), (scalar_t*)y.data_ptr(), total, S, H, D,
                       (int)pos_offset);
  });
  LPP_CHECK_HIP(hipGetLastError());
  return y;
}

}  // namespace lpp

at::Tensor rope_fwd(at::Tensor x, at::Tensor cos_t, at::Tensor sin_t, int64_t pos_offset) {
  return lpp::rope_launch<false>(x, cos_t, sin_t, pos_offset);
}

at::Tensor rope_bwd(at::Tensor dy, at::Tensor cos_t, at::Tensor sin_t, int64_t pos_offset) {
  return lpp::rope_launch<true>(dy, cos_t, sin_t, pos_offset);
}

// rope_bwd that also returns dx^T ([H*D, B*S]) when x is bf16 with D == 128
// and B*S % 64 == 0: {dx, dxT}.  Any other shape runs rope_kernel and
// returns {dx}.
std::vector<at::Tensor> rope_bwd_t(at::Tensor dy, at::Tensor cos_t, at::Tensor sin_t,
                                   int64_t pos_offset) {
  TORCH_CHECK(dy.is_cuda() && dy.is_contiguous() && dy.dim() == 4,
              "rope: x must be [B,S,H,D]");
  const int64_t B = dy.size(0), S = dy.size(1), H = dy.size(2), D = dy.size(3);
  const int64_t T = B * S, C = H * D;
  if (dy.scalar_type() != at::kBFloat16 || D != 128 || T == 0 || T % 64 != 0 ||
      T / 64 > 65535 || T > INT32_MAX || C > INT32_MAX)
    return {lpp::rope_launch<true>(dy, cos_t, sin_t, pos_offset)};
  TORCH_CHECK(cos_t.is_contiguous() && sin_t.is_contiguous());
  TORCH_CHECK(cos_t.scalar_type() == at::kFloat && sin_t.scalar_type() == at::kFloat);
  TORCH_CHECK(cos_t.dim() == 2 && cos_t.size(1) == D / 2 && sin_t.sizes() == cos_t.sizes(),
              "rope: cos/sin must be [Smax, D/2]");
  TORCH_CHECK(pos_offset >= 0 && cos_t.size(0) >= pos_offset + S, "rope cache too short");
  auto dx = at::empty_like(dy);
  auto dxT = at::empty({C, T}, dy.options());
  dim3 grid((unsigned)H, (unsigned)(T / 64));
  hipLaunchKernelGGL(lpp::rope_bwd_t_kernel, grid, dim3(256), 0, lpp::current_stream(),
                     (const __hip_bfloat16*)dy.data_ptr(), cos_t.data_ptr<float>(),
                     sin_t.data_ptr<float>(), (__hip_bfloat16*)dx.data_ptr(),
                     (short*)dxT.data_ptr(), (int)T, (int)S, (int)C, (int)pos_offset);
  LPP_CHECK_HIP(hipGetLastError());
  return {dx, dxT};
}
