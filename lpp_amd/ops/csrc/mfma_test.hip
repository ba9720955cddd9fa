// MFMA fragment-layout validation for gfx950, and single-purpose test kernels
// for the attention kernels' shared tile helpers (attn_tile.h).
//
// v_mfma_f32_16x16x32_bf16 layouts (verified on hardware by
// tests/test_gpu_attention.py::test_mfma_layout against torch.matmul with
// ASYMMETRIC operands):
//   A[16m][32k]: lane l holds m = l&15, k = (l>>4)*8 + j, j=0..7  (bf16x8)
//   B[32k][16n]: lane l holds n = l&15, k = (l>>4)*8 + j
//   C[16m][16n]: lane l holds n = l&15, m = (l>>4)*4 + r, r=0..3  (f32x4)
// These are the layouts the attention kernels build their fragments for.
#include "attn_tile.h"

namespace lpp {

__global__ void mfma_16x16x32_kernel(const __hip_bfloat16* __restrict__ A,
                                     const __hip_bfloat16* __restrict__ B,
                                     float* __restrict__ C) {
  const int l = threadIdx.x;
  bf16x8 a, b;
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const int m = l & 15, ka = (l >> 4) * 8 + j;
    a[j] = *reinterpret_cast<const short*>(&A[m * 32 + ka]);
    const int n = l & 15, kb = (l >> 4) * 8 + j;
    b[j] = *reinterpret_cast<const short*>(&B[kb * 16 + n]);
  }
  f32x4 c = {0.f, 0.f, 0.f, 0.f};
  c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0);
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int n = l & 15, m = (l >> 4) * 4 + r;
    C[m * 16 + n] = c[r];
  }
}

// v_mfma_f32_32x32x16_bf16 layout (forward and dQ;
// tests/test_gpu_attention.py::test_mfma_32x32x16_layout):
//   A[32m][16k]: lane l holds m = l&31, k = (l>>5)*8 + j   (bf16x8)
//   B[16k][32n]: lane l holds n = l&31, k = (l>>5)*8 + j
//   C[32m][32n]: lane l holds n = l&31, m = crow32(r, l>>5) =
//                (r&3) + 8*(r>>2) + 4*(l>>5), r = 0..15 (f32x16)
__global__ void mfma_32x32x16_kernel(const __hip_bfloat16* __restrict__ A,
                                     const __hip_bfloat16* __restrict__ B,
                                     float* __restrict__ C) {
  const int l = threadIdx.x;
  bf16x8 a, b;
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const int m = l & 31, k = (l >> 5) * 8 + j;
    a[j] = *reinterpret_cast<const short*>(&A[m * 16 + k]);
    const int n = l & 31;
    b[j] = *reinterpret_cast<const short*>(&B[k * 32 + n]);
  }
  f32x16 c;
#pragma unroll
  for (int r = 0; r < 16; ++r) c[r] = 0.f;
  c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, c, 0, 0, 0);
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int n = l & 31, m = crow32(r, l >> 5);
    C[m * 32 + n] = c[r];
  }
}

// ---- attn_tile.h helpers (tests/test_gpu_attention_tile.py) -------------------
// One 512-thread workgroup stages a [64][128] tile into a normal and a
// transposed image with the kernels' row assignment, then reads both back
// element by element through the swizzle functions.
__global__ __launch_bounds__(512) void attn_tile_roundtrip_kernel(
    const short* __restrict__ in, short* __restrict__ out_n, short* __restrict__ out_t) {
  __shared__ __attribute__((aligned(16))) char smem[2 * ATTN_IMG_BYTES];
  char* img_n = smem;
  char* img_t = smem + ATTN_IMG_BYTES;
  const int tid = threadIdx.x, wid = tid >> 6, lane = tid & 63;
  const int st_r = lane >> 4, st_c = 8 * (lane & 15);
#pragma unroll
  for (int pass = 0; pass < 2; ++pass) {
    const int r = stage_row(wid, pass, st_r);
    const bf16x8 v = *reinterpret_cast<const bf16x8*>(&in[r * ATTN_D + st_c]);
    stage_normal(img_n, r, st_c, v);
    stage_transposed(img_t, r, st_c, st_r, v);
  }
  __syncthreads();
  for (int i = tid; i < ATTN_TILE_ROWS * ATTN_D; i += 512) {
    out_n[i] = *reinterpret_cast<const short*>(img_n + rswz(i / ATTN_D, i % ATTN_D));
    out_t[i] = *reinterpret_cast<const short*>(
        img_t + tswz(i / ATTN_TILE_ROWS, i % ATTN_TILE_ROWS));
  }
}

// One wave: X[32][32] fp32 read in the 32x32 C layout -> pack_pair's words,
// out[lane][ksl][4].
__global__ __launch_bounds__(64) void attn_pack_pair_kernel(const float* __restrict__ X,
                                                            int* __restrict__ out) {
  const int l = threadIdx.x;
  float p[16];
#pragma unroll
  for (int r = 0; r < 16; ++r) p[r] = X[crow32(r, l >> 5) * 32 + (l & 31)];
  bf16x8 frag[2];
  pack_pair(p, frag);
#pragma unroll
  for (int ksl = 0; ksl < 2; ++ksl)
#pragma unroll
    for (int w = 0; w < 4; ++w)
      out[(l * 2 + ksl) * 4 + w] = reinterpret_cast<const int*>(&frag[ksl])[w];
}

// One wave: X[32][16] fp32 read as two 16x16 C tiles -> pack_frag16's words,
// out[lane][4].
__global__ __launch_bounds__(64) void attn_pack_frag16_kernel(const float* __restrict__ X,
                                                              int* __restrict__ out) {
  const int l = threadIdx.x, hi4 = l >> 4;
  float p[2][4];
#pragma unroll
  for (int qs = 0; qs < 2; ++qs)
#pragma unroll
    for (int r = 0; r < 4; ++r) p[qs][r] = X[(qs * 16 + hi4 * 4 + r) * 16 + (l & 15)];
  const bf16x8 frag = pack_frag16(p, hi4 & 1);
#pragma unroll
  for (int w = 0; w < 4; ++w) out[l * 4 + w] = reinterpret_cast<const int*>(&frag)[w];
}

}  // namespace lpp

at::Tensor mfma_test_32x32x16(at::Tensor A, at::Tensor B) {
  TORCH_CHECK(A.is_cuda() && A.scalar_type() == at::kBFloat16);
  TORCH_CHECK(A.sizes() == at::IntArrayRef({32, 16}) && B.sizes() == at::IntArrayRef({16, 32}));
  auto C = at::zeros({32, 32}, A.options().dtype(at::kFloat));
  hipLaunchKernelGGL(lpp::mfma_32x32x16_kernel, dim3(1), dim3(64), 0,
                     lpp::current_stream(),
                     (const __hip_bfloat16*)A.contiguous().data_ptr(),
                     (const __hip_bfloat16*)B.contiguous().data_ptr(),
                     C.data_ptr<float>());
  LPP_CHECK_HIP(hipGetLastError());
  return C;
}

at::Tensor mfma_test_16x16x32(at::Tensor A, at::Tensor B) {
  TORCH_CHECK(A.is_cuda() && A.scalar_type() == at::kBFloat16);
  TORCH_CHECK(A.sizes() == at::IntArrayRef({16, 32}) && B.sizes() == at::IntArrayRef({32, 16}));
  auto C = at::zeros({16, 16}, A.options().dtype(at::kFloat));
  hipLaunchKernelGGL(lpp::mfma_16x16x32_kernel, dim3(1), dim3(64), 0,
                     lpp::current_stream(),
                     (const __hip_bfloat16*)A.contiguous().data_ptr(),
                     (const __hip_bfloat16*)B.contiguous().data_ptr(),
                     C.data_ptr<float>());
  LPP_CHECK_HIP(hipGetLastError());
  return C;
}

// [64,128] int16 -> (normal [64,128], transposed [128,64]) read back from LDS.
std::vector<at::Tensor> attn_tile_test_roundtrip(at::Tensor tile) {
  TORCH_CHECK(tile.is_cuda() && tile.scalar_type() == at::kShort && tile.is_contiguous());
  TORCH_CHECK(tile.sizes() == at::IntArrayRef({lpp::ATTN_TILE_ROWS, lpp::ATTN_D}));
  auto out_n = at::zeros_like(tile);
  auto out_t = at::zeros({lpp::ATTN_D, lpp::ATTN_TILE_ROWS}, tile.options());
  hipLaunchKernelGGL(lpp::attn_tile_roundtrip_kernel, dim3(1), dim3(512), 0,
                     lpp::current_stream(), tile.data_ptr<short>(),
                     out_n.data_ptr<short>(), out_t.data_ptr<short>());
  LPP_CHECK_HIP(hipGetLastError());
  return {out_n, out_t};
}

// x fp32 [32,32] -> int32 [64,2,4]: each lane's two pack_pair A-fragments.
at::Tensor attn_tile_test_pack_pair(at::Tensor x) {
  TORCH_CHECK(x.is_cuda() && x.scalar_type() == at::kFloat && x.is_contiguous());
  TORCH_CHECK(x.sizes() == at::IntArrayRef({32, 32}));
  auto out = at::zeros({64, 2, 4}, x.options().dtype(at::kInt));
  hipLaunchKernelGGL(lpp::attn_pack_pair_kernel, dim3(1), dim3(64), 0,
                     lpp::current_stream(), x.data_ptr<float>(), out.data_ptr<int>());
  LPP_CHECK_HIP(hipGetLastError());
  return out;
}

// x fp32 [32,16] -> int32 [64,4]: each lane's pack_frag16 A-fragment.
at::Tensor attn_tile_test_pack_frag16(at::Tensor x) {
  TORCH_CHECK(x.is_cuda() && x.scalar_type() == at::kFloat && x.is_contiguous());
  TORCH_CHECK(x.sizes() == at::IntArrayRef({32, 16}));
  auto out = at::zeros({64, 4}, x.options().dtype(at::kInt));
  hipLaunchKernelGGL(lpp::attn_pack_frag16_kernel, dim3(1), dim3(64), 0,
                     lpp::current_stream(), x.data_ptr<float>(), out.data_ptr<int>());
  LPP_CHECK_HIP(hipGetLastError());
  return out;
}
