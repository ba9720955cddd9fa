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
// The 512 threads stage rows min(r, nrows - 1), r = 0..63, of `in` into image
// 0 of buffer buf with the kernels' row assignment (the kernels clamp their
// loads the same way, so a tile is always full).
template <int M>
__device__ __forceinline__ void test_stage_tile(char* smem, int buf, const short* in,
                                                int nrows) {
  const int tid = threadIdx.x, wid = tid >> 6, lane = tid & 63;
#pragma unroll
  for (int pass = 0; pass < 2; ++pass) {
    const int r = min(stage_row(wid, pass, lane >> 4), nrows - 1);
    const bf16x8 v = *reinterpret_cast<const bf16x8*>(&in[r * ATTN_D + 8 * (lane & 15)]);
    stage_chunk(attn_img(smem, 0, buf), attn_stage_off<M>(wid, pass, lane), v);
  }
  __syncthreads();
}

// One 512-thread workgroup stages a [64][128] tile into ONE dual-use image,
// then returns the tile through the forward's row reads and its transpose
// through the forward's transposed reads (32x32x16 operand maps).
__global__ __launch_bounds__(512) void attn_tile_roundtrip_kernel(
    const short* __restrict__ in, short* __restrict__ out_n, short* __restrict__ out_t) {
  __shared__ __attribute__((aligned(16))) char smem[2 * ATTN_IMG_BYTES];
  test_stage_tile<32>(smem, 0, in, ATTN_TILE_ROWS);
  const char* img = attn_img(smem, 0, 0);
  const int wid = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
  // A-fragments (t2, dc): tile[t2*32 + lane&31][dc*16 + (lane>>5)*8 + j]
#pragma unroll
  for (int f = 0; f < 2; ++f) {
    const int t2 = wid >> 2, dc = 2 * (wid & 3) + f;
    const bf16x8 a = read_row_frag(img, attn_row_off32(lane, t2, dc));
    *reinterpret_cast<bf16x8*>(
        &out_n[(t2 * 32 + (lane & 31)) * ATTN_D + dc * 16 + (lane >> 5) * 8]) = a;
  }
  // B-fragments (dt, ks): tile[ks*16 + (lane>>5)*8 + j][dt*32 + lane&31]
#pragma unroll
  for (int f = 0; f < 2; ++f) {
    const int dt = wid >> 1, ks = 2 * (wid & 1) + f;
    const bf16x8 b = read_tr_frag(img, attn_tr_off32(lane, dt, ks, 0),
                                  attn_tr_off32(lane, dt, ks, 1));
    *reinterpret_cast<bf16x8*>(
        &out_t[(dt * 32 + (lane & 31)) * ATTN_TILE_ROWS + ks * 16 + (lane >> 5) * 8]) = b;
  }
}

// The B-fragments exactly as the kernels read them, out[frag][lane][8]:
//   M = 32 (forward, dQ): frag = dt*4 + ks,   dt = 0..3, ks = 0..3
//   M = 16 (dK/dV):       frag = dt*2 + half, dt = 0..7, half = 0..1
// staged into LDS buffer buf of a double-buffered image; each of the 8 waves
// reads two of the 16 fragments.
template <int M>
__global__ __launch_bounds__(512) void attn_tr_fragments_kernel(
    const short* __restrict__ in, short* __restrict__ out, int nrows, int buf) {
  __shared__ __attribute__((aligned(16))) char smem[2 * ATTN_IMG_BYTES];
  test_stage_tile<M>(smem, buf, in, nrows);
  const char* img = attn_img(smem, 0, buf);
  const int wid = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
#pragma unroll
  for (int f = 0; f < 2; ++f) {
    const int frag = 2 * wid + f;
    bf16x8 b;
    if (M == 32)
      b = read_tr_frag(img, attn_tr_off32(lane, frag >> 2, frag & 3, 0),
                       attn_tr_off32(lane, frag >> 2, frag & 3, 1));
    else
      b = read_tr_frag(img, attn_tr_off16(lane, frag >> 1, frag & 1, 0),
                       attn_tr_off16(lane, frag >> 1, frag & 1, 1));
    *reinterpret_cast<bf16x8*>(&out[(frag * 64 + lane) * 8]) = b;
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

// tile int16 [64,128] -> int16 [16,64,8]: the 16 B-fragments of MFMA shape
// `shape` (32 | 16) read from LDS buffer `buf` (0 | 1), rows clamped to nrows.
at::Tensor attn_tile_test_tr_fragments(at::Tensor tile, int64_t shape, int64_t nrows,
                                       int64_t buf) {
  TORCH_CHECK(tile.is_cuda() && tile.scalar_type() == at::kShort && tile.is_contiguous());
  TORCH_CHECK(tile.sizes() == at::IntArrayRef({lpp::ATTN_TILE_ROWS, lpp::ATTN_D}));
  TORCH_CHECK(shape == 32 || shape == 16, "attn_tile_test_tr_fragments: shape 32 or 16");
  TORCH_CHECK(nrows >= 1 && nrows <= lpp::ATTN_TILE_ROWS && (buf == 0 || buf == 1));
  auto out = at::zeros({16, 64, 8}, tile.options());
  auto kernel = shape == 32 ? lpp::attn_tr_fragments_kernel<32>
                            : lpp::attn_tr_fragments_kernel<16>;
  hipLaunchKernelGGL(kernel, dim3(1), dim3(512), 0, lpp::current_stream(),
                     tile.data_ptr<short>(), out.data_ptr<short>(), (int)nrows, (int)buf);
  LPP_CHECK_HIP(hipGetLastError());
  return out;
}

// [64,128] int16 -> (the tile [64,128], its transpose [128,64]), both read back
// from one LDS image: by row reads and by transposed reads.
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
