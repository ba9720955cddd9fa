// Shared 64-row x 128-column bf16 tile transpose: registers -> swizzled LDS
// image -> b128 global stores of the transposed tile.
//
// Used by transpose2d_v2_kernel and by the memory-bound backward producers
// (swiglu_bwd, rope_bwd) that hand the wgrad GEMM its transposed operand in
// the same pass that writes the natural gradient.
//
// Thread mapping (256 threads = 4 waves, four passes per tile): in pass p a
// thread holds the eight bf16 at tile row tt_row(p), tile columns
// tt_col() .. tt_col()+7.  The four lanes {l, l^16, l^32, l^48} of a wave hold
// four consecutive rows of the same column pack; a 4x4 dword butterfly
// across that quad turns row-major dwords into column-major ones, which go
// to LDS as b64 writes under a ((d>>3)^d)&7 block swizzle.  After a barrier
// every LDS read is one b128 of eight consecutive rows of one column.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

namespace lpp {

typedef __attribute__((ext_vector_type(8))) short bf16x8_t;
typedef __attribute__((ext_vector_type(2))) int int2v_t;

constexpr int kTTRows = 64;
constexpr int kTTCols = 128;
constexpr int kTTImgBytes = kTTRows * kTTCols * 2;  // 16 KB per image

// Byte offset of element (column d, row r) in the transposed image.
__device__ __forceinline__ int tt_swz(int d, int r) {
  return (d * 64 + (r ^ ((((d >> 3) ^ d) & 7) << 3))) * 2;
}

// Tile row / first tile column this thread holds in pass 0..3.
__device__ __forceinline__ int tt_row(int pass) {
  const int wid = threadIdx.x >> 6, lane = threadIdx.x & 63;
  return 4 * wid + 16 * pass + ((lane >> 4) & 3);
}
__device__ __forceinline__ int tt_col() { return 8 * (threadIdx.x & 15); }

// Stage the eight bf16 of (tt_row(pass), tt_col()..+7) into the image.  All
// 64 lanes of the wave must call it together (cross-lane shuffles).
__device__ __forceinline__ void tt_stage(char* img, bf16x8_t v, int pass) {
  const int wid = threadIdx.x >> 6;
  const int lane = threadIdx.x & 63;
  const int st_r = (lane >> 4) & 3;    // quad row 0..3
  const int st_c = 8 * (lane & 15);    // col pack 0..120
  // 4x4 dword butterfly across the lane quad {l, l^16, l^32, l^48}
  int dw[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) dw[k] = reinterpret_cast<const int*>(&v)[k];
  {
    int t0 = __shfl_xor(dw[(st_r & 1) ^ 1], 16);
    int t1 = __shfl_xor(dw[((st_r & 1) ^ 1) | 2], 16);
    if (st_r & 1) { dw[0] = t0; dw[2] = t1; } else { dw[1] = t0; dw[3] = t1; }
  }
  {
    int lo = (st_r & 2) ? 0 : 2;
    int t0 = __shfl_xor(dw[lo], 32);
    int t1 = __shfl_xor(dw[lo + 1], 32);
    dw[lo] = t0; dw[lo + 1] = t1;
  }
  const int rq = 4 * wid + 16 * pass;  // quad's first row
  const int d0 = st_c + 2 * st_r;
#pragma unroll
  for (int e = 0; e < 2; ++e) {
    const int d = d0 + e;
    unsigned w01 = e ? (((unsigned)dw[0] >> 16) | ((unsigned)dw[1] & 0xffff0000u))
                     : (((unsigned)dw[0] & 0xffffu) | ((unsigned)dw[1] << 16));
    unsigned w23 = e ? (((unsigned)dw[2] >> 16) | ((unsigned)dw[3] & 0xffff0000u))
                     : (((unsigned)dw[2] & 0xffffu) | ((unsigned)dw[3] << 16));
    int2v_t pair = {(int)w01, (int)w23};
    *reinterpret_cast<int2v_t*>(img + tt_swz(d, rq)) = pair;
  }
}

// Write the staged image as the transposed tile: out is [C, R] row-major
// with leading dimension R (elements); the tile's natural origin is (r0, c0).
// Call after a __syncthreads() that follows the last tt_stage.  8 consecutive
// lanes cover packs 0..7 of one out row (a full 128-B line per 8-lane
// group); each b128 LDS read is one swizzled 8-block, banks spread by p^e
// within the group.
__device__ __forceinline__ void tt_store(const char* img, short* __restrict__ out,
                                         int64_t R, int r0, int c0) {
  const int tid = threadIdx.x;
#pragma unroll
  for (int pass = 0; pass < 4; ++pass) {
    const int d = 32 * pass + (tid >> 3);
    const int p = tid & 7;
    const bf16x8_t v = *reinterpret_cast<const bf16x8_t*>(img + tt_swz(d, 8 * p));
    *reinterpret_cast<bf16x8_t*>(out + (int64_t)(c0 + d) * R + r0 + 8 * p) = v;
  }
}

}  // namespace lpp
