// Device helpers shared by the three attention kernels (attention_fwd.hip,
// attention_bwd.hip) and exercised on their own by the test kernels in
// mfma_test.hip (tests/test_gpu_attention_tile.py): vector types, the two LDS
// image layouts, register-file fragment packs, tile staging and the
// double-buffered tile pipeline.
#pragma once

#include "common.h"

namespace lpp {

typedef __attribute__((ext_vector_type(8))) short bf16x8;
typedef __attribute__((ext_vector_type(16))) float f32x16;
typedef __attribute__((ext_vector_type(4))) float f32x4;
typedef __attribute__((ext_vector_type(2))) int int2v;

constexpr int ATTN_D = 128;        // head dim
constexpr int ATTN_TILE_ROWS = 64; // rows of one staged tile
// One LDS image, normal [64][128] or transposed [128][64], bf16.
constexpr int ATTN_IMG_BYTES = ATTN_TILE_ROWS * ATTN_D * 2;

// Image `slot` of a kernel's dynamic LDS; every image is double-buffered, so a
// kernel with n images uses attn_lds_bytes(n) and its extras start there.
__device__ __forceinline__ char* attn_img(char* smem, int slot, int buf) {
  return smem + (2 * slot + buf) * ATTN_IMG_BYTES;
}
constexpr int attn_lds_bytes(int images) { return 2 * images * ATTN_IMG_BYTES; }

// ---- bit conversions ---------------------------------------------------------
__device__ __forceinline__ unsigned cvt_pk_bf16(float lo, float hi) {
  unsigned r;
  asm("v_cvt_pk_bf16_f32 %0, %1, %2" : "=v"(r) : "v"(lo), "v"(hi));
  return r;
}
__device__ __forceinline__ float bf16_to_f32(short s) {
  union { unsigned u; float f; } cv;
  cv.u = ((unsigned)(unsigned short)s) << 16;
  return cv.f;
}
__device__ __forceinline__ short f32_to_bf16(float f) {
  __hip_bfloat16 h = __float2bfloat16(f);
  return *reinterpret_cast<short*>(&h);
}
__device__ __forceinline__ float as_f(int v) { return __int_as_float(v); }
__device__ __forceinline__ int as_i(float v) { return __float_as_int(v); }

// Row of register r in the 32x32 MFMA C layout, for a lane of half hi2 = lane>>5.
__device__ __forceinline__ int crow32(int r, int hi2) {
  return (r & 3) + 8 * (r >> 2) + 4 * hi2;
}

// ---- LDS image layouts -------------------------------------------------------
// Normal image [rows][128] bf16, row stride 256 B, byte offset XORed with
// (row&15)<<4: the 16-lane ds_read_b128 A-fragment groups are conflict-free.
__device__ __forceinline__ int rswz(int row, int col_elem) {
  return row * 256 + ((col_elem * 2) ^ ((row & 15) << 4));
}
// Transposed image [128 d][64 r] bf16; byte offset of element (d, r) =
// (d*64 + (r ^ ((((d>>3) ^ d) & 7) << 3))) * 2.  Writes are ~2-way (the XOR
// varies with the lane's d), B-fragment reads conflict-free (measured 0.9%
// conflict cycles in the forward vs 8-15% for padded strides).
__device__ __forceinline__ int tswz(int d, int r) {
  return (d * 64 + (r ^ ((((d >> 3) ^ d) & 7) << 3))) * 2;
}

// 4x4 dword butterfly across the lane quad {l, l^16, l^32, l^48}, each lane
// holding 8 bf16 of one row at the same column c: the lane with quad position
// p ends holding dword p of each quad row, out[i] = row i at columns c+2p, c+2p+1.
__device__ __forceinline__ void quad_transpose(const bf16x8& v, int p, int out[4]) {
#pragma unroll
  for (int k = 0; k < 4; ++k) out[k] = reinterpret_cast<const int*>(&v)[k];
  {  // bit0 of dword index <-> bit0 of quad pos (xor 16)
    int t0 = __shfl_xor(out[(p & 1) ^ 1], 16);
    int t1 = __shfl_xor(out[((p & 1) ^ 1) | 2], 16);
    if (p & 1) { out[0] = t0; out[2] = t1; } else { out[1] = t0; out[3] = t1; }
  }
  {  // bit1 of dword index <-> bit1 of quad pos (xor 32)
    int lo = (p & 2) ? 0 : 2;
    int t0 = __shfl_xor(out[lo], 32);
    int t1 = __shfl_xor(out[lo + 1], 32);
    out[lo] = t0; out[lo + 1] = t1;
  }
}

// Write the quad-transposed columns into a transposed image as 2x ds_write_b64;
// r0 = quad's first row (multiple of 4), d0 = first column this lane owns.
__device__ __forceinline__ void write_transposed(char* img, int r0, int d0,
                                                 const int dw[4]) {
#pragma unroll
  for (int e = 0; e < 2; ++e) {
    const int d = d0 + e;  // column e: bf16 of rows 0..3 = half e of dw[0..3]
    unsigned w01 = e ? (((unsigned)dw[0] >> 16) | ((unsigned)dw[1] & 0xffff0000u))
                     : (((unsigned)dw[0] & 0xffffu) | ((unsigned)dw[1] << 16));
    unsigned w23 = e ? (((unsigned)dw[2] >> 16) | ((unsigned)dw[3] & 0xffff0000u))
                     : (((unsigned)dw[2] & 0xffffu) | ((unsigned)dw[3] << 16));
    int2v pair = {(int)w01, (int)w23};
    *reinterpret_cast<int2v*>(img + tswz(d, r0)) = pair;
  }
}

// ---- staging -----------------------------------------------------------------
// 512 threads stage one [64][128] tile in two passes of one 8-element row-slice
// per thread: wave wid takes rows 4*wid .. 4*wid+3 (+32 in pass 1), lane l row
// position p = l>>4 and column 8*(l&15), so each lane quad {l, l^16, l^32, l^48}
// holds four consecutive rows at one column for the transpose butterfly.
__device__ __forceinline__ int stage_row(int wid, int pass, int p) {
  return 4 * wid + 32 * pass + p;
}
// One row-slice (row r, columns c..c+7) into a normal image: a b128 write.
__device__ __forceinline__ void stage_normal(char* img, int r, int c, const bf16x8& v) {
  *reinterpret_cast<bf16x8*>(img + rswz(r, c)) = v;
}
// The quad's four row-slices into a transposed image; every lane of the quad
// calls this with its own row r = r0 + p.
__device__ __forceinline__ void stage_transposed(char* img, int r, int c, int p,
                                                 const bf16x8& v) {
  int dw[4];
  quad_transpose(v, p, dw);
  write_transposed(img, r - p, c + 2 * p, dw);
}

// ---- fragment packs (registers only, no LDS) ----------------------------------
// 32x32x16: one 16-reg group in crow32 order, p[r] = C[crow32(r, hi2)][lane&31],
// of this lane and its ^32 partner -> two A-fragments of the transpose,
// out[ksl] = A[m = lane&31][k = ksl*16 + hi2*8 + j].  Each permlane32_swap
// fills two A-fragment words for both lane halves.
__device__ __forceinline__ void pack_pair(const float p[16], bf16x8 out[2]) {
#pragma unroll
  for (int ksl = 0; ksl < 2; ++ksl) {
    const float* pr = &p[8 * ksl];
    const unsigned x1 = cvt_pk_bf16(pr[0], pr[1]);
    const unsigned x2 = cvt_pk_bf16(pr[2], pr[3]);
    const unsigned y1 = cvt_pk_bf16(pr[4], pr[5]);
    const unsigned y2 = cvt_pk_bf16(pr[6], pr[7]);
    const int2v a = __builtin_amdgcn_permlane32_swap((int)x1, (int)y1, false, false);
    const int2v b = __builtin_amdgcn_permlane32_swap((int)x2, (int)y2, false, false);
    int w[4] = {a[0], b[0], a[1], b[1]};
    out[ksl] = *reinterpret_cast<const bf16x8*>(w);
  }
}

// 16x16x32: two 16x16 C tiles, p[qs][r] = C[qs*16 + (lane>>4)*4 + r][lane&15]
// -> the A-fragment of the transpose, A[m = lane&15][k = (lane>>4)*8 + j]:
//   sources: X_qs = cvt_pk(p[qs][0], p[qs][1]), Y_qs = cvt_pk(p[qs][2], p[qs][3])
//   a = permlane32_swap(X0, X1); c  = permlane16_swap(a[0], a[0]);
//   c' = permlane16_swap(a[1], a[1])
//   d0 = (hi4&1) ? c'[0] : a[0];   d2 = (hi4&1) ? a[1] : c[1]
// (and the same for the Y family giving d1, d3).
__device__ __forceinline__ bf16x8 pack_frag16(const float p[2][4], int hi4_odd) {
  unsigned X0 = cvt_pk_bf16(p[0][0], p[0][1]);
  unsigned Y0 = cvt_pk_bf16(p[0][2], p[0][3]);
  unsigned X1 = cvt_pk_bf16(p[1][0], p[1][1]);
  unsigned Y1 = cvt_pk_bf16(p[1][2], p[1][3]);
  const int2v ax = __builtin_amdgcn_permlane32_swap((int)X0, (int)X1, false, false);
  const int2v cx = __builtin_amdgcn_permlane16_swap(ax[0], ax[0], false, false);
  const int2v cpx = __builtin_amdgcn_permlane16_swap(ax[1], ax[1], false, false);
  const int2v ay = __builtin_amdgcn_permlane32_swap((int)Y0, (int)Y1, false, false);
  const int2v cy = __builtin_amdgcn_permlane16_swap(ay[0], ay[0], false, false);
  const int2v cpy = __builtin_amdgcn_permlane16_swap(ay[1], ay[1], false, false);
  int w[4];
  w[0] = hi4_odd ? cpx[0] : ax[0];
  w[1] = hi4_odd ? cpy[0] : ay[0];
  w[2] = hi4_odd ? ax[1] : cx[1];
  w[3] = hi4_odd ? ay[1] : cy[1];
  return *reinterpret_cast<const bf16x8*>(w);
}

// ---- tile pipeline -----------------------------------------------------------
// Runs body(tile0, cur) for tile0 = begin, begin+STEP, .. < end over
// double-buffered LDS images, staging one tile ahead with one barrier per tile:
//   ld(tile0, pass, a, b)          two global row-slices of a tile -> registers
//   write(buf, tile0, pass, a, b)  those registers -> the images of buffer buf
//   body(tile0, cur)               compute on buffer cur
// Write-after-barrier (guide T14): tile t+1, already in registers, is written
// right AFTER the barrier of tile t, so the LDS writes overlap tile t's MFMAs
// instead of serialising behind them, and tile t+2's loads re-issue at once
// into the freed registers, getting the whole compute phase to land (guide G15;
// +7-9% over write-before-barrier on the GEMM A/B, the placement the forward
// previously used).  No barrier separates those writes from tile t's MFMAs:
// they go to the other buffer, which every wave left at the barrier before.
// The barrier sits outside every wave condition of the body.  The forward and
// dK/dV call this; dQ writes the same steps out (see attention_bwd.hip).
template <int STEP, class Ld, class Write, class Body>
__device__ __forceinline__ void attn_tile_pipeline(int begin, int end, Ld ld, Write write,
                                                   Body body) {
  bf16x8 a0, b0, a1, b1;
  ld(begin, 0, a0, b0);
  ld(begin, 1, a1, b1);
  write(0, begin, 0, a0, b0);
  write(0, begin, 1, a1, b1);
  if (begin + STEP < end) {
    ld(begin + STEP, 0, a0, b0);
    ld(begin + STEP, 1, a1, b1);
  }
  __syncthreads();
  for (int t0 = begin, cur = 0; t0 < end; t0 += STEP, cur ^= 1) {
    if (t0 + STEP < end) {
      write(cur ^ 1, t0 + STEP, 0, a0, b0);
      write(cur ^ 1, t0 + STEP, 1, a1, b1);
      if (t0 + 2 * STEP < end) {
        ld(t0 + 2 * STEP, 0, a0, b0);
        ld(t0 + 2 * STEP, 1, a1, b1);
      }
    }
    body(t0, cur);
    __syncthreads();
  }
}

}  // namespace lpp
