// Device helpers shared by the three attention kernels (attention_fwd.hip,
// attention_bwd.hip) and exercised on their own by the test kernels in
// mfma_test.hip (tests/test_gpu_attention_tile.py,
// tests/test_gpu_attention_tr_image.py): vector types, the dual-use LDS image
// layout with its staging, row-read and transposed-read addresses,
// register-file fragment packs and the double-buffered tile pipeline.
#pragma once

#include "common.h"

namespace lpp {

typedef __attribute__((ext_vector_type(8))) short bf16x8;
typedef __attribute__((ext_vector_type(4))) short bf16x4;
typedef __attribute__((ext_vector_type(16))) float f32x16;
typedef __attribute__((ext_vector_type(4))) float f32x4;
typedef __attribute__((ext_vector_type(2))) int int2v;

constexpr int ATTN_D = 128;        // head dim
constexpr int ATTN_TILE_ROWS = 64; // rows of one staged tile
// One LDS image, [64][128] bf16.
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
// 2^x for the P of the tile loops: one v_exp_f32.  exp2f() under plain -O3
// wraps that instruction in five more (compare, select, add, select, ldexp)
// that rescale arguments below -126 so the result comes out as a subnormal.
// Contract: x = -inf (a masked score) gives exactly 0, as exp2f does; a result
// below 2^-126 is flushed to 0 where exp2f returned a subnormal; every other
// result has the same bits.  Such a P is below 1.2e-38 beside a row sum of at
// least 2^-8 (defer-max threshold) and accumulators many orders larger, so no
// output bit moves unless an accumulator is itself subnormal-sized.
__device__ __forceinline__ float attn_exp2(float x) { return __builtin_amdgcn_exp2f(x); }
__device__ __forceinline__ float as_f(int v) { return __int_as_float(v); }
__device__ __forceinline__ int as_i(float v) { return __float_as_int(v); }

// Row of register r in the 32x32 MFMA C layout, for a lane of half hi2 = lane>>5.
__device__ __forceinline__ int crow32(int r, int hi2) {
  return (r & 3) + 8 * (r >> 2) + 4 * hi2;
}

// ---- LDS image layout ---------------------------------------------------------
// One image [64][128] bf16 with 256-byte rows serves BOTH kinds of fragment
// read: the row reads (ds_read_b128, A operands) and the column reads of the
// B operands, taken with the transposing ds_read_b64_tr_b16, so no tile is kept
// a second time in transposed form.  attn_off<M>(row, ch) is the byte offset of
// 16-byte chunk ch (0..15) of a row; the chunk is XORed with a function of
// row & 15 that depends on the MFMA shape M whose operands are read from it:
//   M = 32 (32x32x16: forward, dQ)  (row&3)<<2 | (row>>2)&3
//   M = 16 (16x16x32: dK/dV)        f(r)=2r, f(4+r)=8+2r, f(8+r)=9+2r,
//                                   f(12+r)=2r+1  (r = 0..3)
// Every access pattern below is free of bank conflicts on its layout
// (tests/test_attention_lds_layout.py runs a bank model over the addresses
// bound as attention_lds_addresses).  All functions are evaluated on the host
// as well, from this header.
#define ATTN_HD __host__ __device__ __forceinline__

ATTN_HD int attn_swz32(int row) { return ((row & 3) << 2) | ((row >> 2) & 3); }
ATTN_HD int attn_swz16(int row) {
  const int a = row & 3, b = (row >> 2) & 3;
  return (a << 1) | (((b ^ (b >> 1)) & 1) << 3) | (b >> 1);
}
template <int M>
ATTN_HD int attn_off(int row, int ch) {
  static_assert(M == 32 || M == 16, "MFMA shape: 32 (32x32x16) or 16 (16x16x32)");
  return 256 * row + 16 * (ch ^ (M == 32 ? attn_swz32(row) : attn_swz16(row)));
}

// ---- staging -----------------------------------------------------------------
// 512 threads stage one [64][128] tile in two passes of one 8-element row-slice
// (one chunk, a ds_write_b128) per thread: wave wid takes rows 4*wid .. 4*wid+3
// (+32 in pass 1), lane l row position l>>4 and chunk l&15.
ATTN_HD int stage_row(int wid, int pass, int p) { return 4 * wid + 32 * pass + p; }
template <int M>
ATTN_HD int attn_stage_off(int wid, int pass, int lane) {
  return attn_off<M>(stage_row(wid, pass, lane >> 4), lane & 15);
}

// ---- fragment addresses --------------------------------------------------------
// Each read's offset is (base ^ column term) + row term: a per-lane base, taken
// from attn_off at the fragment's first position, XORed with a compile-time
// column term (the swizzle is an XOR and the base keeps those bits clear of the
// row part) plus a compile-time row term for the instruction's offset field
// (the swizzles repeat every 16 rows).  A kernel short of registers keeps the
// one base and recomputes the XOR per read (dQ).
//
// Row reads (A operands), one ds_read_b128:
//   32x32x16  A[m = lane&31][k = (lane>>5)*8 + j] = tile[t2*32 + m][dc*16 + k]
//   16x16x32  A[m = lane&15][k = (lane>>4)*8 + j] = tile[rt*16 + m][dc*32 + k]
ATTN_HD int attn_row_base32(int lane) { return attn_off<32>(lane & 31, lane >> 5); }
ATTN_HD int attn_row_at32(int base, int t2, int dc) {
  return (base ^ (32 * dc)) + 32 * 256 * t2;
}
ATTN_HD int attn_row_off32(int lane, int t2, int dc) {
  return attn_row_at32(attn_row_base32(lane), t2, dc);
}
ATTN_HD int attn_row_base16(int lane) { return attn_off<16>(lane & 15, lane >> 4); }
ATTN_HD int attn_row_at16(int base, int rt, int dc) {
  return (base ^ (64 * dc)) + 16 * 256 * rt;
}
ATTN_HD int attn_row_off16(int lane, int rt, int dc) {
  return attn_row_at16(attn_row_base16(lane), rt, dc);
}
// Transposed reads (B operands), two ds_read_b64_tr_b16 (h = 0, 1) of four rows
// each.  In a 16-lane group, lane 4q+p supplies the address of row q, columns
// 4p..4p+3 of a 4-row x 16-column block, and lane i receives column i with row
// q in element q; the two reads fill k = hi*8 + j, j = 4h .. 4h+3:
//   32x32x16  B[k = (lane>>5)*8 + j][n = lane&31] = tile[ks*16 + k][dt*32 + n]
//   16x16x32  B[k = (lane>>4)*8 + j][n = lane&15] = tile[half*32 + k][dt*16 + n]
// Rows 4h+q of an 8-row group differ from rows q in one swizzle bit: chunk bit 0
// (M = 32) or chunk bit 3 (M = 16).
ATTN_HD int attn_tr_base32(int lane) {
  const int q = (lane >> 2) & 3, p = lane & 3;
  return attn_off<32>((lane >> 5) * 8 + q, 2 * ((lane >> 4) & 1) + (p >> 1)) + 8 * (p & 1);
}
ATTN_HD int attn_tr_at32(int base, int dt, int ks, int h) {
  return (base ^ (64 * dt + 16 * h)) + 4 * 256 * h + 16 * 256 * ks;
}
ATTN_HD int attn_tr_off32(int lane, int dt, int ks, int h) {
  return attn_tr_at32(attn_tr_base32(lane), dt, ks, h);
}
ATTN_HD int attn_tr_base16(int lane) {
  const int q = (lane >> 2) & 3, p = lane & 3;
  return attn_off<16>((lane >> 4) * 8 + q, p >> 1) + 8 * (p & 1);
}
ATTN_HD int attn_tr_at16(int base, int dt, int half, int h) {
  return (base ^ (32 * dt) ^ (128 * h)) + 4 * 256 * h + 32 * 256 * half;
}
ATTN_HD int attn_tr_off16(int lane, int dt, int half, int h) {
  return attn_tr_at16(attn_tr_base16(lane), dt, half, h);
}

// ---- LDS accesses --------------------------------------------------------------
// One row-slice (a 16-byte chunk) into an image at a staging offset.
__device__ __forceinline__ void stage_chunk(char* img, int off, const bf16x8& v) {
  *reinterpret_cast<bf16x8*>(img + off) = v;
}
__device__ __forceinline__ bf16x8 read_row_frag(const char* img, int off) {
  return *reinterpret_cast<const bf16x8*>(img + off);
}
// ds_read_b64_tr_b16 needs EXEC all ones: call this under wave-uniform control
// flow only (the wave id is a scalar in every kernel, tiles are always full).
__device__ __forceinline__ bf16x8 read_tr_frag(const char* img, int off0, int off1) {
  typedef __attribute__((address_space(3))) bf16x4 lds_bf16x4;
  const bf16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_bf16x4*)(img + off0));
  const bf16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_bf16x4*)(img + off1));
  return __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
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
