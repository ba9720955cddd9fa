// Flash-style causal attention BACKWARD for gfx950 (CDNA4), bf16, D=128.
//
// Completes the implicit-mask attention path (see attention_fwd.hip): the
// reference never had a working flash attention (README.md:141-143) and
// materialises the [B,1,S,S] mask host-side; here the backward recomputes
// P = exp2(c*QK^T - LSE2) tile-by-tile from the forward's base-2 logsumexp,
// so nothing S^2-shaped is ever stored.
//
// Same swapped-operand MFMA structure as the forward (v_mfma_f32_32x32x16):
// the softmax-corrected tensors (P, dS) are always computed with the
// REDUCTION-FREE axis in the lane dimension, so the elementwise
// dS = P*(dP - delta) needs no cross-lane traffic, and the packed A-
// fragments for the accumulating GEMMs come from the same
// v_cvt_pk_bf16_f32 + permlane32_swap construction the forward uses.
//
// Three kernels:
//   1. delta[b,h,s] = rowsum(dO * O)                       (memory-bound)
//   2. dQ kernel — 8 waves x 32 q rows (lane = q): per KV tile of 64,
//        S^T  = mfma(K_lds, Q_reg)   C[kv regs][q lane]
//        dP^T = mfma(V_lds, dO_reg)  same layout
//        P    = exp2(c*S^T - L[own q]);  dS = P*(dP^T - delta[own q])
//        dQ  += mfma(pack(dS), K^T image)          (scale at epilogue)
//   3. dK/dV kernel — 8 waves x 16 kv rows (lane = kv, 16x16x32
//      fragments), 2 waves/SIMD (one workgroup per CU); grid over KV blocks
//      x B*HKV; per
//      double-buffered 64-row q tile (two 32-row compute halves):
//        S    = mfma(Q_lds, K_reg)   C[q regs][kv lane]
//        dP   = mfma(dO_lds, V_reg)  same layout
//        P    = exp2(c*S - L[q])  (L,delta broadcast from a staged tile)
//        dV  += mfma(pack(P),  dO^T image)
//        dK  += mfma(pack(dS), Q^T image)
//      P/dS pack to A-fragments via a cvt_pk + permlane32/16_swap network
//      (pack_frag16) — no LDS roundtrip.
//      GQA: the G query heads sharing a kv head accumulate in-register.
//
// LDS images: "normal" [rows][128] tiles XOR-swizzled ((row&15)<<4) for the
// A-fragment ds_read_b128; "transposed" [128][64] tswz images (the
// forward's XOR layout), filled by the same in-register 4x4 dword
// butterfly as the forward's V image.
#include "common.h"
#include "attn_order.h"

namespace lpp {

typedef __attribute__((ext_vector_type(8))) short bf16x8;
typedef __attribute__((ext_vector_type(16))) float f32x16;
typedef __attribute__((ext_vector_type(2))) int int2v;

constexpr int AB_D = 128;

__device__ __forceinline__ int bswz(int row, int col_elem) {
  return row * 256 + ((col_elem * 2) ^ ((row & 15) << 4));
}
__device__ __forceinline__ unsigned cvt_pk_bf16_(float lo, float hi) {
  unsigned r;
  asm("v_cvt_pk_bf16_f32 %0, %1, %2" : "=v"(r) : "v"(lo), "v"(hi));
  return r;
}
__device__ __forceinline__ float bf2f_(short s) {
  union { unsigned u; float f; } cv;
  cv.u = ((unsigned)(unsigned short)s) << 16;
  return cv.f;
}
__device__ __forceinline__ short f2bf_(float f) {
  __hip_bfloat16 h = __float2bfloat16(f);
  return *reinterpret_cast<short*>(&h);
}

// 4x4 dword butterfly across the lane quad {l, l^16, l^32, l^48}: lane with
// quad position p ends holding dword p of each quad row (see the forward).
// Returns the four dwords (rows 0..3 of the quad at columns c+2p, c+2p+1).
__device__ __forceinline__ void quad_transpose(const bf16x8& v, int st_r, int out[4]) {
#pragma unroll
  for (int k = 0; k < 4; ++k) out[k] = reinterpret_cast<const int*>(&v)[k];
  {
    int t0 = __shfl_xor(out[(st_r & 1) ^ 1], 16);
    int t1 = __shfl_xor(out[((st_r & 1) ^ 1) | 2], 16);
    if (st_r & 1) { out[0] = t0; out[2] = t1; } else { out[1] = t0; out[3] = t1; }
  }
  {
    int lo = (st_r & 2) ? 0 : 2;
    int t0 = __shfl_xor(out[lo], 32);
    int t1 = __shfl_xor(out[lo + 1], 32);
    out[lo] = t0; out[lo + 1] = t1;
  }
}

// Transposed [128][64] image with the forward's XOR layout: byte offset of
// element (d, r) = (d*64 + (r ^ ((((d>>3) ^ d) & 7) << 3))) * 2.  Writes are
// ~2-way (the XOR varies with the lane's d), B-fragment reads conflict-free
// (measured 0.9% conflict cycles in the forward vs 8-15% for padded strides).
__device__ __forceinline__ int tswz(int d, int r) {
  return (d * 64 + (r ^ ((((d >> 3) ^ d) & 7) << 3))) * 2;
}

// write the quad-transposed columns into a [128][64] tswz image;
// r0 = quad's first row (multiple of 4), d0 = first column this lane owns.
__device__ __forceinline__ void write_transposed(char* img, int r0, int d0,
                                                 const int dw[4]) {
#pragma unroll
  for (int e = 0; e < 2; ++e) {
    const int d = d0 + e;
    unsigned w01 = e ? (((unsigned)dw[0] >> 16) | ((unsigned)dw[1] & 0xffff0000u))
                     : (((unsigned)dw[0] & 0xffffu) | ((unsigned)dw[1] << 16));
    unsigned w23 = e ? (((unsigned)dw[2] >> 16) | ((unsigned)dw[3] & 0xffff0000u))
                     : (((unsigned)dw[2] & 0xffffu) | ((unsigned)dw[3] << 16));
    int2v pair = {(int)w01, (int)w23};
    *reinterpret_cast<int2v*>(img + tswz(d, r0)) = pair;
  }
}

// pack one 16-reg crow-ordered f32 group (this lane + its ^32 partner) into
// two MFMA A-fragments covering k = 0..31 of that group's axis.
__device__ __forceinline__ void pack_pair(const float p[16], bf16x8 out[2]) {
#pragma unroll
  for (int ksl = 0; ksl < 2; ++ksl) {
    const float* pr = &p[8 * ksl];
    const unsigned x1 = cvt_pk_bf16_(pr[0], pr[1]);
    const unsigned x2 = cvt_pk_bf16_(pr[2], pr[3]);
    const unsigned y1 = cvt_pk_bf16_(pr[4], pr[5]);
    const unsigned y2 = cvt_pk_bf16_(pr[6], pr[7]);
    const int2v a = __builtin_amdgcn_permlane32_swap((int)x1, (int)y1, false, false);
    const int2v b = __builtin_amdgcn_permlane32_swap((int)x2, (int)y2, false, false);
    int w[4] = {a[0], b[0], a[1], b[1]};
    out[ksl] = *reinterpret_cast<const bf16x8*>(w);
  }
}

// ---------------------------------------------------------------------------
// delta = rowsum(dO * O), written as [B,H,S] fp32 (same layout as LSE2).
__global__ __launch_bounds__(256) void attn_bwd_delta_kernel(
    const short* __restrict__ dO, const short* __restrict__ O,
    float* __restrict__ delta, int64_t rows, int S, int H) {
  const int lg = threadIdx.x & 15;
  const int grp = (blockIdx.x * 256 + (int)threadIdx.x) >> 4;
  const int64_t stride = ((int64_t)gridDim.x * 256) >> 4;
  for (int64_t r = grp; r < rows; r += stride) {
    const bf16x8 d8 = *reinterpret_cast<const bf16x8*>(&dO[r * AB_D + lg * 8]);
    const bf16x8 o8 = *reinterpret_cast<const bf16x8*>(&O[r * AB_D + lg * 8]);
    float acc = 0.f;
#pragma unroll
    for (int j = 0; j < 8; ++j) acc += bf2f_(d8[j]) * bf2f_(o8[j]);
#pragma unroll
    for (int m = 1; m < 16; m <<= 1) acc += __shfl_xor(acc, m);
    if (lg == 0) {
      const int h = (int)(r % H);
      const int64_t bs = r / H;
      const int s = (int)(bs % S);
      const int64_t b = bs / S;
      delta[(b * H + h) * S + s] = acc;
    }
  }
}

// ---------------------------------------------------------------------------
// dQ: 8 waves x 32 q rows (lane&31 = own q row), KV tiles of 64,
// double-buffered K (normal), V (normal), K^T (tswz image).
constexpr int DQ_QW = 32, DQ_WAVES = 8, DQ_QB = 256, DQ_KVB = 64;

// Double-buffered images (96 KB LDS): staging runs one tile ahead and the
// loop has one barrier per tile.  After the barrier of tile t the registers
// holding tile t+1 are written into the other buffer and the global loads of
// tile t+2 are issued; no barrier separates those LDS writes from tile t's
// MFMAs.  The wave id is read into a scalar register, so the tile class
// (past the diagonal / masked / interior) is a scalar branch; interior tiles
// (entirely below the wave's diagonal and inside S) run a straight-line
// softmax, diagonal and tail tiles the masked form.
// gfx950 (hipcc -O3): NumVgprs 254, ScratchSize 0, Occupancy 2 waves/SIMD.
// 2 waves/SIMD = one 512-thread workgroup per CU; 256 VGPRs
__global__ __launch_bounds__(512, 2) void attn_bwd_dq_kernel(
    const short* __restrict__ Q, const short* __restrict__ K,
    const short* __restrict__ V, const short* __restrict__ dO,
    const float* __restrict__ LSE2, const float* __restrict__ Delta,
    short* __restrict__ dQ,
    int B, int S, int H, int HKV, float c, float scale,
    int order_mode, int order_G) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  // K@0 V@32K Kt@64K (+buf*16K each)
  auto k_lds = [&](int buf) -> char* { return smem + buf * 16384; };
  auto v_lds = [&](int buf) -> char* { return smem + 32768 + buf * 16384; };
  auto kt_lds = [&](int buf) -> char* { return smem + 65536 + buf * 16384; };

  const int tid = threadIdx.x;
  const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);  // wave-uniform: scalar
  const int lane = tid & 63;
  const int lq = lane & 31;
  const int hi2 = lane >> 5;

  const AttnBlock ob = attn_block_order(blockIdx.x, (S + DQ_QB - 1) / DQ_QB, B * H,
                                        order_G, ATTN_ORDER_FWD_DQ, order_mode);
  const int qblk = ob.blk;
  const int b = ob.head / H;
  const int h = ob.head % H;
  const int hkv = h / (H / HKV);
  const int64_t sHD = (int64_t)H * AB_D;
  const int64_t sHkvD = (int64_t)HKV * AB_D;
  const int64_t q_base = (((int64_t)b * S) * H + h) * AB_D;
  const int64_t kv_base = (((int64_t)b * S) * HKV + hkv) * AB_D;
  const int64_t ld_base = ((int64_t)b * H + h) * S;

  const int qw0 = qblk * DQ_QB + wid * DQ_QW;
  const int qrow = qw0 + lq;

  bf16x8 qf[8], dof[8];
  {
    const int64_t rb = q_base + (int64_t)min(qrow, S - 1) * sHD;
#pragma unroll
    for (int dc = 0; dc < 8; ++dc) {
      qf[dc] = *reinterpret_cast<const bf16x8*>(&Q[rb + dc * 16 + hi2 * 8]);
      dof[dc] = *reinterpret_cast<const bf16x8*>(&dO[rb + dc * 16 + hi2 * 8]);
    }
  }
  const float Lq = LSE2[ld_base + min(qrow, S - 1)];
  const float Dq = Delta[ld_base + min(qrow, S - 1)];

  const int st_r = lane >> 4;
  const int st_c = 8 * (lane & 15);
  const int kv_end = min(S, (qblk + 1) * DQ_QB);

  auto ld_tile = [&](int kv0, int pass, bf16x8& kreg, bf16x8& vreg) {
    const int row = min(kv0 + 4 * wid + 32 * pass + st_r, S - 1);
    const int64_t rb = kv_base + (int64_t)row * sHkvD + st_c;
    kreg = *reinterpret_cast<const bf16x8*>(&K[rb]);
    vreg = *reinterpret_cast<const bf16x8*>(&V[rb]);
  };
  auto write_tile = [&](int buf, int pass, bf16x8 kreg, bf16x8 vreg) {
    const int r = 4 * wid + 32 * pass + st_r;
    *reinterpret_cast<bf16x8*>(k_lds(buf) + bswz(r, st_c)) = kreg;
    *reinterpret_cast<bf16x8*>(v_lds(buf) + bswz(r, st_c)) = vreg;
    int dw[4];
    quad_transpose(kreg, st_r, dw);
    write_transposed(kt_lds(buf), 4 * wid + 32 * pass, st_c + 2 * st_r, dw);
  };

  f32x16 dq_acc[4];
#pragma unroll
  for (int dt = 0; dt < 4; ++dt)
#pragma unroll
    for (int r = 0; r < 16; ++r) dq_acc[dt][r] = 0.f;

  bf16x8 kreg0, kreg1, vreg0, vreg1;
  ld_tile(0, 0, kreg0, vreg0);
  ld_tile(0, 1, kreg1, vreg1);
  write_tile(0, 0, kreg0, vreg0);
  write_tile(0, 1, kreg1, vreg1);
  if (DQ_KVB < kv_end) {  // T14: pre-load tile 1 to registers
    ld_tile(DQ_KVB, 0, kreg0, vreg0);
    ld_tile(DQ_KVB, 1, kreg1, vreg1);
  }
  __syncthreads();

  for (int kv0 = 0, cur = 0; kv0 < kv_end; kv0 += DQ_KVB, cur ^= 1) {
    // T14 write-after-barrier: tile t+1 (in registers) goes into the other
    // buffer after the barrier and tile t+2's loads re-issue at once.
    if (kv0 + DQ_KVB < kv_end) {
      write_tile(cur ^ 1, 0, kreg0, vreg0);
      write_tile(cur ^ 1, 1, kreg1, vreg1);
      if (kv0 + 2 * DQ_KVB < kv_end) {
        ld_tile(kv0 + 2 * DQ_KVB, 0, kreg0, vreg0);
        ld_tile(kv0 + 2 * DQ_KVB, 1, kreg1, vreg1);
      }
    }

    if (kv0 < qw0 + DQ_QW) {
      // wave-uniform tile class: interior tiles take the straight-line form
      const bool need_mask = (kv0 + DQ_KVB > qw0) || (kv0 + DQ_KVB > S);
      // The tile runs as two independent 32-key halves, so only one half's
      // S^T/dP^T accumulators are live at a time and one half's softmax can
      // sit under the other half's MFMAs.  Each st/dpt element still sums
      // dc = 0..7 and each dq_acc element ks = 0..3, in that order.
#pragma unroll
      for (int t2 = 0; t2 < 2; ++t2) {
        f32x16 st, dpt;
#pragma unroll
        for (int r = 0; r < 16; ++r) { st[r] = 0.f; dpt[r] = 0.f; }
        __builtin_amdgcn_s_setprio(1);  // favour the MFMA cluster (guide T5)
#pragma unroll
        for (int dc = 0; dc < 8; ++dc) {
          const bf16x8 ak = *reinterpret_cast<const bf16x8*>(
              k_lds(cur) + bswz(t2 * 32 + lq, dc * 16 + hi2 * 8));
          const bf16x8 av = *reinterpret_cast<const bf16x8*>(
              v_lds(cur) + bswz(t2 * 32 + lq, dc * 16 + hi2 * 8));
          st = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ak, qf[dc], st, 0, 0, 0);
          dpt = __builtin_amdgcn_mfma_f32_32x32x16_bf16(av, dof[dc], dpt, 0, 0, 0);
        }
        __builtin_amdgcn_s_setprio(0);

        float ds[16];
        if (need_mask) {
#pragma unroll
          for (int r = 0; r < 16; ++r) {
            const int kv = kv0 + t2 * 32 + (r & 3) + 8 * (r >> 2) + 4 * hi2;
            const bool ok = (kv <= qrow) && (kv < S);
            const float e = exp2f(fmaf(st[r], c, -Lq));
            ds[r] = (ok ? e : 0.f) * (dpt[r] - Dq);
          }
        } else {
#pragma unroll
          for (int r = 0; r < 16; ++r)
            ds[r] = exp2f(fmaf(st[r], c, -Lq)) * (dpt[r] - Dq);
        }

        bf16x8 dsa[2];
        pack_pair(ds, dsa);

        __builtin_amdgcn_s_setprio(1);
#pragma unroll
        for (int dt = 0; dt < 4; ++dt) {
          const int d = dt * 32 + lq;
#pragma unroll
          for (int ks = 0; ks < 2; ++ks) {
            const bf16x8 bk = *reinterpret_cast<const bf16x8*>(
                kt_lds(cur) + tswz(d, (2 * t2 + ks) * 16 + hi2 * 8));
            dq_acc[dt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(dsa[ks], bk, dq_acc[dt], 0, 0, 0);
          }
        }
        __builtin_amdgcn_s_setprio(0);
      }
    }

    __syncthreads();  // the one barrier per tile, outside every wave condition
  }

#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int row = qw0 + (r & 3) + 8 * (r >> 2) + 4 * hi2;
    if (row >= S) continue;
    const int64_t rb = q_base + (int64_t)row * sHD;
#pragma unroll
    for (int dt = 0; dt < 4; ++dt) dQ[rb + dt * 32 + lq] = f2bf_(dq_acc[dt][r] * scale);
  }
}

// ---------------------------------------------------------------------------
// dK/dV: 8 waves x 16 kv rows (lane&15 = own kv row; 16x16x32 MFMA
// fragments), 512 threads, 2 waves/SIMD with no spills.  Grid over
// (S/128 kv blocks) x (B*HKV).  Per 32-row q tile (double-buffered):
//   S    = mfma16(Q_lds, K_reg)   C[q regs][kv lane]
//   dP   = mfma16(dO_lds, V_reg)  same layout
//   P    = exp2(c*S - L[q]);  dS = P*(dP - delta[q])   (L/D staged)
//   pack P, dS through a per-wave LDS tile into A[m=kv][k=q] fragments
//   dV  += mfma16(pack(P),  dO^T image);  dK += mfma16(pack(dS), Q^T image)
// GQA: the G query heads sharing a kv head accumulate in-register.
constexpr int KV_KW = 16, KV_WG = 128, KV_QT = 64;
constexpr int TS40 = 40;  // transposed-image row stride (odd word count)

typedef __attribute__((ext_vector_type(4))) float f32x4;


// Pack a (lane = n-axis, regs = crow16 q-axis) C-layout value set into the
// 16x16x32 MFMA A-fragment A[m = lane&15][k = (lane>>4)*8 + j] with pure
// cross-lane VALU ops (no LDS):
//   sources: X_qs = cvt_pk(p[qs][0], p[qs][1]), Y_qs = cvt_pk(p[qs][2], p[qs][3])
//   a = permlane32_swap(X0, X1); c  = permlane16_swap(a[0], a[0]);
//   c' = permlane16_swap(a[1], a[1])
//   d0 = (hi4&1) ? c'[0] : a[0];   d2 = (hi4&1) ? a[1] : c[1]
// (and the same for the Y family giving d1, d3).
__device__ __forceinline__ bf16x8 pack_frag16(const float p[2][4], int hi4_odd) {
  unsigned X0 = cvt_pk_bf16_(p[0][0], p[0][1]);
  unsigned Y0 = cvt_pk_bf16_(p[0][2], p[0][3]);
  unsigned X1 = cvt_pk_bf16_(p[1][0], p[1][1]);
  unsigned Y1 = cvt_pk_bf16_(p[1][2], p[1][3]);
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

// Same pipeline as the dQ kernel: double-buffered images (129 KB LDS), staging
// one tile ahead, one barrier per tile, scalar wave id, straight-line softmax
// on the half-tiles that need no mask.
// gfx950 (hipcc -O3): NumVgprs 220, ScratchSize 0, Occupancy 2 waves/SIMD.
// 2 waves/SIMD = one 512-thread workgroup per CU; 256 VGPRs
__global__ __launch_bounds__(512, 2) void attn_bwd_dkdv_kernel(
    const short* __restrict__ Q, const short* __restrict__ K,
    const short* __restrict__ V, const short* __restrict__ dO,
    const float* __restrict__ LSE2, const float* __restrict__ Delta,
    short* __restrict__ dK, short* __restrict__ dV,
    int B, int S, int H, int HKV, float c, float scale,
    int order_mode, int order_G) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  // 64-row tiles, [128][64] transposed images (16 KB each, +buf*16K):
  // Q@0 dO@32K Qt@64K dOt@96K L@128K D@128K+512
  auto q_lds = [&](int buf) -> char* { return smem + buf * 16384; };
  auto do_lds = [&](int buf) -> char* { return smem + 32768 + buf * 16384; };
  auto qt_lds = [&](int buf) -> char* { return smem + 65536 + buf * 16384; };
  auto dot_lds = [&](int buf) -> char* { return smem + 98304 + buf * 16384; };
  auto l_buf = [&](int buf) -> float* {
    return reinterpret_cast<float*>(smem + 131072) + buf * 64; };
  auto d_buf = [&](int buf) -> float* {
    return reinterpret_cast<float*>(smem + 131072 + 512) + buf * 64; };

  const int tid = threadIdx.x;
  const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);  // wave-uniform: scalar
  const int lane = tid & 63;
  const int l16 = lane & 15;
  const int hi4 = (lane >> 4) & 3;

  const AttnBlock ob = attn_block_order(blockIdx.x, (S + KV_WG - 1) / KV_WG, B * HKV,
                                        order_G, ATTN_ORDER_DKDV, order_mode);
  const int kvblk = ob.blk;
  const int b = ob.head / HKV;
  const int hkv = ob.head % HKV;
  const int G = H / HKV;
  const int64_t sHD = (int64_t)H * AB_D;
  const int64_t sHkvD = (int64_t)HKV * AB_D;
  const int64_t kv_base = (((int64_t)b * S) * HKV + hkv) * AB_D;

  const int kvw0 = kvblk * KV_WG + wid * KV_KW;  // wave's 16 kv rows
  const int kvrow = kvw0 + l16;                       // lane's kv row

  // K/V B-fragments (16x16x32: lane n = l16 = kv row, k = hi4*8+j)
  bf16x8 kf[4], vf[4];
  {
    const int64_t rb = kv_base + (int64_t)min(kvrow, S - 1) * sHkvD;
#pragma unroll
    for (int dc = 0; dc < 4; ++dc) {
      kf[dc] = *reinterpret_cast<const bf16x8*>(&K[rb + dc * 32 + hi4 * 8]);
      vf[dc] = *reinterpret_cast<const bf16x8*>(&V[rb + dc * 32 + hi4 * 8]);
    }
  }

  f32x4 dv_acc[8], dk_acc[8];
#pragma unroll
  for (int dt = 0; dt < 8; ++dt)
#pragma unroll
    for (int r = 0; r < 4; ++r) { dv_acc[dt][r] = 0.f; dk_acc[dt][r] = 0.f; }

  const int st_r = (lane >> 4) & 3;
  const int st_c = 8 * (lane & 15);
  const int qstart = kvblk * KV_WG;

  for (int g = 0; g < G; ++g) {
    const int h = hkv * G + g;
    const int64_t q_base = (((int64_t)b * S) * H + h) * AB_D;
    const int64_t ld_base = ((int64_t)b * H + h) * S;

    // two passes: 512 threads x 8 elems x 2 = one [64][128] tile
    auto ld_tile = [&](int qt0, int pass, bf16x8& qreg, bf16x8& dreg) {
      const int row = min(qt0 + 4 * wid + 32 * pass + st_r, S - 1);
      const int64_t rb = q_base + (int64_t)row * sHD + st_c;
      qreg = *reinterpret_cast<const bf16x8*>(&Q[rb]);
      dreg = *reinterpret_cast<const bf16x8*>(&dO[rb]);
    };
    auto write_tile = [&](int buf, int qt0, int pass, bf16x8 qreg, bf16x8 dreg) {
      const int r = 4 * wid + 32 * pass + st_r;
      *reinterpret_cast<bf16x8*>(q_lds(buf) + bswz(r, st_c)) = qreg;
      *reinterpret_cast<bf16x8*>(do_lds(buf) + bswz(r, st_c)) = dreg;
      int dw[4];
      quad_transpose(qreg, st_r, dw);
      write_transposed(qt_lds(buf), r - st_r, st_c + 2 * st_r, dw);
      quad_transpose(dreg, st_r, dw);
      write_transposed(dot_lds(buf), r - st_r, st_c + 2 * st_r, dw);
      if (pass == 0 && tid < 128) {
        const int qi = min(qt0 + (tid & 63), S - 1);
        if (tid < 64) l_buf(buf)[tid] = LSE2[ld_base + qi];
        else d_buf(buf)[tid & 63] = Delta[ld_base + qi];
      }
    };

    bf16x8 qreg0, dreg0, qreg1, dreg1;
    ld_tile(qstart, 0, qreg0, dreg0);
    ld_tile(qstart, 1, qreg1, dreg1);
    write_tile(0, qstart, 0, qreg0, dreg0);
    write_tile(0, qstart, 1, qreg1, dreg1);
    if (qstart + KV_QT < S) {  // T14: pre-load tile 1 to registers
      ld_tile(qstart + KV_QT, 0, qreg0, dreg0);
      ld_tile(qstart + KV_QT, 1, qreg1, dreg1);
    }
    __syncthreads();

    for (int qt0 = qstart, cur = 0; qt0 < S; qt0 += KV_QT, cur ^= 1) {
      // T14 write-after-barrier (see dq kernel)
      if (qt0 + KV_QT < S) {
        write_tile(cur ^ 1, qt0 + KV_QT, 0, qreg0, dreg0);
        write_tile(cur ^ 1, qt0 + KV_QT, 1, qreg1, dreg1);
        if (qt0 + 2 * KV_QT < S) {
          ld_tile(qt0 + 2 * KV_QT, 0, qreg0, dreg0);
          ld_tile(qt0 + 2 * KV_QT, 1, qreg1, dreg1);
        }
      }

      if (qt0 + KV_QT - 1 >= kvw0) {
#pragma unroll
        for (int half = 0; half < 2; ++half) {
          const int qh0 = qt0 + half * 32;
          if (qh0 + 31 < kvw0) continue;
          f32x4 st[2], dpt[2];
#pragma unroll
          for (int qs = 0; qs < 2; ++qs)
#pragma unroll
            for (int r = 0; r < 4; ++r) { st[qs][r] = 0.f; dpt[qs][r] = 0.f; }
          __builtin_amdgcn_s_setprio(1);
#pragma unroll
          for (int dc = 0; dc < 4; ++dc) {
#pragma unroll
            for (int qs = 0; qs < 2; ++qs) {
              const bf16x8 aq = *reinterpret_cast<const bf16x8*>(
                  q_lds(cur) + bswz(half * 32 + qs * 16 + l16, dc * 32 + hi4 * 8));
              const bf16x8 ad = *reinterpret_cast<const bf16x8*>(
                  do_lds(cur) + bswz(half * 32 + qs * 16 + l16, dc * 32 + hi4 * 8));
              st[qs] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(aq, kf[dc], st[qs], 0, 0, 0);
              dpt[qs] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ad, vf[dc], dpt[qs], 0, 0, 0);
            }
          }
          __builtin_amdgcn_s_setprio(0);

          // wave-uniform tile class.  An interior half-tile has
          // kvrow < qh0 and qh0 + 32 <= S, so every lane's kv row is inside S
          // and no element needs a mask: straight-line form.
          const bool need_mask = (qh0 < kvw0 + KV_KW) || (qh0 + 32 > S);
          float p[2][4], ds[2][4];
#pragma unroll
          for (int qs = 0; qs < 2; ++qs) {
            const int q0 = half * 32 + qs * 16 + hi4 * 4;
            const f32x4 Lr = *reinterpret_cast<const f32x4*>(&l_buf(cur)[q0]);
            const f32x4 Dr = *reinterpret_cast<const f32x4*>(&d_buf(cur)[q0]);
            if (need_mask) {
#pragma unroll
              for (int r = 0; r < 4; ++r) {
                const int q = qt0 + q0 + r;
                const bool ok = (kvrow < S) && (q >= kvrow) && (q < S);
                const float e = exp2f(fmaf(st[qs][r], c, -Lr[r]));
                p[qs][r] = ok ? e : 0.f;
                ds[qs][r] = p[qs][r] * (dpt[qs][r] - Dr[r]);
              }
            } else {
#pragma unroll
              for (int r = 0; r < 4; ++r) {
                p[qs][r] = exp2f(fmaf(st[qs][r], c, -Lr[r]));
                ds[qs][r] = p[qs][r] * (dpt[qs][r] - Dr[r]);
              }
            }
          }

          // cross-lane permlane pack (no LDS traffic)
          const bf16x8 pa = pack_frag16(p, hi4 & 1);
          const bf16x8 dsa = pack_frag16(ds, hi4 & 1);

          __builtin_amdgcn_s_setprio(1);
#pragma unroll
          for (int dt = 0; dt < 8; ++dt) {
            const int d = dt * 16 + l16;
            const bf16x8 bd = *reinterpret_cast<const bf16x8*>(
                dot_lds(cur) + tswz(d, half * 32 + hi4 * 8));
            const bf16x8 bq = *reinterpret_cast<const bf16x8*>(
                qt_lds(cur) + tswz(d, half * 32 + hi4 * 8));
            dv_acc[dt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(pa, bd, dv_acc[dt], 0, 0, 0);
            dk_acc[dt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(dsa, bq, dk_acc[dt], 0, 0, 0);
          }
          __builtin_amdgcn_s_setprio(0);
        }
      }

      __syncthreads();  // the one barrier per tile, outside every wave condition
    }
    __syncthreads();  // buffer 0 reuse across g
  }

#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int row = kvw0 + hi4 * 4 + r;
    if (row >= S) continue;
    const int64_t rb = kv_base + (int64_t)row * sHkvD;
#pragma unroll
    for (int dt = 0; dt < 8; ++dt) {
      dV[rb + dt * 16 + l16] = f2bf_(dv_acc[dt][r]);
      dK[rb + dt * 16 + l16] = f2bf_(dk_acc[dt][r] * scale);
    }
  }
}

// ---- launches ----------------------------------------------------------------
void launch_attn_fwd(const at::Tensor& q, const at::Tensor& k, const at::Tensor& v,
                     at::Tensor& o, at::Tensor& lse2, int order_mode, int order_G);

static void launch_attn_bwd_delta(const at::Tensor& dO, const at::Tensor& o,
                                  at::Tensor& delta) {
  const int B = dO.size(0), S = dO.size(1), H = dO.size(2);
  const int64_t rows = (int64_t)B * S * H;
  const int grid = grid_for(rows * 16, 256);
  hipLaunchKernelGGL(attn_bwd_delta_kernel, dim3(grid), dim3(256), 0, current_stream(),
                     (const short*)dO.data_ptr(), (const short*)o.data_ptr(),
                     delta.data_ptr<float>(), rows, S, H);
  LPP_CHECK_HIP(hipGetLastError());
}

// order_G <= 0 (both launches): heads per group = ATTN_GROUP_WAVES resident
// waves of workgroups per XCD (32 CUs x one workgroup per CU) over nblk; the
// factor is the measured winner of the G sweep, not a residency
// (profiles/README.md, Round 4).
static void launch_attn_bwd_dq(const at::Tensor& dO, const at::Tensor& q,
                               const at::Tensor& k, const at::Tensor& v,
                               const at::Tensor& lse2, const at::Tensor& delta,
                               at::Tensor& dq, int order_mode, int order_G) {
  const int B = q.size(0), S = q.size(1), H = q.size(2);
  const int HKV = k.size(2);
  const float scale = 1.0f / std::sqrt((float)AB_D);
  const float c = scale * 1.4426950408889634f;
  const int qblocks = (S + DQ_QB - 1) / DQ_QB;
  if (order_G <= 0)
    order_G = attn_order_group(ATTN_GROUP_WAVES * ATTN_RESIDENT_PER_XCD, qblocks);
  const size_t lds = 98304;
  hipLaunchKernelGGL(attn_bwd_dq_kernel, dim3(qblocks * B * H), dim3(512), lds,
                     current_stream(), (const short*)q.data_ptr(), (const short*)k.data_ptr(),
                     (const short*)v.data_ptr(), (const short*)dO.data_ptr(),
                     lse2.data_ptr<float>(), delta.data_ptr<float>(),
                     (short*)dq.data_ptr(), B, S, H, HKV, c, scale, order_mode, order_G);
  LPP_CHECK_HIP(hipGetLastError());
}

static void launch_attn_bwd_dkdv(const at::Tensor& dO, const at::Tensor& q,
                                 const at::Tensor& k, const at::Tensor& v,
                                 const at::Tensor& lse2, const at::Tensor& delta,
                                 at::Tensor& dk, at::Tensor& dv, int order_mode,
                                 int order_G) {
  const int B = q.size(0), S = q.size(1), H = q.size(2);
  const int HKV = k.size(2);
  const float scale = 1.0f / std::sqrt((float)AB_D);
  const float c = scale * 1.4426950408889634f;
  const int kvblocks = (S + KV_WG - 1) / KV_WG;
  if (order_G <= 0)
    order_G = attn_order_group(ATTN_GROUP_WAVES * ATTN_RESIDENT_PER_XCD, kvblocks);
  const size_t lds = 131072 + 1024;
  hipLaunchKernelGGL(attn_bwd_dkdv_kernel, dim3(kvblocks * B * HKV), dim3(512), lds,
                     current_stream(), (const short*)q.data_ptr(), (const short*)k.data_ptr(),
                     (const short*)v.data_ptr(), (const short*)dO.data_ptr(),
                     lse2.data_ptr<float>(), delta.data_ptr<float>(),
                     (short*)dk.data_ptr(), (short*)dv.data_ptr(), B, S, H, HKV, c,
                     scale, order_mode, order_G);
  LPP_CHECK_HIP(hipGetLastError());
}

}  // namespace lpp

static void attention_bwd_check(const at::Tensor& dO, const at::Tensor& q,
                                const at::Tensor& k, const at::Tensor& v,
                                const at::Tensor& o, const at::Tensor& lse2) {
  TORCH_CHECK(q.is_cuda() && q.scalar_type() == at::kBFloat16, "attention_bwd: bf16 only");
  TORCH_CHECK(q.dim() == 4 && q.size(3) == lpp::AB_D, "attention_bwd: [B,S,H,128] required");
  TORCH_CHECK(dO.is_contiguous() && q.is_contiguous() && k.is_contiguous() &&
              v.is_contiguous() && o.is_contiguous() && lse2.is_contiguous());
  TORCH_CHECK(q.size(2) % k.size(2) == 0);
}

std::vector<at::Tensor> attention_bwd(at::Tensor dO, at::Tensor q, at::Tensor k,
                                      at::Tensor v, at::Tensor o, at::Tensor lse2) {
  attention_bwd_check(dO, q, k, v, o, lse2);
  const int B = q.size(0), S = q.size(1), H = q.size(2);
  auto delta = at::empty({B, H, S}, q.options().dtype(at::kFloat));
  lpp::launch_attn_bwd_delta(dO, o, delta);
  auto dq = at::empty_like(q);
  auto dk = at::empty_like(k);
  auto dv = at::empty_like(v);
  const int mode = lpp::attn_order_mode();
  lpp::launch_attn_bwd_dq(dO, q, k, v, lse2, delta, dq, mode ? lpp::ATTN_MODE1_DQ : 0, 0);
  lpp::launch_attn_bwd_dkdv(dO, q, k, v, lse2, delta, dk, dv,
                            mode ? lpp::ATTN_MODE1_DKDV : 0, 0);
  return {dq, dk, dv};
}

// Device-timed A/B of one attention kernel under an explicit block order:
// kernel "fwd" | "dq" | "dkdv", order (mode, G; G <= 0 = the computed group).
// One hipEvent pair per launch; returns the ms of each of `reps` launches
// after `warmup` untimed ones.
std::vector<double> attention_time_kernel(std::string kernel, at::Tensor dO, at::Tensor q,
                                          at::Tensor k, at::Tensor v, at::Tensor o,
                                          at::Tensor lse2, int64_t mode, int64_t G,
                                          int64_t warmup, int64_t reps) {
  attention_bwd_check(dO, q, k, v, o, lse2);
  TORCH_CHECK(mode == 0 || mode == 1, "attention_time_kernel: mode 0 or 1");
  TORCH_CHECK(kernel == "fwd" || kernel == "dq" || kernel == "dkdv",
              "attention_time_kernel: kernel is fwd, dq or dkdv");
  const int B = q.size(0), S = q.size(1), H = q.size(2);
  auto delta = at::empty({B, H, S}, q.options().dtype(at::kFloat));
  lpp::launch_attn_bwd_delta(dO, o, delta);
  auto o2 = at::empty_like(q), dq = at::empty_like(q);
  auto lse_out = at::empty_like(lse2);
  auto dk = at::empty_like(k), dv = at::empty_like(v);
  auto launch = [&] {
    if (kernel == "fwd") lpp::launch_attn_fwd(q, k, v, o2, lse_out, (int)mode, (int)G);
    else if (kernel == "dq")
      lpp::launch_attn_bwd_dq(dO, q, k, v, lse2, delta, dq, (int)mode, (int)G);
    else lpp::launch_attn_bwd_dkdv(dO, q, k, v, lse2, delta, dk, dv, (int)mode, (int)G);
  };
  auto stream = lpp::current_stream();
  hipEvent_t e0, e1;
  LPP_CHECK_HIP(hipEventCreate(&e0));
  LPP_CHECK_HIP(hipEventCreate(&e1));
  for (int64_t i = 0; i < warmup; ++i) launch();
  std::vector<double> ms;
  for (int64_t i = 0; i < reps; ++i) {
    LPP_CHECK_HIP(hipEventRecord(e0, stream));
    launch();
    LPP_CHECK_HIP(hipEventRecord(e1, stream));
    LPP_CHECK_HIP(hipEventSynchronize(e1));
    float t = 0.f;
    LPP_CHECK_HIP(hipEventElapsedTime(&t, e0, e1));
    ms.push_back(t);
  }
  LPP_CHECK_HIP(hipEventDestroy(e0));
  LPP_CHECK_HIP(hipEventDestroy(e1));
  return ms;
}
