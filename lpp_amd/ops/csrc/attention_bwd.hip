// Flash-style causal attention BACKWARD for gfx950 (CDNA4), bf16, D=128.
//
// Completes the implicit-mask attention path (see attention_fwd.hip): the
// reference never had a working flash attention (README.md:141-143) and
// materialises the [B,1,S,S] mask host-side; here the backward recomputes
// P = exp2(c*QK^T - LSE2) tile-by-tile from the forward's base-2 logsumexp,
// so nothing S^2-shaped is ever stored.
//
// Same swapped-operand MFMA structure as the forward: the softmax-corrected
// tensors (P, dS) are always computed with the REDUCTION-FREE axis in the
// lane dimension, so the elementwise dS = P*(dP - delta) needs no cross-lane
// traffic, and the packed A-fragments for the accumulating GEMMs are built
// in registers (pack_pair / pack_frag16, attn_tile.h).  Both big kernels run
// one 512-thread workgroup per CU (2 waves/SIMD) through the attn_tile_pipeline
// schedule (dK/dV calls the template, dQ writes the same steps out):
// double-buffered 64-row LDS tiles, one dual-use image per staged operand
// (attn_tile.h), read by rows (ds_read_b128) for the A-fragments and by columns
// (ds_read_b64_tr_b16) for the B-fragments, one barrier per tile.  The
// wave id is read into a scalar register, so the tile class (past the
// diagonal / masked / interior) is a scalar branch; interior tiles run a
// straight-line softmax, diagonal and tail tiles the masked form.
//
// Three kernels:
//   1. delta[b,h,s] = rowsum(dO * O)                       (memory-bound)
//   2. dQ — 8 waves x 32 q rows (lane&31 = own q row, 32x32x16 fragments),
//      grid over 256-row q blocks x B*H; per 64-row KV tile, run as two
//      32-key halves:
//        S^T  = mfma(K_lds, Q_reg)   C[kv regs][q lane]
//        dP^T = mfma(V_lds, dO_reg)  same layout
//        P    = exp2(c*S^T - L[own q]);  dS = P*(dP^T - delta[own q])
//        dQ  += mfma(pack_pair(dS), K_lds transposed reads)  (scale at epilogue)
//   3. dK/dV — 8 waves x 16 kv rows (lane&15 = own kv row, 16x16x32
//      fragments), grid over 128-row kv blocks x B*HKV; per 64-row q tile,
//      run as two 32-row halves:
//        S    = mfma(Q_lds, K_reg)   C[q regs][kv lane]
//        dP   = mfma(dO_lds, V_reg)  same layout
//        P    = exp2(c*S - L[q]);  dS = P*(dP - delta[q])
//                                    (L, delta read from a staged tile)
//        dV  += mfma(pack_frag16(P),  dO_lds transposed reads)
//        dK  += mfma(pack_frag16(dS), Q_lds transposed reads)  (scale at epilogue)
//      GQA: the G query heads sharing a kv head accumulate in-register.
#include "attention.h"

namespace lpp {

// ---------------------------------------------------------------------------
// delta = rowsum(dO * O), written as [B,H,S] fp32 (same layout as LSE2).
__global__ __launch_bounds__(256) void attn_bwd_delta_kernel(
    const short* __restrict__ dO, const short* __restrict__ O,
    float* __restrict__ delta, int64_t rows, int S, int H) {
  const int lg = threadIdx.x & 15;
  const int grp = (blockIdx.x * 256 + (int)threadIdx.x) >> 4;
  const int64_t stride = ((int64_t)gridDim.x * 256) >> 4;
  for (int64_t r = grp; r < rows; r += stride) {
    const bf16x8 d8 = *reinterpret_cast<const bf16x8*>(&dO[r * ATTN_D + lg * 8]);
    const bf16x8 o8 = *reinterpret_cast<const bf16x8*>(&O[r * ATTN_D + lg * 8]);
    float acc = 0.f;
#pragma unroll
    for (int j = 0; j < 8; ++j) acc += bf16_to_f32(d8[j]) * bf16_to_f32(o8[j]);
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
// dQ.  LDS images (64 KB, attn_off<32>): K (row reads for S^T, transposed reads
// for dQ) and V (row reads).
constexpr int DQ_QW = 32, DQ_QB = 256, DQ_KVB = ATTN_TILE_ROWS;
enum { DQ_K, DQ_V, DQ_IMAGES };
constexpr int DQ_LDS_BYTES = attn_lds_bytes(DQ_IMAGES);

// DOCS (packed rows, see attention_fwd.hip): DocStart bounds the keys of each
// query from below; the tile loop begins at the workgroup's first start and a
// wave skips the tiles that end before its own.  DOCS=false is the plain kernel.
// gfx950 (hipcc -O3): DOCS=false NumVgprs 232, DOCS=true NumVgprs 232; both
// ScratchSize 0, Occupancy 2 waves/SIMD.
// 2 waves/SIMD = one 512-thread workgroup per CU; 256 VGPRs
template <bool DOCS>
__global__ __launch_bounds__(512, 2) void attn_bwd_dq_kernel(
    const short* __restrict__ Q, const short* __restrict__ K,
    const short* __restrict__ V, const short* __restrict__ dO,
    const float* __restrict__ LSE2, const float* __restrict__ Delta,
    short* __restrict__ dQ, const int* __restrict__ DocStart,
    int B, int S, int H, int HKV, float c, float scale,
    int order_mode, int order_G) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  auto k_lds = [&](int buf) -> char* { return attn_img(smem, DQ_K, buf); };
  auto v_lds = [&](int buf) -> char* { return attn_img(smem, DQ_V, buf); };

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
  const int64_t sHD = (int64_t)H * ATTN_D;
  const int64_t sHkvD = (int64_t)HKV * ATTN_D;
  const int64_t q_base = (((int64_t)b * S) * H + h) * ATTN_D;
  const int64_t kv_base = (((int64_t)b * S) * HKV + hkv) * ATTN_D;
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
  const int st_off[2] = {attn_stage_off<32>(wid, 0, lane), attn_stage_off<32>(wid, 1, lane)};
  const int kv_end = min(S, (qblk + 1) * DQ_QB);

  // Document starts (DOCS): the lane's own and, wave-uniform, the wave's
  // smallest (first row) and largest (last valid row) and the workgroup's
  // smallest (first row; qblk * DQ_QB < S always), floored to a tile.
  int qs = 0, qs_wmin = 0, qs_wmax = 0, kv_begin = 0;
  if constexpr (DOCS) {
    const int* ds_row = DocStart + (int64_t)b * S;
    qs = ds_row[min(qrow, S - 1)];
    qs_wmin = __builtin_amdgcn_readfirstlane(ds_row[min(qw0, S - 1)]);
    qs_wmax = __builtin_amdgcn_readfirstlane(ds_row[min(qw0 + DQ_QW - 1, S - 1)]);
    // clamped to the rows that exist, whatever the tensor holds
    kv_begin = min(max(__builtin_amdgcn_readfirstlane(ds_row[qblk * DQ_QB]), 0),
                   qblk * DQ_QB) & ~(DQ_KVB - 1);
  }

  auto ld_tile = [&](int kv0, int pass, bf16x8& kreg, bf16x8& vreg) {
    const int row = min(kv0 + stage_row(wid, pass, st_r), S - 1);
    const int64_t rb = kv_base + (int64_t)row * sHkvD + st_c;
    kreg = *reinterpret_cast<const bf16x8*>(&K[rb]);
    vreg = *reinterpret_cast<const bf16x8*>(&V[rb]);
  };
  auto write_tile = [&](int buf, int pass, bf16x8 kreg, bf16x8 vreg) {
    stage_chunk(k_lds(buf), st_off[pass], kreg);
    stage_chunk(v_lds(buf), st_off[pass], vreg);
  };

  f32x16 dq_acc[4];
#pragma unroll
  for (int dt = 0; dt < 4; ++dt)
#pragma unroll
    for (int r = 0; r < 16; ++r) dq_acc[dt][r] = 0.f;

  // attn_tile_pipeline (attn_tile.h) written out: passing this body to the
  // template cost 57 more v_mov_b32 and measured 3-5% slower (round 5, at 254
  // VGPRs).
  bf16x8 kreg0, kreg1, vreg0, vreg1;
  ld_tile(kv_begin, 0, kreg0, vreg0);
  ld_tile(kv_begin, 1, kreg1, vreg1);
  write_tile(0, 0, kreg0, vreg0);
  write_tile(0, 1, kreg1, vreg1);
  if (kv_begin + DQ_KVB < kv_end) {
    ld_tile(kv_begin + DQ_KVB, 0, kreg0, vreg0);
    ld_tile(kv_begin + DQ_KVB, 1, kreg1, vreg1);
  }
  __syncthreads();
  for (int kv0 = kv_begin, cur = 0; kv0 < kv_end; kv0 += DQ_KVB, cur ^= 1) {
    if (kv0 + DQ_KVB < kv_end) {
      write_tile(cur ^ 1, 0, kreg0, vreg0);
      write_tile(cur ^ 1, 1, kreg1, vreg1);
      if (kv0 + 2 * DQ_KVB < kv_end) {
        ld_tile(kv0 + 2 * DQ_KVB, 0, kreg0, vreg0);
        ld_tile(kv0 + 2 * DQ_KVB, 1, kreg1, vreg1);
      }
    }
    // causal: not past this wave's diagonal; documents: not wholly before the
    // first key any row of this wave sees (both scalar conditions)
    if (kv0 < qw0 + DQ_QW && !(DOCS && kv0 + DQ_KVB <= qs_wmin)) {
      // wave-uniform tile class: interior tiles take the straight-line form
      const bool need_mask =
          (kv0 + DQ_KVB > qw0) || (kv0 + DQ_KVB > S) || (DOCS && kv0 < qs_wmax);
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
          const bf16x8 ak = read_row_frag(k_lds(cur), attn_row_off32(lane, t2, dc));
          const bf16x8 av = read_row_frag(v_lds(cur), attn_row_off32(lane, t2, dc));
          st = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ak, qf[dc], st, 0, 0, 0);
          dpt = __builtin_amdgcn_mfma_f32_32x32x16_bf16(av, dof[dc], dpt, 0, 0, 0);
        }
        __builtin_amdgcn_s_setprio(0);

        float ds[16];
        if (need_mask) {
#pragma unroll
          for (int r = 0; r < 16; ++r) {
            const int kv = kv0 + t2 * 32 + crow32(r, hi2);
            const bool ok = (kv <= qrow) && (kv < S) && (!DOCS || kv >= qs);
            const float e = attn_exp2(fmaf(st[r], c, -Lq));
            ds[r] = (ok ? e : 0.f) * (dpt[r] - Dq);
          }
        } else {
#pragma unroll
          for (int r = 0; r < 16; ++r)
            ds[r] = attn_exp2(fmaf(st[r], c, -Lq)) * (dpt[r] - Dq);
        }

        bf16x8 dsa[2];
        pack_pair(ds, dsa);

        __builtin_amdgcn_s_setprio(1);
#pragma unroll
        for (int dt = 0; dt < 4; ++dt) {
#pragma unroll
          for (int ks = 0; ks < 2; ++ks) {
            const bf16x8 bk =
                read_tr_frag(k_lds(cur), attn_tr_off32(lane, dt, 2 * t2 + ks, 0),
                             attn_tr_off32(lane, dt, 2 * t2 + ks, 1));
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
    const int row = qw0 + crow32(r, hi2);
    if (row >= S) continue;
    const int64_t rb = q_base + (int64_t)row * sHD;
#pragma unroll
    for (int dt = 0; dt < 4; ++dt)
      dQ[rb + dt * 32 + lq] = f32_to_bf16(dq_acc[dt][r] * scale);
  }
}

// ---------------------------------------------------------------------------
// dK/dV.  LDS images (64 KB, attn_off<16>): Q and dO, each read by rows for S
// and dP and by transposed reads for dK and dV; then the tile's 64 LSE2 and 64
// delta values, double-buffered like the images.
constexpr int KV_KW = 16, KV_WG = 128, KV_QT = ATTN_TILE_ROWS;
enum { KV_Q, KV_DO, KV_IMAGES };
constexpr int KV_LD_OFF = attn_lds_bytes(KV_IMAGES);                   // float L[2][64]
constexpr int KV_D_OFF = KV_LD_OFF + 2 * KV_QT * (int)sizeof(float);   // float D[2][64]
constexpr int KV_LDS_BYTES = KV_D_OFF + 2 * KV_QT * (int)sizeof(float);

// DOCS (packed rows): DocEnd[b][j] (int32 [B,S], non-decreasing, > j) is one
// past the last token of the document that holds key j; key j is seen by
// queries j .. DocEnd[b][j]-1.  It is monotone, so the workgroup's q loop ends
// at the end of its last key row and a wave skips the tiles from the end of its
// own last row on.  No per-query lookup.  DOCS=false is the plain kernel.
// gfx950 (hipcc -O3): DOCS=false NumVgprs 204, DOCS=true NumVgprs 232; both
// ScratchSize 0, Occupancy 2 waves/SIMD.
// 2 waves/SIMD = one 512-thread workgroup per CU; 256 VGPRs
template <bool DOCS>
__global__ __launch_bounds__(512, 2) void attn_bwd_dkdv_kernel(
    const short* __restrict__ Q, const short* __restrict__ K,
    const short* __restrict__ V, const short* __restrict__ dO,
    const float* __restrict__ LSE2, const float* __restrict__ Delta,
    short* __restrict__ dK, short* __restrict__ dV, const int* __restrict__ DocEnd,
    int B, int S, int H, int HKV, float c, float scale,
    int order_mode, int order_G) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  auto q_lds = [&](int buf) -> char* { return attn_img(smem, KV_Q, buf); };
  auto do_lds = [&](int buf) -> char* { return attn_img(smem, KV_DO, buf); };
  auto l_buf = [&](int buf) -> float* {
    return reinterpret_cast<float*>(smem + KV_LD_OFF) + buf * KV_QT; };
  auto d_buf = [&](int buf) -> float* {
    return reinterpret_cast<float*>(smem + KV_D_OFF) + buf * KV_QT; };

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
  const int64_t sHD = (int64_t)H * ATTN_D;
  const int64_t sHkvD = (int64_t)HKV * ATTN_D;
  const int64_t kv_base = (((int64_t)b * S) * HKV + hkv) * ATTN_D;

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
  const int st_off[2] = {attn_stage_off<16>(wid, 0, lane), attn_stage_off<16>(wid, 1, lane)};
  const int qstart = kvblk * KV_WG;

  // Document ends (DOCS): the lane's own and, wave-uniform, those of the
  // wave's first and last key row and of the workgroup's last key row, where
  // the q loop ends: the same value in all 512 threads (the pipeline's barrier
  // is inside the loop) and > qstart, since DocEnd[j] > j and qstart < S.
  int ke = S, ke_wmin = S, ke_wmax = S, q_end = S;
  if constexpr (DOCS) {
    const int* de_row = DocEnd + (int64_t)b * S;
    ke = de_row[min(kvrow, S - 1)];
    ke_wmin = __builtin_amdgcn_readfirstlane(de_row[min(kvw0, S - 1)]);
    ke_wmax = __builtin_amdgcn_readfirstlane(de_row[min(kvw0 + KV_KW - 1, S - 1)]);
    // clamped to (qstart, S], whatever the tensor holds
    q_end = min(max(__builtin_amdgcn_readfirstlane(de_row[min(qstart + KV_WG - 1, S - 1)]),
                    qstart + 1), S);
  }

  for (int g = 0; g < G; ++g) {
    const int h = hkv * G + g;
    const int64_t q_base = (((int64_t)b * S) * H + h) * ATTN_D;
    const int64_t ld_base = ((int64_t)b * H + h) * S;

    auto ld_tile = [&](int qt0, int pass, bf16x8& qreg, bf16x8& dreg) {
      const int row = min(qt0 + stage_row(wid, pass, st_r), S - 1);
      const int64_t rb = q_base + (int64_t)row * sHD + st_c;
      qreg = *reinterpret_cast<const bf16x8*>(&Q[rb]);
      dreg = *reinterpret_cast<const bf16x8*>(&dO[rb]);
    };
    auto write_tile = [&](int buf, int qt0, int pass, bf16x8 qreg, bf16x8 dreg) {
      stage_chunk(q_lds(buf), st_off[pass], qreg);
      stage_chunk(do_lds(buf), st_off[pass], dreg);
      if (pass == 0 && tid < 128) {
        const int qi = min(qt0 + (tid & 63), S - 1);
        if (tid < 64) l_buf(buf)[tid] = LSE2[ld_base + qi];
        else d_buf(buf)[tid & 63] = Delta[ld_base + qi];
      }
    };

    attn_tile_pipeline<KV_QT>(qstart, DOCS ? q_end : S, ld_tile, write_tile,
                              [&](int qt0, int cur) {
      if (qt0 + KV_QT - 1 < kvw0) return;  // causal: tile above this wave's diagonal
      if constexpr (DOCS) {
        if (qt0 >= ke_wmax) return;  // documents: past the last query of this wave's keys
      }
#pragma unroll
      for (int half = 0; half < 2; ++half) {
        const int qh0 = qt0 + half * 32;
        if (qh0 + 31 < kvw0) continue;
        if constexpr (DOCS) {
          if (qh0 >= ke_wmax) continue;
        }
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
            const int off = attn_row_off16(lane, 2 * half + qs, dc);
            const bf16x8 aq = read_row_frag(q_lds(cur), off);
            const bf16x8 ad = read_row_frag(do_lds(cur), off);
            st[qs] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(aq, kf[dc], st[qs], 0, 0, 0);
            dpt[qs] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ad, vf[dc], dpt[qs], 0, 0, 0);
          }
        }
        __builtin_amdgcn_s_setprio(0);

        // wave-uniform tile class.  An interior half-tile has
        // kvrow < qh0 and qh0 + 32 <= S, so every lane's kv row is inside S
        // and no element needs a mask: straight-line form.
        const bool need_mask =
            (qh0 < kvw0 + KV_KW) || (qh0 + 32 > S) || (DOCS && qh0 + 32 > ke_wmin);
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
              const bool ok = (kvrow < S) && (q >= kvrow) && (q < S) && (!DOCS || q < ke);
              const float e = attn_exp2(fmaf(st[qs][r], c, -Lr[r]));
              p[qs][r] = ok ? e : 0.f;
              ds[qs][r] = p[qs][r] * (dpt[qs][r] - Dr[r]);
            }
          } else {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
              p[qs][r] = attn_exp2(fmaf(st[qs][r], c, -Lr[r]));
              ds[qs][r] = p[qs][r] * (dpt[qs][r] - Dr[r]);
            }
          }
        }

        const bf16x8 pa = pack_frag16(p, hi4 & 1);
        const bf16x8 dsa = pack_frag16(ds, hi4 & 1);

        __builtin_amdgcn_s_setprio(1);
#pragma unroll
        for (int dt = 0; dt < 8; ++dt) {
          const int off0 = attn_tr_off16(lane, dt, half, 0);
          const int off1 = attn_tr_off16(lane, dt, half, 1);
          const bf16x8 bd = read_tr_frag(do_lds(cur), off0, off1);
          const bf16x8 bq = read_tr_frag(q_lds(cur), off0, off1);
          dv_acc[dt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(pa, bd, dv_acc[dt], 0, 0, 0);
          dk_acc[dt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(dsa, bq, dk_acc[dt], 0, 0, 0);
        }
        __builtin_amdgcn_s_setprio(0);
      }
    });
    __syncthreads();  // buffer 0 reuse across g
  }

#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int row = kvw0 + hi4 * 4 + r;
    if (row >= S) continue;
    const int64_t rb = kv_base + (int64_t)row * sHkvD;
#pragma unroll
    for (int dt = 0; dt < 8; ++dt) {
      dV[rb + dt * 16 + l16] = f32_to_bf16(dv_acc[dt][r]);
      dK[rb + dt * 16 + l16] = f32_to_bf16(dk_acc[dt][r] * scale);
    }
  }
}

// ---- launches (order_G: see attention.h) --------------------------------------
void launch_attn_bwd_delta(const at::Tensor& dO, const at::Tensor& o, at::Tensor& delta) {
  const int B = dO.size(0), S = dO.size(1), H = dO.size(2);
  const int64_t rows = (int64_t)B * S * H;
  const int grid = grid_for(rows * 16, 256);
  hipLaunchKernelGGL(attn_bwd_delta_kernel, dim3(grid), dim3(256), 0, current_stream(),
                     (const short*)dO.data_ptr(), (const short*)o.data_ptr(),
                     delta.data_ptr<float>(), rows, S, H);
  LPP_CHECK_HIP(hipGetLastError());
}

void launch_attn_bwd_dq(const at::Tensor& dO, const at::Tensor& q, const at::Tensor& k,
                        const at::Tensor& v, const at::Tensor& lse2,
                        const at::Tensor& delta, at::Tensor& dq, int order_mode,
                        int order_G, const at::Tensor* doc_start) {
  const int B = q.size(0), S = q.size(1), H = q.size(2);
  const int HKV = k.size(2);
  const AttnScale sc = attn_scale();
  const int qblocks = (S + DQ_QB - 1) / DQ_QB;
  if (order_G <= 0)
    order_G = attn_order_group(ATTN_GROUP_WAVES * ATTN_RESIDENT_PER_XCD, qblocks);
  const int* ds = doc_start ? doc_start->data_ptr<int>() : nullptr;
  hipLaunchKernelGGL(ds ? attn_bwd_dq_kernel<true> : attn_bwd_dq_kernel<false>,
                     dim3(qblocks * B * H), dim3(512), DQ_LDS_BYTES,
                     current_stream(), (const short*)q.data_ptr(), (const short*)k.data_ptr(),
                     (const short*)v.data_ptr(), (const short*)dO.data_ptr(),
                     lse2.data_ptr<float>(), delta.data_ptr<float>(),
                     (short*)dq.data_ptr(), ds, B, S, H, HKV, sc.c, sc.scale, order_mode,
                     order_G);
  LPP_CHECK_HIP(hipGetLastError());
}

void launch_attn_bwd_dkdv(const at::Tensor& dO, const at::Tensor& q, const at::Tensor& k,
                          const at::Tensor& v, const at::Tensor& lse2,
                          const at::Tensor& delta, at::Tensor& dk, at::Tensor& dv,
                          int order_mode, int order_G, const at::Tensor* doc_end) {
  const int B = q.size(0), S = q.size(1), H = q.size(2);
  const int HKV = k.size(2);
  const AttnScale sc = attn_scale();
  const int kvblocks = (S + KV_WG - 1) / KV_WG;
  if (order_G <= 0)
    order_G = attn_order_group(ATTN_GROUP_WAVES * ATTN_RESIDENT_PER_XCD, kvblocks);
  const int* de = doc_end ? doc_end->data_ptr<int>() : nullptr;
  hipLaunchKernelGGL(de ? attn_bwd_dkdv_kernel<true> : attn_bwd_dkdv_kernel<false>,
                     dim3(kvblocks * B * HKV), dim3(512),
                     KV_LDS_BYTES, current_stream(), (const short*)q.data_ptr(),
                     (const short*)k.data_ptr(), (const short*)v.data_ptr(),
                     (const short*)dO.data_ptr(), lse2.data_ptr<float>(),
                     delta.data_ptr<float>(), (short*)dk.data_ptr(),
                     (short*)dv.data_ptr(), de, B, S, H, HKV, sc.c, sc.scale, order_mode,
                     order_G);
  LPP_CHECK_HIP(hipGetLastError());
}

}  // namespace lpp
