// Single-token decode attention over an FP8 (e4m3) ragged KV cache, gfx950:
// attention_decode_mfma.hip with half the cache bytes.  Same contract, same
// decomposition and the same workspace: grid (ceil(max_len/C), Hkv, N), 256
// threads, a wave owns C/4 keys in steps of 32, one unnormalised fp32 partial
// per head and chunk, finished by attn_decode_combine_kernel.
//
// Format (attn_fp8.h): a cached row is 128 e4m3 bytes plus one power-of-two
// fp32 scale, k_scale / v_scale [slots,Hkv,Tmax], key-contiguous so a wave
// reads the scales of its 32 keys as one dense run.  byte * scale is exact in
// bf16, so the cache is turned into bf16 in registers, the scale folded into
// v_cvt_scalef32_pk_bf16_fp8, and the bf16 MFMAs, the V staging and the softmax
// of the bf16 kernel run on it unchanged.  Q and P stay bf16.
//
// Every group size 1, 2, 4, 8 and 16 runs here: the group's heads are the N
// side of v_mfma_f32_16x16x32_bf16 and the columns past REP are zero.  A step
// of 32 keys is 8 KB of cache against 16 MFMAs and 64 conversions, far below
// what the loads take, whatever REP is.
//
// Scores, S^T = K Q^T.  The contraction index of an MFMA is free as long as
// both operands agree, so a lane does not take 8 dims per k-step from four
// places of the row but owns one run of it:
//   A = K   lane l: key l&15 of the tile, dims g*32 .. g*32+31 (g = l>>4): two
//           16-byte loads per tile, converted with the key's scale; k-step ks
//           takes bytes ks*8 .. +7, i.e. dims g*32 + ks*8 + i at k = g*8 + i.
//   B = Q^T lane l: head l&15, the same dims: chunk g*4 + ks of the rotated q
//           in LDS (the bf16 kernel reads chunk ks*4 + g).
// Output, O^T += V^T P^T: a V key row is 128 bytes, so 8 lanes fetch one row in
// 16-byte loads (lane l: key l>>3 of 8, dims (l&7)*16 .. +15) and a step is 4
// loads, not 8.  Each lane converts its 16 dims with the key's scale and stores
// the two bf16 chunks 2(l&7), 2(l&7)+1 of the staged row; under vstage_off's
// swizzle (chunk ^ 2(row & 7)) they stay one aligned 32-byte pair.  The
// ds_read_b64_tr_b16 side, P and the accumulators are the bf16 kernel's.
//
// The step holding key p loads under a per-lane predicate: keys < p from the
// cache, key p from LDS, nothing beyond - no cache byte and no scale at a
// position >= p is ever addressed.  The new token is quantised first (waves 0
// and 1 of the owner workgroup: amax by a wave reduction, the exponent from the
// float's bits, v_cvt_pk_fp8_f32) and kn_s / vn_s then hold its dequantised
// bf16 row, so it is attended as exactly what a later call reads back.
//
// Every merge order is fixed, so a row's bits depend on its own data and p alone.
//
// PAGED (attn_paged.h): as in attention_decode_mfma.hip - the one or two page
// ids of a wave's keys come from scalar loads ahead of the prologue and a step
// adds its page's base.  The scales take the same lookup, scale[page, hkv,
// t & 63]: a step's 32 scales stay one dense run.  The new token's bytes and
// scale go to the page of key p.
// The slot instantiation keeps the row's base folded into its per-lane
// pointers, as it always had; the paged one adds the page's base per step.
// gfx950 (hipcc -O3), slot / paged, every REP: NumVgprs 105-106 / 103-104
// (C = 128, 4 waves/SIMD), 144 / 148 (C = 256, 3), 144 / 140 (C = 512, 3);
// ScratchSize 0 everywhere.
#include "attention_decode.h"
#include "attn_fp8.h"

namespace lpp {

template <int REP, int C, bool PAGED>
__global__ __launch_bounds__(kDecodeThreads, 3) void attn_decode_fp8_kernel(
    const __hip_bfloat16* __restrict__ q,      // [N,1,H,128]
    const __hip_bfloat16* __restrict__ k_new,  // [N,1,Hkv,128]
    const __hip_bfloat16* __restrict__ v_new,  // [N,1,Hkv,128]
    uint8_t* k_cache,                          // [slots,Tmax,Hkv,128] e4m3; PAGED: the pool
    uint8_t* v_cache,
    float* k_scale,                            // [slots,Hkv,Tmax]
    float* v_scale,
    const float* __restrict__ cos_t,           // [Smax,64]
    const float* __restrict__ sin_t,
    const int64_t* __restrict__ positions,     // [N] or null
    const int64_t* __restrict__ rows,          // [N] or null
    int64_t* lengths,                          // [slots] or null
    float* __restrict__ ws,                    // [N,H,J,kDecodeWs]
    PageTable pt,                              // PAGED: slots counts the table's rows
    int uniform_pos, int max_len, int slots, int Tmax, int Hkv, int J, float c) {
  static_assert(REP >= 1 && REP <= 16, "the group's heads are one MFMA tile of 16 columns");
  constexpr int KPW = C / kDecodeWaves;        // keys per wave
  constexpr int STEP = kMfmaStep;
  constexpr int NSTEP = KPW / STEP;
  constexpr int HALF = ATTN_D / 2;
  static_assert(KPW % STEP == 0, "chunk must split into whole wave steps");

  const int j = blockIdx.x, kvh = blockIdx.y, n = blockIdx.z;
  const int H = Hkv * REP;
  const DecodeRow row = decode_row(positions, rows, n, uniform_pos, slots, max_len);
  if (!row.ok) return;
  const int p = row.p;
  const int chunk0 = j * C;
  if (chunk0 > p) return;                      // chunk starts beyond this row
  const bool owner = p < chunk0 + C;           // this chunk holds the new token

  __shared__ uint32_t q_s[REP][HALF];          // rotated q, bf16 pairs
  __shared__ uint4 kn_s[ATTN_D / 8];           // k_new: rotated, then dequantised, bf16
  __shared__ uint4 vn_s[ATTN_D / 8];
  // V staging of the 4 waves in the loop, the 4-wave merge after it
  __shared__ __attribute__((aligned(16))) char buf_s[decode_mfma_lds<REP>()];
  float(*st_s)[REP][kDecodeWs] = reinterpret_cast<float(*)[REP][kDecodeWs]>(buf_s);

  const int tid = threadIdx.x;
  const int lane = tid & (kWave - 1);
  const int wid = __builtin_amdgcn_readfirstlane(tid / kWave);
  const int l16 = lane & 15;                   // K: key of a tile; Q, S, P, O: head
  const int g = lane >> 4;                     // lane group
  const int c8 = lane & 7, kr = lane >> 3;     // V: 16-dim run and key of a load

  // key 0 of the row in the slot layout; PAGED: a step adds its page's (page_kv)
  const int64_t row_base = PAGED ? 0 : ((row.r * Tmax) * (int64_t)Hkv + kvh) * ATTN_D;  // bytes
  const int64_t key_stride = (int64_t)Hkv * ATTN_D;
  const int64_t scale_base = PAGED ? 0 : (row.r * Hkv + kvh) * (int64_t)Tmax;
  const int wave0 = chunk0 + wid * KPW;        // first key of this wave
  // PAGED: where this wave's keys and scales live, its one or two pages
  [[maybe_unused]] const DecodeRuns<PAGED, KPW> runs(pt, row.r, Tmax, Hkv, kvh, wave0, p);
  auto page_kv = [&](int key0) -> int64_t {
    if constexpr (PAGED) return runs.at(key0 - wave0).kv;
    else return 0;
  };
  auto page_scale = [&](int key0) -> int64_t {
    if constexpr (PAGED) return runs.at(key0 - wave0).scale;
    else return 0;
  };

  // ---- RoPE (pairs (d, d+64), fp32, rounded to bf16) -> LDS -----------------
  const float* cr = cos_t + (int64_t)p * HALF;
  const float* sr = sin_t + (int64_t)p * HALF;
  {
    unsigned short* q16 = reinterpret_cast<unsigned short*>(&q_s[0][0]);
    const __hip_bfloat16* qn = q + ((int64_t)n * H + (int64_t)kvh * REP) * ATTN_D;
    for (int idx = tid; idx < REP * HALF; idx += kDecodeThreads) {
      const int h = idx / HALF, d = idx % HALF;
      const float a = __bfloat162float(qn[h * ATTN_D + d]);
      const float b = __bfloat162float(qn[h * ATTN_D + d + HALF]);
      const float cs = cr[d], sn = sr[d];
      q16[h * ATTN_D + d] = (unsigned short)bf16_bits(__fsub_rn(__fmul_rn(a, cs), __fmul_rn(b, sn)));
      q16[h * ATTN_D + d + HALF] =
          (unsigned short)bf16_bits(__fadd_rn(__fmul_rn(b, cs), __fmul_rn(a, sn)));
    }
  }
  if (owner) {
    const int64_t nb = ((int64_t)n * Hkv + kvh) * ATTN_D;
    if (tid < HALF) {
      unsigned short* k16 = reinterpret_cast<unsigned short*>(kn_s);
      const float a = __bfloat162float(k_new[nb + tid]);
      const float b = __bfloat162float(k_new[nb + tid + HALF]);
      const float cs = cr[tid], sn = sr[tid];
      k16[tid] = (unsigned short)bf16_bits(__fsub_rn(__fmul_rn(a, cs), __fmul_rn(b, sn)));
      k16[tid + HALF] = (unsigned short)bf16_bits(__fadd_rn(__fmul_rn(b, cs), __fmul_rn(a, sn)));
    } else if (tid < HALF + ATTN_D / 8) {
      vn_s[tid - HALF] = reinterpret_cast<const uint4*>(v_new + nb)[tid - HALF];
    }
  }
  __syncthreads();

  // ---- quantise the new token, keep its dequantised row, store it ------------
  // Wave 0 takes K, wave 1 V; lane l holds dims 2l and 2l+1.  The cache entry
  // at p is read by nobody in this launch, so it is stored right here.
  if (owner) {                                 // workgroup-uniform
    KvRun at_p{0, 0, true};                    // PAGED: the page of key p
    if constexpr (PAGED) at_p = kv_run<PAGED>(pt, row.r, Tmax, Hkv, kvh, p);
    if (wid < 2) {
      uint32_t* rw = reinterpret_cast<uint32_t*>(wid == 0 ? kn_s : vn_s);
      const uint32_t w = rw[lane];
      const float a = as_f((int)(w << 16)), b = as_f((int)(w & 0xffff0000u));
      float amax = fmaxf(fabsf(a), fabsf(b));
#pragma unroll
      for (int off = kWave / 2; off > 0; off >>= 1) amax = fmaxf(amax, __shfl_xor(amax, off));
      const int e = fp8_row_exp(amax);
      const float sc = fp8_pow2(e), inv = fp8_pow2(-e);
      const uint32_t qb = fp8_pack2(__fmul_rn(a, inv), __fmul_rn(b, inv));
      const fp8_f32x2 dq = fp8_unpack2(qb);
      rw[lane] = cvt_pk_bf16(__fmul_rn(dq[0], sc), __fmul_rn(dq[1], sc));  // exact
      // (a table entry outside the pool: the token is not stored)
      uint8_t* dst =
          (wid == 0 ? k_cache : v_cache) + row_base + at_p.kv + (int64_t)p * key_stride;
      if (at_p.ok) reinterpret_cast<unsigned short*>(dst)[lane] = (unsigned short)qb;
      if (at_p.ok && lane == 0)
        (wid == 0 ? k_scale : v_scale)[scale_base + at_p.scale + p] = sc;
    } else if (lengths && kvh == 0 && tid == 2 * kWave) {
      lengths[row.r] = (int64_t)p + 1;
    }
    __syncthreads();
  }

  // ---- Q^T fragments: head l16 (none at l16 >= REP), dims g*32 + ks*8 .. +7 ----
  bf16x8 qf[4];
#pragma unroll
  for (int ks = 0; ks < 4; ++ks) {
    uint4 w = make_uint4(0u, 0u, 0u, 0u);
    if (l16 < REP) w = reinterpret_cast<const uint4*>(&q_s[l16 % REP][0])[g * 4 + ks];
    qf[ks] = __builtin_bit_cast(bf16x8, w);
  }

  float m = kDecodeMinM, l = 0.f;              // of head l16, over this lane's keys
  f32x4 acc[8];                                // O^T: dims dt*16 + g*4 + r of head l16
#pragma unroll
  for (int dt = 0; dt < 8; ++dt) acc[dt] = f32x4{0.f, 0.f, 0.f, 0.f};

  // K of tile t: key +16t + l16, 32 bytes at g*32.  V load i: key +8i + kr, 16 bytes.
  // All four from key 0 of the row; PAGED: of the step's page, added per step.
  const uint8_t* kp = k_cache + row_base + (int64_t)l16 * key_stride + g * 32;
  const uint8_t* vp = v_cache + row_base + (int64_t)kr * key_stride + c8 * 16;
  const float* ksp = k_scale + scale_base + l16;
  const float* vsp = v_scale + scale_base + kr;

  char* vst = buf_s + wid * kVStageBytes;      // this wave's staging
  // load i stores chunks 2*c8, 2*c8 + 1 of row 8i + kr: 32 bytes at
  // vstage_off(kr, 2 * c8) = 256 kr + 32 (c8 ^ kr)
  const int vst_wr = vstage_off(kr, 2 * c8);
  const int q4 = (lane >> 2) & 3, p4 = lane & 3;
  // transposed read of tile dt, half h: rows 16h + 4g + q4, dims 16dt + 4p4 ..
  const int vst_rd = vstage_off(4 * g + q4, p4 >> 1) + 8 * (p4 & 1);

  uint4 kraw[2][2], vraw[4];                   // e4m3 as loaded
  float ksc[2], vsc[4];                        // their keys' scales
  bf16x8 kf[2][4];

  auto load_k = [&](int key0) {                // 32 cached keys from key0
    const uint8_t* kq = kp + page_kv(key0);
    const float* ksq = ksp + page_scale(key0);
#pragma unroll
    for (int t = 0; t < 2; ++t) {
      const uint4* src = reinterpret_cast<const uint4*>(kq + (key0 + 16 * t) * key_stride);
      kraw[t][0] = src[0];
      kraw[t][1] = src[1];
      ksc[t] = ksq[key0 + 16 * t];
    }
  };
  auto load_v = [&](int key0) {
    const uint8_t* vq = vp + page_kv(key0);
    const float* vsq = vsp + page_scale(key0);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      vraw[i] = *reinterpret_cast<const uint4*>(vq + (key0 + 8 * i) * key_stride);
      vsc[i] = vsq[key0 + 8 * i];
    }
  };
  auto convert_k = [&]() {
#pragma unroll
    for (int t = 0; t < 2; ++t) {
      kf[t][0] = fp8x8_to_bf16(kraw[t][0].x, kraw[t][0].y, ksc[t]);
      kf[t][1] = fp8x8_to_bf16(kraw[t][0].z, kraw[t][0].w, ksc[t]);
      kf[t][2] = fp8x8_to_bf16(kraw[t][1].x, kraw[t][1].y, ksc[t]);
      kf[t][3] = fp8x8_to_bf16(kraw[t][1].z, kraw[t][1].w, ksc[t]);
    }
  };
  auto stage_row = [&](int i, bf16x8 lo, bf16x8 hi) {
    bf16x8* dst = reinterpret_cast<bf16x8*>(vst + vst_wr + 8 * 256 * i);
    dst[0] = lo;
    dst[1] = hi;
  };
  auto stage_fence = [&]() {
    // the transposed reads below follow these stores in program order
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
  };
  auto stage_v = [&]() {
#pragma unroll
    for (int i = 0; i < 4; ++i)
      stage_row(i, fp8x8_to_bf16(vraw[i].x, vraw[i].y, vsc[i]),
                fp8x8_to_bf16(vraw[i].z, vraw[i].w, vsc[i]));
    stage_fence();
  };
  auto scores = [&](f32x4(&st)[2]) {
#pragma unroll
    for (int t = 0; t < 2; ++t) {
      st[t] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int ks = 0; ks < 4; ++ks)
        st[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(kf[t][ks], qf[ks], st[t], 0, 0, 0);
    }
  };
  // Online-softmax update with the step's scores (st[t][r]: key 16t + 4g + r,
  // -inf where masked), then O^T += V^T P^T from the staged V.
  auto softmax_pv = [&](f32x4(&st)[2]) {
    float mx = fmaxf(fmaxf(fmaxf(st[0][0], st[0][1]), fmaxf(st[0][2], st[0][3])),
                     fmaxf(fmaxf(st[1][0], st[1][1]), fmaxf(st[1][2], st[1][3])));
    mx = max_across_rows(mx);                  // finite: every step holds a valid key
    const float mn = fmaxf(m, mx * c);
    const float al = attn_exp2(m - mn);
    m = mn;
    float pr[2][4], ps = 0.f;
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        pr[t][r] = attn_exp2(fmaf(st[t][r], c, -mn));
        ps += pr[t][r];
      }
    l = l * al + ps;
    const unsigned pw[4] = {cvt_pk_bf16(pr[0][0], pr[0][1]), cvt_pk_bf16(pr[0][2], pr[0][3]),
                            cvt_pk_bf16(pr[1][0], pr[1][1]), cvt_pk_bf16(pr[1][2], pr[1][3])};
    const bf16x8 pf = *reinterpret_cast<const bf16x8*>(pw);
#pragma unroll
    for (int dt = 0; dt < 8; ++dt) {
      const int off = vst_rd ^ (32 * dt);
      const bf16x8 vf = read_tr_frag(vst, off, off + 16 * 256);
      acc[dt] *= al;
      acc[dt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(vf, pf, acc[dt], 0, 0, 0);
    }
    __builtin_amdgcn_wave_barrier();           // the next stage_v stays behind these reads
  };

  // ---- steps of 32 cached keys (< p): no mask, no clamp -----------------------
  int nfull = (p - wave0) / STEP;
  nfull = p <= wave0 ? 0 : (nfull > NSTEP ? NSTEP : nfull);
  if (nfull > 0) {
    load_k(wave0);
    load_v(wave0);
  }
#pragma unroll 1
  for (int s = 0; s < nfull; ++s) {
    const int next = wave0 + (s + 1) * STEP;
    f32x4 st[2];
    stage_v();
    if (s + 1 < nfull) load_v(next);
    convert_k();
    if (s + 1 < nfull) load_k(next);
    scores(st);
    softmax_pv(st);
  }

  // ---- the step that holds key p ---------------------------------------------
  // Wave-uniform condition (ds_read_b64_tr_b16 and MFMA run with EXEC all ones);
  // the loads inside are per lane: cached keys < p with their scales, then the
  // new token's dequantised row from LDS, zeros beyond (their P is 0; staged V
  // has to be finite).
  if (nfull < NSTEP && p >= wave0 && p - wave0 < KPW) {
    const int key0 = wave0 + nfull * STEP;     // key0 <= p < key0 + 32
    const uint8_t* kq = kp + page_kv(key0);
    const uint8_t* vq = vp + page_kv(key0);
    const float* ksq = ksp + page_scale(key0);
    const float* vsq = vsp + page_scale(key0);
#pragma unroll
    for (int t = 0; t < 2; ++t) {
      const int key = key0 + 16 * t + l16;
      kraw[t][0] = kraw[t][1] = make_uint4(0u, 0u, 0u, 0u);
      ksc[t] = 1.f;
      if (key < p) {
        const uint4* src = reinterpret_cast<const uint4*>(kq + (key0 + 16 * t) * key_stride);
        kraw[t][0] = src[0];
        kraw[t][1] = src[1];
        ksc[t] = ksq[key0 + 16 * t];
      }
    }
    convert_k();
#pragma unroll
    for (int t = 0; t < 2; ++t)
      if (key0 + 16 * t + l16 == p) {
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) kf[t][ks] = __builtin_bit_cast(bf16x8, kn_s[g * 4 + ks]);
      }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int key = key0 + 8 * i + kr;
      uint4 w = make_uint4(0u, 0u, 0u, 0u);
      float sc = 1.f;
      if (key < p) {
        w = *reinterpret_cast<const uint4*>(vq + (key0 + 8 * i) * key_stride);
        sc = vsq[key0 + 8 * i];
      }
      bf16x8 lo = fp8x8_to_bf16(w.x, w.y, sc), hi = fp8x8_to_bf16(w.z, w.w, sc);
      if (key == p) {
        lo = __builtin_bit_cast(bf16x8, vn_s[2 * c8]);
        hi = __builtin_bit_cast(bf16x8, vn_s[2 * c8 + 1]);
      }
      stage_row(i, lo, hi);
    }
    stage_fence();
    f32x4 st[2];
    scores(st);
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
      for (int r = 0; r < 4; ++r)
        if (key0 + 16 * t + 4 * g + r > p) st[t][r] = -INFINITY;
    softmax_pv(st);
  }

  // ---- the wave's state -> LDS ------------------------------------------------
  // m is already common to the 4 lane groups and O^T is complete (the MFMA
  // summed over all 32 keys of a step); l is summed over the groups here.
  l = sum_across_rows(l);
  __syncthreads();                             // every wave is done with its staging
  if (l16 < REP) {
    const int h = l16 % REP;
#pragma unroll
    for (int dt = 0; dt < 8; ++dt)
      *reinterpret_cast<float4*>(&st_s[wid][h][dt * 16 + g * 4]) =
          make_float4(acc[dt][0], acc[dt][1], acc[dt][2], acc[dt][3]);
    if (g == 0) {
      st_s[wid][h][ATTN_D] = m;
      st_s[wid][h][ATTN_D + 1] = l;
    }
  }
  __syncthreads();

  // ---- merge the 4 waves, write the chunk's partial ---------------------------
  float* wsn = ws + (((int64_t)n * H + (int64_t)kvh * REP) * J + j) * kDecodeWs;
  for (int idx = tid; idx < REP * (ATTN_D + 1); idx += kDecodeThreads) {
    const int h = idx / (ATTN_D + 1), d = idx % (ATTN_D + 1);
    float mx = st_s[0][h][ATTN_D];
#pragma unroll
    for (int w = 1; w < kDecodeWaves; ++w) mx = fmaxf(mx, st_s[w][h][ATTN_D]);
    // d < 128: acc[d]; d == 128: l (stored one past m)
    const int src = d < ATTN_D ? d : ATTN_D + 1;
    float sum = 0.f;
#pragma unroll
    for (int w = 0; w < kDecodeWaves; ++w)
      sum += st_s[w][h][src] * exp2f(st_s[w][h][ATTN_D] - mx);
    float* dst = wsn + (int64_t)h * J * kDecodeWs;
    dst[src] = sum;
    if (d == ATTN_D) dst[ATTN_D] = mx;
  }
}

template <int REP, int C, bool PAGED>
static void launch_decode_fp8(const at::Tensor& q, const at::Tensor& k_new,
                              const at::Tensor& v_new, at::Tensor& k_cache, at::Tensor& v_cache,
                              at::Tensor& k_scale, at::Tensor& v_scale, const at::Tensor& cos_t,
                              const at::Tensor& sin_t, const int64_t* positions,
                              const int64_t* rows, int64_t* lengths, at::Tensor& o,
                              const DecodeTable& bt, int uniform_pos, int max_len) {
  const int N = q.size(0), H = q.size(2), Hkv = k_new.size(2);
  const int slots = bt.rows, Tmax = k_cache.size(1);
  const int J = (max_len + C - 1) / C;
  auto ws = at::empty({N, H, J, kDecodeWs}, q.options().dtype(at::kFloat));
  hipLaunchKernelGGL((attn_decode_fp8_kernel<REP, C, PAGED>), dim3(J, Hkv, N), dim3(kDecodeThreads), 0,
                     current_stream(), (const __hip_bfloat16*)q.data_ptr(),
                     (const __hip_bfloat16*)k_new.data_ptr(),
                     (const __hip_bfloat16*)v_new.data_ptr(), (uint8_t*)k_cache.data_ptr(),
                     (uint8_t*)v_cache.data_ptr(), k_scale.data_ptr<float>(),
                     v_scale.data_ptr<float>(), cos_t.data_ptr<float>(), sin_t.data_ptr<float>(),
                     positions, rows, lengths, ws.data_ptr<float>(), bt.pt, uniform_pos, max_len,
                     slots, Tmax, Hkv, J, attn_scale().c);
  LPP_CHECK_HIP(hipGetLastError());
  launch_decode_combine<C>(ws, positions, rows, o, uniform_pos, max_len, slots, N, H, J);
}

}  // namespace lpp

// attention_decode over e4m3 caches with per-(slot, kv head, token) scales.
// chunk as for attention_decode; there is one kernel, so no impl.  block_table:
// the paged layout (attn_paged.h), scales [num_pages,Hkv,64].
at::Tensor attention_decode_fp8(at::Tensor q, at::Tensor k_new, at::Tensor v_new,
                                at::Tensor k_cache, at::Tensor v_cache, at::Tensor k_scale,
                                at::Tensor v_scale, at::Tensor cos_t, at::Tensor sin_t,
                                c10::optional<at::Tensor> positions,
                                c10::optional<at::Tensor> rows,
                                c10::optional<at::Tensor> lengths, int64_t uniform_pos,
                                int64_t max_len, int64_t chunk,
                                c10::optional<at::Tensor> block_table) {
  const char* who = "attention_decode_fp8";
  const lpp::DecodeTable bt =
      lpp::decode_check_args(who, q, k_new, v_new, k_cache, v_cache, cos_t, sin_t, positions,
                             rows, lengths, uniform_pos, max_len, &k_scale, &v_scale, block_table);
  auto o = at::empty_like(q);
  if (q.size(0) == 0) return o;
  const int64_t* pp = positions.has_value() ? positions->data_ptr<int64_t>() : nullptr;
  const int64_t* rp = rows.has_value() ? rows->data_ptr<int64_t>() : nullptr;
  int64_t* lp = lengths.has_value() ? lengths->data_ptr<int64_t>() : nullptr;
  const int rep = (int)(q.size(2) / k_new.size(2));
  if (chunk == 0) chunk = lpp::kDecodeChunk;
#define LPP_DECODE_FP8(R, CC)                                                                 \
  if (rep == R && chunk == CC) {                                                              \
    if (bt.pt.table)                                                                          \
      lpp::launch_decode_fp8<R, CC, true>(q, k_new, v_new, k_cache, v_cache, k_scale, v_scale, \
                                          cos_t, sin_t, pp, rp, lp, o, bt, (int)uniform_pos,  \
                                          (int)max_len);                                      \
    else                                                                                      \
      lpp::launch_decode_fp8<R, CC, false>(q, k_new, v_new, k_cache, v_cache, k_scale,        \
                                           v_scale, cos_t, sin_t, pp, rp, lp, o, bt,          \
                                           (int)uniform_pos, (int)max_len);                   \
    return o;                                                                                 \
  }
#define LPP_DECODE_FP8_CHUNKS(R) LPP_DECODE_FP8(R, 128) LPP_DECODE_FP8(R, 256) LPP_DECODE_FP8(R, 512)
  LPP_DECODE_FP8_CHUNKS(1)
  LPP_DECODE_FP8_CHUNKS(2)
  LPP_DECODE_FP8_CHUNKS(4)
  LPP_DECODE_FP8_CHUNKS(8)
  LPP_DECODE_FP8_CHUNKS(16)
#undef LPP_DECODE_FP8_CHUNKS
#undef LPP_DECODE_FP8
  TORCH_CHECK(false, who, ": H/Hkv must be 1, 2, 4, 8 or 16 and chunk 0, 128, 256 or 512, got ",
              rep, ", ", chunk);
}
