// Single-token decode attention over the ragged KV cache for GQA groups of 8
// and 16 query heads: the MFMA variant of attention_decode.hip (gfx950).
//
// Same contract, same decomposition and the same workspace as the vector-ALU
// kernel: grid (ceil(max_len/C), Hkv, N), 256 threads; a workgroup owns keys
// [jC, (j+1)C) of one (row, kv head), serves all REP heads of it and writes one
// unnormalised fp32 partial per head, which attn_decode_combine_kernel
// (attention_decode.h) finishes.  Wave w owns C/4 consecutive keys and walks
// them in steps of 32.  What differs is where the products run: the group's
// heads are the N side of v_mfma_f32_16x16x32_bf16 (columns 8..15 are zero at
// REP = 8), so a step of 32 keys costs 16 MFMAs instead of 32*REP dot products
// and 32*REP*128 FMAs on the vector ALU.
//
// Scores, S^T = K Q^T (two 16-key tiles per step, 4 k-steps of 32 dims):
//   A = K   lane l: key l&15 of the tile, dims ks*32 + (l>>4)*8 .. +7 - one
//           16-byte global load straight into the fragment, no LDS.  Over the
//           4 k-steps a lane reads its key's 256-byte row in 64-byte runs.
//   B = Q^T lane l: head l&15, the same dims, from the rotated q in LDS; read
//           once and held for the whole kernel (16 VGPRs).
//   C       lane l: head l&15, keys (l>>4)*4 + r, r = 0..3 of the tile.
// Online softmax (exp2 domain): a lane keeps m and l of its head over the keys
// it sees.  Only the running max is agreed between the four 16-lane groups
// (two permlane swaps per step), because the PV product sums P over the keys of
// all four; l stays a per-lane partial until the epilogue and the rescale
// factor is per lane, no broadcast.
//
// Output, O^T += V^T P^T (8 tiles of 16 dims, one k-step of 32 keys):
//   B = P^T lane l: head l&15, k = (l>>4)*8 + i.  The lane's own 8 scores are
//           that fragment with k <-> key (i>>2)*16 + (l>>4)*4 + (i&3): four
//           v_cvt_pk, no cross-lane movement.
//   A = V^T lane l: dim l&15 of the tile, the same 8 keys.  Memory holds V
//           key-major, so the step's 32 key rows go through LDS: stored as
//           they arrive (one 16-byte chunk per lane and load, four whole key
//           rows per wave load) and read back with ds_read_b64_tr_b16, each
//           16-lane group addressing its own keys (l>>4)*4 + q and 16 + the
//           same.  Chunk c of staged row r sits at chunk c ^ 2(r & 7): the 8
//           rows of a 32-lane half then cover all 64 banks, and a store's 8
//           lanes keep 8 different chunks.
//   C       lane l: head l&15, dims dt*16 + (l>>4)*4 + r: 8 x f32x4.
// The staging is wave-private (8 KB per wave) and single-buffered: a wave's
// LDS accesses complete in order, so the loop has waitcnts and no barrier.
// The next step's V is loaded into the registers the store just freed, the
// next step's K into the fragments once the score MFMAs have consumed them.
//
// Steps whose 32 keys are all cached (< p) run without a mask or a clamp.  The
// one step that holds key p - in one wave of one workgroup per (n, kv head) -
// loads under a per-lane predicate: keys < p from the cache, key p from the
// rotated k_new / v_new in LDS, nothing beyond.  No cache element at a position
// >= p is ever addressed, and the new token is never read back from the cache.
// That workgroup also stores it, and lengths[row] = p + 1.
//
// Every merge order is fixed (lane groups, waves, chunks), so a row's bits
// depend on its own data and p alone.
//
// PAGED (attn_paged.h): a step of 32 keys is half a 64-key page, so its page id
// is wave-uniform.  A wave's C/4 keys are one page, or two at C = 512; both
// ids are fetched by scalar loads before the RoPE prologue, and a step adds
// its page's base (SGPRs) where the slot layout adds the row's.  The fragment
// layouts, the staging, the predicated owner step and every merge order are
// untouched, so paged and slot results are bit-identical.
// gfx950 (hipcc -O3), slot / paged, REP 8 and 16 alike: NumVgprs 124 / 124
// (C = 128, 4 waves/SIMD), 158 / 158 (C = 256, 3), 158 / 154 (C = 512, 3);
// SGPRs 48-64 / 54-71; ScratchSize 0 everywhere.
#include "attention_decode.h"

namespace lpp {

template <int REP, int C, bool PAGED>
__global__ __launch_bounds__(kDecodeThreads, 3) void attn_decode_mfma_kernel(
    const __hip_bfloat16* __restrict__ q,      // [N,1,H,128]
    const __hip_bfloat16* __restrict__ k_new,  // [N,1,Hkv,128]
    const __hip_bfloat16* __restrict__ v_new,  // [N,1,Hkv,128]
    __hip_bfloat16* k_cache,                   // [slots,Tmax,Hkv,128]; PAGED: the pool
    __hip_bfloat16* v_cache,
    const float* __restrict__ cos_t,           // [Smax,64]
    const float* __restrict__ sin_t,
    const int64_t* __restrict__ positions,     // [N] or null
    const int64_t* __restrict__ rows,          // [N] or null
    int64_t* lengths,                          // [slots] or null
    float* __restrict__ ws,                    // [N,H,J,kDecodeWs]
    PageTable pt,                              // PAGED: slots counts the table's rows
    int uniform_pos, int max_len, int slots, int Tmax, int Hkv, int J, float c) {
  static_assert(REP == 8 || REP == 16, "one MFMA tile of heads: 8 (half empty) or 16");
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
  __shared__ uint4 kn_s[ATTN_D / 8];           // rotated k_new, bf16
  __shared__ uint4 vn_s[ATTN_D / 8];
  // V staging of the 4 waves in the loop, the 4-wave merge after it
  __shared__ __attribute__((aligned(16))) char buf_s[decode_mfma_lds<REP>()];
  float(*st_s)[REP][kDecodeWs] = reinterpret_cast<float(*)[REP][kDecodeWs]>(buf_s);

  const int tid = threadIdx.x;
  const int lane = tid & (kWave - 1);
  const int wid = __builtin_amdgcn_readfirstlane(tid / kWave);
  const int l16 = lane & 15;                   // K: key of a tile; Q, S, P, O: head
  const int g = lane >> 4;                     // lane group
  const int wave0 = chunk0 + wid * KPW;        // first key of this wave
  // where this wave's keys live: the row, or its one or two pages
  const DecodeRuns<PAGED, KPW> runs(pt, row.r, Tmax, Hkv, kvh, wave0, p);

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

  // ---- Q^T fragments: head l16 (none at REP = 8, l16 >= 8), dims ks*32 + g*8 ..
  bf16x8 qf[4];
#pragma unroll
  for (int ks = 0; ks < 4; ++ks) {
    uint4 w = make_uint4(0u, 0u, 0u, 0u);
    if (l16 < REP) w = reinterpret_cast<const uint4*>(&q_s[l16 % REP][0])[ks * 4 + g];
    qf[ks] = __builtin_bit_cast(bf16x8, w);
  }

  float m = kDecodeMinM, l = 0.f;              // of head l16, over this lane's keys
  f32x4 acc[8];                                // O^T: dims dt*16 + g*4 + r of head l16
#pragma unroll
  for (int dt = 0; dt < 8; ++dt) acc[dt] = f32x4{0.f, 0.f, 0.f, 0.f};

  const int64_t key_stride = (int64_t)Hkv * ATTN_D;
  // K fragment of (tile t, k-step ks): key +16t, dims +32ks.  V load i: key +4i.
  // Both from key 0 of the row, or of the step's page (runs.at).
  const __hip_bfloat16* kp = k_cache + (int64_t)l16 * key_stride + g * 8;
  const __hip_bfloat16* vp = v_cache + (int64_t)g * key_stride + l16 * 8;

  char* vst = buf_s + wid * kVStageBytes;      // this wave's staging
  // load i stores chunk l16 of row 4i + g = 8(i>>1) + 4(i&1) + g
  const int vst_wr[2] = {vstage_off(g, l16), vstage_off(4 + g, l16)};
  const int q4 = (lane >> 2) & 3, p4 = lane & 3;
  // transposed read of tile dt, half h: rows 16h + 4g + q4, dims 16dt + 4p4 ..
  const int vst_rd = vstage_off(4 * g + q4, p4 >> 1) + 8 * (p4 & 1);

  bf16x8 kf[2][4];
  uint4 vr[8];

  auto load_k = [&](int key0) {                // 32 cached keys from key0
    const __hip_bfloat16* kq = kp + runs.at(key0 - wave0).kv;
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
      for (int ks = 0; ks < 4; ++ks)
        kf[t][ks] = *reinterpret_cast<const bf16x8*>(kq + (key0 + 16 * t) * key_stride + 32 * ks);
  };
  auto load_v = [&](int key0) {
    const __hip_bfloat16* vq = vp + runs.at(key0 - wave0).kv;
#pragma unroll
    for (int i = 0; i < 8; ++i)
      vr[i] = *reinterpret_cast<const uint4*>(vq + (key0 + 4 * i) * key_stride);
  };
  auto stage_v = [&]() {
#pragma unroll
    for (int i = 0; i < 8; ++i)
      *reinterpret_cast<uint4*>(vst + vst_wr[i & 1] + 8 * 256 * (i >> 1)) = vr[i];
    // the transposed reads below follow these stores in program order
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
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
    scores(st);
    if (s + 1 < nfull) load_k(next);
    softmax_pv(st);
  }

  // ---- the step that holds key p ---------------------------------------------
  // Wave-uniform condition (ds_read_b64_tr_b16 and MFMA run with EXEC all ones);
  // the loads inside are per lane: cached keys < p, then the new token from
  // LDS, zeros beyond (their P is 0; staged V has to be finite).
  if (nfull < NSTEP && p >= wave0 && p - wave0 < KPW) {
    const int key0 = wave0 + nfull * STEP;     // key0 <= p < key0 + 32
    const int64_t base = runs.at(key0 - wave0).kv;
#pragma unroll
    for (int t = 0; t < 2; ++t) {
      const int key = key0 + 16 * t + l16;
#pragma unroll
      for (int ks = 0; ks < 4; ++ks) {
        uint4 w = make_uint4(0u, 0u, 0u, 0u);
        if (key < p)
          w = *reinterpret_cast<const uint4*>(kp + base + (key0 + 16 * t) * key_stride + 32 * ks);
        else if (key == p)
          w = kn_s[ks * 4 + g];
        kf[t][ks] = __builtin_bit_cast(bf16x8, w);
      }
    }
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const int key = key0 + 4 * i + g;
      uint4 w = make_uint4(0u, 0u, 0u, 0u);
      if (key < p)
        w = *reinterpret_cast<const uint4*>(vp + base + (key0 + 4 * i) * key_stride);
      else if (key == p)
        w = vn_s[l16];
      vr[i] = w;
    }
    f32x4 st[2];
    stage_v();
    scores(st);
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
      for (int r = 0; r < 4; ++r)
        if (key0 + 16 * t + 4 * g + r > p) st[t][r] = -INFINITY;
    softmax_pv(st);
  }

  // ---- cache write: the owner is the one workgroup per (n, kv head) ----------
  if (owner) {
    const KvRun at_p = kv_run<PAGED>(pt, row.r, Tmax, Hkv, kvh, p);
    const int64_t dst = at_p.kv + (int64_t)p * key_stride;
    if (!at_p.ok) {
      // a table entry outside the pool: the token is not stored
    } else if (tid < ATTN_D / 8) {
      reinterpret_cast<uint4*>(k_cache + dst)[tid] = kn_s[tid];
    } else if (tid < ATTN_D / 4) {
      reinterpret_cast<uint4*>(v_cache + dst)[tid - ATTN_D / 8] = vn_s[tid - ATTN_D / 8];
    }
    if (lengths && kvh == 0 && tid == kWave) lengths[row.r] = (int64_t)p + 1;
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
static void launch_decode_mfma_rc(const at::Tensor& q, const at::Tensor& k_new,
                                  const at::Tensor& v_new, at::Tensor& k_cache,
                                  at::Tensor& v_cache, const at::Tensor& cos_t,
                                  const at::Tensor& sin_t, const int64_t* positions,
                                  const int64_t* rows, int64_t* lengths, at::Tensor& o,
                                  const DecodeTable& bt, int uniform_pos, int max_len) {
  const int N = q.size(0), H = q.size(2), Hkv = k_new.size(2);
  const int slots = bt.rows, Tmax = k_cache.size(1);
  const int J = (max_len + C - 1) / C;
  auto ws = at::empty({N, H, J, kDecodeWs}, q.options().dtype(at::kFloat));
  hipLaunchKernelGGL((attn_decode_mfma_kernel<REP, C, PAGED>), dim3(J, Hkv, N), dim3(kDecodeThreads),
                     0, current_stream(), (const __hip_bfloat16*)q.data_ptr(),
                     (const __hip_bfloat16*)k_new.data_ptr(),
                     (const __hip_bfloat16*)v_new.data_ptr(),
                     (__hip_bfloat16*)k_cache.data_ptr(), (__hip_bfloat16*)v_cache.data_ptr(),
                     cos_t.data_ptr<float>(), sin_t.data_ptr<float>(), positions, rows,
                     lengths, ws.data_ptr<float>(), bt.pt, uniform_pos, max_len, slots, Tmax, Hkv,
                     J, attn_scale().c);
  LPP_CHECK_HIP(hipGetLastError());
  launch_decode_combine<C>(ws, positions, rows, o, uniform_pos, max_len, slots, N, H, J);
}

void launch_decode_mfma(int rep, int chunk, const at::Tensor& q, const at::Tensor& k_new,
                        const at::Tensor& v_new, at::Tensor& k_cache, at::Tensor& v_cache,
                        const at::Tensor& cos_t, const at::Tensor& sin_t,
                        const int64_t* positions, const int64_t* rows, int64_t* lengths,
                        at::Tensor& o, const DecodeTable& bt, int uniform_pos, int max_len) {
#define LPP_DECODE_MFMA(R, CC)                                                               \
  if (rep == R && chunk == CC) {                                                             \
    if (bt.pt.table)                                                                         \
      return launch_decode_mfma_rc<R, CC, true>(q, k_new, v_new, k_cache, v_cache, cos_t,    \
                                                sin_t, positions, rows, lengths, o, bt,      \
                                                uniform_pos, max_len);                       \
    return launch_decode_mfma_rc<R, CC, false>(q, k_new, v_new, k_cache, v_cache, cos_t,     \
                                               sin_t, positions, rows, lengths, o, bt,       \
                                               uniform_pos, max_len);                        \
  }
  LPP_DECODE_MFMA(8, 128);
  LPP_DECODE_MFMA(8, 256);
  LPP_DECODE_MFMA(8, 512);
  LPP_DECODE_MFMA(16, 128);
  LPP_DECODE_MFMA(16, 256);
  LPP_DECODE_MFMA(16, 512);
#undef LPP_DECODE_MFMA
  TORCH_CHECK(false, "attention_decode: no MFMA kernel for H/Hkv ", rep, ", chunk ", chunk);
}

}  // namespace lpp
