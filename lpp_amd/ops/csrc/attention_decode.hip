// Fused single-token decode attention over the ragged KV cache (gfx950).
//
// One launch per layer-step does, for batch row n at cache row r = rows[n] and
// position p = positions[n]: RoPE of q[n] and k_new[n] at p, the cache write
// k_cache[r,p] / v_cache[r,p] (and lengths[r] = p + 1), and attention of the
// rotated q over keys 0..p of row r.  A second small kernel combines the
// per-chunk partials.
//
// Decomposition: grid (ceil(max_len/C), Hkv, N), 256 threads.  A workgroup owns
// keys [jC, (j+1)C) of one (row, kv head) and serves all REP = H/Hkv query
// heads of it, so every K/V byte is read once.  Wave w owns C/4 consecutive
// keys and walks them in steps of 16 (8 at REP = 8): one 16-byte load per lane
// fetches 8 dims of one key (lane = 16*key + dim-octet), so a wave instruction
// moves 4 whole key rows.  K/V go straight to VGPRs (memory-bound GEMV, M <= 8:
// an LDS round trip is pure overhead); the next step's loads are issued before
// the current step is consumed.  LDS holds only the rotated q, the rotated new
// token and the 4-wave reduce.
//
// Every 16-lane group runs its own online softmax (exp2 domain) over the keys
// it sees; the groups of a wave merge by shuffles, the 4 waves through LDS and
// the chunks in the combine kernel, each in a fixed order.  A row's result
// therefore depends on that row's data and p alone - not on N, on the other
// rows, on the row order or on max_len.
//
// No workgroup reads a cache element written in this launch: positions >= p
// of a row are never addressed (those > p hold stale data of earlier
// requests), and the workgroup whose chunk holds p takes the new token from
// the inputs.  That workgroup is also the one that stores it.
#include "attention.h"
#include "common.h"

namespace lpp {

constexpr int kDecodeChunk = 256;   // C: keys per workgroup (profiles/README.md, Round 6)
constexpr int kDecodeThreads = 256;
constexpr int kDecodeWaves = kDecodeThreads / kWave;
constexpr int kDecodeWs = ATTN_D + 4;  // fp32 partial: acc[128], m, l, pad to 16 B
constexpr float kDecodeMinM = -1e30f;  // running max of an empty state (finite: no inf - inf)

typedef __attribute__((__vector_size__(2 * sizeof(__bf16)))) __bf16 bf16x2_t;

__device__ __forceinline__ float dot2_bf16(uint32_t a, uint32_t b, float c) {
#if __has_builtin(__builtin_amdgcn_fdot2_f32_bf16)
  return __builtin_amdgcn_fdot2_f32_bf16(__builtin_bit_cast(bf16x2_t, a),
                                         __builtin_bit_cast(bf16x2_t, b), c, false);
#else
  c = fmaf(__uint_as_float(a << 16), __uint_as_float(b << 16), c);
  return fmaf(__uint_as_float(a & 0xffff0000u), __uint_as_float(b & 0xffff0000u), c);
#endif
}

// Sum over the 16 lanes of a DPP row, result in every lane: lane^1 and lane^2
// by quad permutes, then the mirrored half row and the mirrored row (after the
// quad steps every lane of a quad, then of a half row, holds the same value).
// DPP rides on the add; __shfl_xor would go through the LDS crossbar.
template <int CTRL>
__device__ __forceinline__ float dpp_add(float x) {
  const int y = __builtin_amdgcn_update_dpp(0, __float_as_int(x), CTRL, 0xf, 0xf, true);
  return x + __int_as_float(y);
}
__device__ __forceinline__ float row16_sum(float x) {
  x = dpp_add<0xB1>(x);   // quad_perm [1,0,3,2]
  x = dpp_add<0x4E>(x);   // quad_perm [2,3,0,1]
  x = dpp_add<0x141>(x);  // row_half_mirror
  return dpp_add<0x140>(x);  // row_mirror
}

__device__ __forceinline__ uint32_t bf16_bits(float x) {
  return (uint32_t)__builtin_bit_cast(unsigned short, __float2bfloat16(x));
}

// Row metadata shared by both kernels.  A row whose cache row or position is
// out of range is skipped (nothing read, nothing written, o = 0).
struct DecodeRow {
  int64_t r;
  int p;
  bool ok;
};
__device__ __forceinline__ DecodeRow decode_row(const int64_t* positions, const int64_t* rows,
                                                int n, int uniform_pos, int slots,
                                                int max_len) {
  const int64_t p = positions ? positions[n] : (int64_t)uniform_pos;
  const int64_t r = rows ? rows[n] : (int64_t)n;
  DecodeRow d;
  d.ok = r >= 0 && r < slots && p >= 0 && p < max_len;
  d.r = r;
  d.p = (int)p;
  return d;
}

template <int REP, int C>
__global__ __launch_bounds__(kDecodeThreads, 2) void attn_decode_kernel(
    const __hip_bfloat16* __restrict__ q,      // [N,1,H,128]
    const __hip_bfloat16* __restrict__ k_new,  // [N,1,Hkv,128]
    const __hip_bfloat16* __restrict__ v_new,  // [N,1,Hkv,128]
    __hip_bfloat16* k_cache,                   // [slots,Tmax,Hkv,128]
    __hip_bfloat16* v_cache,
    const float* __restrict__ cos_t,           // [Smax,64]
    const float* __restrict__ sin_t,
    const int64_t* __restrict__ positions,     // [N] or null
    const int64_t* __restrict__ rows,          // [N] or null
    int64_t* lengths,                          // [slots] or null
    float* __restrict__ ws,                    // [N,H,J,kDecodeWs]
    int uniform_pos, int max_len, int slots, int Tmax, int Hkv, int J, float c) {
  constexpr int KPW = C / kDecodeWaves;        // keys per wave
  // keys per wave step: G loads x 4 key rows; 8 heads leave registers for 2
  constexpr int G = REP >= 8 ? 2 : 4;
  constexpr int STEP = 4 * G;
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
  __shared__ __attribute__((aligned(16))) float st_s[kDecodeWaves][REP][kDecodeWs];

  const int tid = threadIdx.x;
  const int lane = tid & (kWave - 1), wid = tid / kWave;
  const int lg = lane >> 4;                    // key within a 4-key load
  const int dl = lane & 15;                    // dim octet: dims dl*8 .. dl*8+7

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

  // ---- this lane's q: dims dl*8.. of every head, bf16 pairs ------------------
  uint4 qr[REP];
#pragma unroll
  for (int h = 0; h < REP; ++h) qr[h] = reinterpret_cast<const uint4*>(&q_s[h][0])[dl];

  float m[REP], l[REP], acc[REP][8];
#pragma unroll
  for (int h = 0; h < REP; ++h) {
    m[h] = kDecodeMinM;
    l[h] = 0.f;
#pragma unroll
    for (int d = 0; d < 8; ++d) acc[h][d] = 0.f;
  }

  // One online-softmax update of this lane group's state with G keys (8 dims of
  // each in this lane); bias[i] = 0 if key i takes part, -inf if not (an add,
  // so that the row sum above it stays out of divergent control flow).
  auto step = [&](const uint4(&kd)[G], const uint4(&vd)[G], const float(&bias)[G]) {
    float sc[REP][G];
#pragma unroll
    for (int i = 0; i < G; ++i) {
#pragma unroll
      for (int h = 0; h < REP; ++h) {
        float d = dot2_bf16(qr[h].x, kd[i].x, 0.f);
        d = dot2_bf16(qr[h].y, kd[i].y, d);
        d = dot2_bf16(qr[h].z, kd[i].z, d);
        d = dot2_bf16(qr[h].w, kd[i].w, d);
        sc[h][i] = fmaf(row16_sum(d), c, bias[i]);
      }
    }
#pragma unroll
    for (int h = 0; h < REP; ++h) {
      float mx = m[h];
#pragma unroll
      for (int i = 0; i < G; ++i) mx = fmaxf(mx, sc[h][i]);
      const float al = exp2f(m[h] - mx);
      m[h] = mx;
      float ps = 0.f;
#pragma unroll
      for (int i = 0; i < G; ++i) {
        sc[h][i] = exp2f(sc[h][i] - mx);
        ps += sc[h][i];
      }
      l[h] = l[h] * al + ps;
#pragma unroll
      for (int d = 0; d < 8; ++d) acc[h][d] *= al;
    }
#pragma unroll
    for (int i = 0; i < G; ++i) {
      const uint32_t w[4] = {vd[i].x, vd[i].y, vd[i].z, vd[i].w};
      float vf[8];
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        vf[2 * t] = __uint_as_float(w[t] << 16);
        vf[2 * t + 1] = __uint_as_float(w[t] & 0xffff0000u);
      }
#pragma unroll
      for (int h = 0; h < REP; ++h)
#pragma unroll
        for (int d = 0; d < 8; ++d) acc[h][d] = fmaf(sc[h][i], vf[d], acc[h][d]);
    }
  };

  // ---- cached keys: key < p only --------------------------------------------------
  // Positions >= p of the row are never addressed: a load past the last cached
  // key is aimed at key p - 1 instead and its score masked, so the loop has no
  // branch and reads nothing stale and nothing written in this launch.
  const int64_t row_base = ((row.r * Tmax) * (int64_t)Hkv + kvh) * ATTN_D;  // key 0
  const int64_t key_stride = (int64_t)Hkv * ATTN_D;
  const int wave0 = chunk0 + wid * KPW;        // first key of this wave
  int nst = (p - wave0 + STEP - 1) / STEP;     // steps holding a cached key: a prefix
  nst = p <= wave0 ? 0 : (nst > NSTEP ? NSTEP : nst);
  const __hip_bfloat16* kp = k_cache + row_base + dl * 8;
  const __hip_bfloat16* vp = v_cache + row_base + dl * 8;

  uint4 kb[2][G], vb[2][G];
  auto load_step = [&](int s, uint4(&kd)[G], uint4(&vd)[G]) {
#pragma unroll
    for (int i = 0; i < G; ++i) {
      const int key = wave0 + s * STEP + i * 4 + lg;
      const int64_t off = (int64_t)(key < p ? key : p - 1) * key_stride;
      kd[i] = *reinterpret_cast<const uint4*>(kp + off);
      vd[i] = *reinterpret_cast<const uint4*>(vp + off);
    }
  };
  auto cached_step = [&](int s, const uint4(&kd)[G], const uint4(&vd)[G]) {
    float bias[G];
#pragma unroll
    for (int i = 0; i < G; ++i) bias[i] = wave0 + s * STEP + i * 4 + lg < p ? 0.f : -INFINITY;
    step(kd, vd, bias);
  };

  // Two steps per trip so the two register buffers keep static names; not
  // unrolled further, which would only raise the register count.
  if (nst > 0) load_step(0, kb[0], vb[0]);
#pragma unroll 1
  for (int s = 0; s < nst; s += 2) {
    if (s + 1 < nst) load_step(s + 1, kb[1], vb[1]);
    cached_step(s, kb[0], vb[0]);
    if (s + 1 < nst) {
      if (s + 2 < nst) load_step(s + 2, kb[0], vb[0]);
      cached_step(s + 1, kb[1], vb[1]);
    }
  }

  // ---- the new token (key p), from the inputs ------------------------------------
  // One more update in the wave and lane group that own key p.
  if (owner && wid == (p - chunk0) / KPW) {
    float bias[G];
#pragma unroll
    for (int i = 0; i < G; ++i) {
      kb[0][i] = kn_s[dl];
      vb[0][i] = vn_s[dl];
      bias[i] = i == 0 && lg == (p & 3) ? 0.f : -INFINITY;
    }
    step(kb[0], vb[0], bias);
  }

  // ---- cache write: the owner is the one workgroup per (n, kv head) ----------
  if (owner) {
    const int64_t dst = row_base + (int64_t)p * key_stride;
    if (tid < ATTN_D / 8) reinterpret_cast<uint4*>(k_cache + dst)[tid] = kn_s[tid];
    else if (tid < ATTN_D / 4)
      reinterpret_cast<uint4*>(v_cache + dst)[tid - ATTN_D / 8] = vn_s[tid - ATTN_D / 8];
    if (lengths && kvh == 0 && tid == kWave) lengths[row.r] = (int64_t)p + 1;
  }


  // ---- merge the 4 lane groups of the wave (fixed order) ---------------------
#pragma unroll
  for (int h = 0; h < REP; ++h) {
    float mx = fmaxf(m[h], __shfl_xor(m[h], 16, kWave));
    mx = fmaxf(mx, __shfl_xor(mx, 32, kWave));
    const float f = exp2f(m[h] - mx);
    float lv = l[h] * f;
    lv += __shfl_xor(lv, 16, kWave);
    lv += __shfl_xor(lv, 32, kWave);
#pragma unroll
    for (int d = 0; d < 8; ++d) {
      float a = acc[h][d] * f;
      a += __shfl_xor(a, 16, kWave);
      a += __shfl_xor(a, 32, kWave);
      acc[h][d] = a;
    }
    if (lg == 0) {
      float4* dst = reinterpret_cast<float4*>(&st_s[wid][h][dl * 8]);
      dst[0] = make_float4(acc[h][0], acc[h][1], acc[h][2], acc[h][3]);
      dst[1] = make_float4(acc[h][4], acc[h][5], acc[h][6], acc[h][7]);
      if (dl == 0) {
        st_s[wid][h][ATTN_D] = mx;
        st_s[wid][h][ATTN_D + 1] = lv;
      }
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

// o[n,h,:] = sum_j acc_j 2^(m_j - M) / sum_j l_j 2^(m_j - M) over the row's
// ceil((p+1)/C) chunks, in chunk order.  One chunk takes the same path.
template <int C>
__global__ __launch_bounds__(ATTN_D) void attn_decode_combine_kernel(
    const float* __restrict__ ws, const int64_t* __restrict__ positions,
    const int64_t* __restrict__ rows, __hip_bfloat16* __restrict__ o, int uniform_pos,
    int max_len, int slots, int H, int J) {
  const int h = blockIdx.x, n = blockIdx.y, d = threadIdx.x;
  const DecodeRow row = decode_row(positions, rows, n, uniform_pos, slots, max_len);
  __hip_bfloat16* on = o + ((int64_t)n * H + h) * ATTN_D;
  if (!row.ok) {
    on[d] = __float2bfloat16(0.f);
    return;
  }
  const int nj = row.p / C + 1;                // <= J: p < max_len <= J*C
  const float* w = ws + ((int64_t)n * H + h) * J * kDecodeWs;
  float mx = kDecodeMinM, lv = 0.f, a = 0.f;
  for (int jj = 0; jj < nj; ++jj) {
    const float* wj = w + (int64_t)jj * kDecodeWs;
    const float mj = wj[ATTN_D];
    const float mn = fmaxf(mx, mj);
    const float f0 = exp2f(mx - mn), f1 = exp2f(mj - mn);
    a = a * f0 + wj[d] * f1;
    lv = lv * f0 + wj[ATTN_D + 1] * f1;
    mx = mn;
  }
  on[d] = __float2bfloat16(a / lv);
}

template <int REP, int C>
static void launch_decode(const at::Tensor& q, const at::Tensor& k_new, const at::Tensor& v_new,
                          at::Tensor& k_cache, at::Tensor& v_cache, const at::Tensor& cos_t,
                          const at::Tensor& sin_t, const int64_t* positions,
                          const int64_t* rows, int64_t* lengths, at::Tensor& o,
                          int uniform_pos, int max_len) {
  const int N = q.size(0), H = q.size(2), Hkv = k_new.size(2);
  const int slots = k_cache.size(0), Tmax = k_cache.size(1);
  const int J = (max_len + C - 1) / C;
  auto ws = at::empty({N, H, J, kDecodeWs}, q.options().dtype(at::kFloat));
  auto stream = current_stream();
  hipLaunchKernelGGL((attn_decode_kernel<REP, C>), dim3(J, Hkv, N), dim3(kDecodeThreads), 0,
                     stream, (const __hip_bfloat16*)q.data_ptr(),
                     (const __hip_bfloat16*)k_new.data_ptr(),
                     (const __hip_bfloat16*)v_new.data_ptr(),
                     (__hip_bfloat16*)k_cache.data_ptr(), (__hip_bfloat16*)v_cache.data_ptr(),
                     cos_t.data_ptr<float>(), sin_t.data_ptr<float>(), positions, rows,
                     lengths, ws.data_ptr<float>(), uniform_pos, max_len, slots, Tmax, Hkv, J,
                     attn_scale().c);
  LPP_CHECK_HIP(hipGetLastError());
  hipLaunchKernelGGL((attn_decode_combine_kernel<C>), dim3(H, N), dim3(ATTN_D), 0, stream,
                     ws.data_ptr<float>(), positions, rows, (__hip_bfloat16*)o.data_ptr(),
                     uniform_pos, max_len, slots, H, J);
  LPP_CHECK_HIP(hipGetLastError());
}

template <int C>
static void launch_decode_rep(int rep, const at::Tensor& q, const at::Tensor& k_new,
                              const at::Tensor& v_new, at::Tensor& k_cache,
                              at::Tensor& v_cache, const at::Tensor& cos_t,
                              const at::Tensor& sin_t, const int64_t* positions,
                              const int64_t* rows, int64_t* lengths, at::Tensor& o,
                              int uniform_pos, int max_len) {
#define LPP_DECODE_REP(R)                                                                  \
  case R:                                                                                  \
    return launch_decode<R, C>(q, k_new, v_new, k_cache, v_cache, cos_t, sin_t, positions, \
                               rows, lengths, o, uniform_pos, max_len)
  switch (rep) {
    LPP_DECODE_REP(1);
    LPP_DECODE_REP(2);
    LPP_DECODE_REP(4);
    LPP_DECODE_REP(8);
    default:
      TORCH_CHECK(false, "attention_decode: H/Hkv must be 1, 2, 4 or 8, got ", rep);
  }
#undef LPP_DECODE_REP
}

// True when [a, a + na) and [b, b + nb) (bytes) share no address.
static bool disjoint(const void* a, size_t na, const void* b, size_t nb) {
  const char* ca = (const char*)a;
  const char* cb = (const char*)b;
  return ca + na <= cb || cb + nb <= ca;
}

}  // namespace lpp

using lpp::ATTN_D;

int64_t attention_decode_chunk() { return lpp::kDecodeChunk; }

// chunk = 0: the compiled-in C.  128 / 256 / 512 select the other instantiations
// for the chunk-size sweep (scripts/decode_bench.py); results differ in the
// last bits between chunk sizes, never between calls of one size.
at::Tensor attention_decode(at::Tensor q, at::Tensor k_new, at::Tensor v_new,
                            at::Tensor k_cache, at::Tensor v_cache, at::Tensor cos_t,
                            at::Tensor sin_t, c10::optional<at::Tensor> positions,
                            c10::optional<at::Tensor> rows,
                            c10::optional<at::Tensor> lengths, int64_t uniform_pos,
                            int64_t max_len, int64_t chunk) {
  const char* who = "attention_decode";
  TORCH_CHECK(q.is_cuda() && q.scalar_type() == at::kBFloat16, who, ": bf16 CUDA q required");
  TORCH_CHECK(q.dim() == 4 && q.size(1) == 1 && q.size(3) == ATTN_D, who,
              ": q must be [N,1,H,128]");
  const int64_t N = q.size(0), H = q.size(2);
  TORCH_CHECK(k_new.dim() == 4 && k_new.size(0) == N && k_new.size(1) == 1 &&
                  k_new.size(3) == ATTN_D && v_new.sizes() == k_new.sizes(),
              who, ": k_new/v_new must be [N,1,Hkv,128]");
  const int64_t Hkv = k_new.size(2);
  TORCH_CHECK(Hkv >= 1 && H % Hkv == 0, who, ": H must be a multiple of Hkv");
  TORCH_CHECK(k_cache.dim() == 4 && k_cache.size(2) == Hkv && k_cache.size(3) == ATTN_D &&
                  v_cache.sizes() == k_cache.sizes(),
              who, ": caches must be [slots,Tmax,Hkv,128]");
  for (const at::Tensor* t : {&k_new, &v_new, &k_cache, &v_cache})
    TORCH_CHECK(t->is_cuda() && t->scalar_type() == at::kBFloat16 && t->is_contiguous() &&
                    t->device() == q.device(),
                who, ": k/v tensors must be contiguous bf16 on q's device");
  TORCH_CHECK(q.is_contiguous(), who, ": q must be contiguous");
  for (const at::Tensor* t : {&cos_t, &sin_t})
    TORCH_CHECK(t->is_cuda() && t->scalar_type() == at::kFloat && t->is_contiguous() &&
                    t->dim() == 2 && t->size(1) == ATTN_D / 2 && t->device() == q.device(),
                who, ": cos/sin must be contiguous fp32 [Smax,64]");
  TORCH_CHECK(cos_t.size(0) == sin_t.size(0), who, ": cos/sin length mismatch");
  const int64_t slots = k_cache.size(0), Tmax = k_cache.size(1);
  TORCH_CHECK(max_len >= 1 && max_len <= Tmax && max_len <= cos_t.size(0), who,
              ": max_len ", max_len, " must be in [1, min(Tmax, rope table)]");
  TORCH_CHECK(k_cache.numel() < ((int64_t)1 << 40) && N <= 65535 && H <= 65535, who,
              ": shape out of range");  // grid y/z limits; 64-bit offsets beyond

  auto check_index = [&](const c10::optional<at::Tensor>& t, int64_t numel, const char* name) {
    if (!t.has_value()) return;
    TORCH_CHECK(t->is_cuda() && t->device() == q.device() &&
                    t->scalar_type() == at::kLong && t->is_contiguous() && t->dim() == 1 &&
                    t->numel() == numel,
                who, ": ", name, " must be a contiguous int64 [", numel, "] on q's device");
  };
  check_index(positions, N, "positions");
  check_index(rows, N, "rows");
  check_index(lengths, slots, "lengths");
  if (!rows.has_value()) TORCH_CHECK(N <= slots, who, ": N > slots needs rows");
  if (!positions.has_value())
    TORCH_CHECK(uniform_pos >= 0 && uniform_pos < max_len, who, ": uniform_pos out of range");
  if (positions.has_value() && lengths.has_value())
    // other workgroups still read positions after the owner stored lengths[r]
    TORCH_CHECK(lpp::disjoint(positions->data_ptr(), positions->nbytes(),
                              lengths->data_ptr(), lengths->nbytes()),
                who, ": positions must not alias lengths");
  // the inputs are read by workgroups other than the one that writes the cache
  for (const at::Tensor* c : {&k_cache, &v_cache})
    for (const at::Tensor* t : {&q, &k_new, &v_new})
      TORCH_CHECK(lpp::disjoint(c->data_ptr(), c->nbytes(), t->data_ptr(), t->nbytes()), who,
                  ": q/k_new/v_new must not alias the caches");
  TORCH_CHECK(lpp::disjoint(k_cache.data_ptr(), k_cache.nbytes(), v_cache.data_ptr(),
                            v_cache.nbytes()),
              who, ": k_cache and v_cache must not alias");

  auto o = at::empty_like(q);
  if (N == 0) return o;
  const int64_t* pp = positions.has_value() ? positions->data_ptr<int64_t>() : nullptr;
  const int64_t* rp = rows.has_value() ? rows->data_ptr<int64_t>() : nullptr;
  int64_t* lp = lengths.has_value() ? lengths->data_ptr<int64_t>() : nullptr;
  const int rep = (int)(H / Hkv);
  if (chunk == 0) chunk = lpp::kDecodeChunk;
#define LPP_DECODE_CHUNK(CC)                                                             \
  case CC:                                                                               \
    lpp::launch_decode_rep<CC>(rep, q, k_new, v_new, k_cache, v_cache, cos_t, sin_t, pp, \
                               rp, lp, o, (int)uniform_pos, (int)max_len);               \
    break
  switch (chunk) {
    LPP_DECODE_CHUNK(128);
    LPP_DECODE_CHUNK(256);
    LPP_DECODE_CHUNK(512);
    default:
      TORCH_CHECK(false, who, ": chunk must be 0, 128, 256 or 512");
  }
#undef LPP_DECODE_CHUNK
  return o;
}
