// Flash-style causal attention FORWARD for gfx950 (CDNA4), bf16, D=128.
//
// Replaces the materialised-mask eager attention the reference is stuck
// with (README.md:141-143: flash attention "did not work" under DS-PP;
// the [B,1,S,S] fp16 mask is built host-side, data/flan.py:194-243).
// The causal mask is implicit — nothing S^2-shaped ever exists.
//
// Structure = the CDNA4 guide's 8-wave 32x32 ladder (plain HIP):
//   - workgroup = 8 waves x 32 q rows = 256 q rows; KV tile = 64 rows
//   - SWAPPED QK^T: S^T = mfma_32x32x16(A=K, B=Q), so each lane holds the
//     scores of ONE q row (q = lane&31) in its registers -> the online
//     softmax row-reduce is in-register (fmax chain + one permlane32_swap
//     with the partner lane), no ds_bpermute chains
//   - P -> PV A-fragments via v_cvt_pk_bf16_f32 + permlane32_swap pairs
//     (each swap fills two A-frag words for both lane halves uniformly)
//   - K tile [64][128] in LDS, XOR-swizzled ((row&15)<<4) -> the 16-lane
//     ds_read_b128 A-fragment groups are conflict-free
//   - V tile stored TRANSPOSED [128][64] with a ((d>>3)^d)&7 XOR image;
//     the PV B-fragment read is 8 contiguous bf16, ~conflict-free; the
//     transpose itself is done in-register (4x4 dword butterfly across
//     lane quads) so the LDS writes are vectorised b64, ~2-way
//   - double-buffered LDS, one barrier per KV tile; next tile's global
//     loads issued before the compute phase (async-STAGE split)
//   - defer-max online softmax (RESCALE_THRESHOLD=8): the O rescale (and
//     its cross-lane alpha redistribution) runs only when the running max
//     actually grows; decision taken before this tile's P is exponentiated
//     and after the previous tile's PV is complete (the safe order)
//   - O accumulates in the standard C layout (rows in regs); the final
//     1/l (and any alpha) is redistributed reg-row-wise via ds_bpermute
//   - outputs: O bf16 and LSE2[B,H,S] fp32 (base-2 logsumexp of the
//     scaled scores; consumed by the backward kernels)
#include "common.h"
#include "attn_order.h"

namespace lpp {

typedef __attribute__((ext_vector_type(8))) short bf16x8;
typedef __attribute__((ext_vector_type(16))) float f32x16;
typedef __attribute__((ext_vector_type(2))) int int2v;

constexpr int AF_D = 128;      // head dim
constexpr int AF_QW = 32;      // q rows per wave
constexpr int AF_WAVES = 8;
constexpr int AF_QB = AF_QW * AF_WAVES;  // 256 q rows per workgroup
constexpr int AF_KVB = 64;     // kv tile rows
constexpr float AF_THR = 8.0f; // defer-max threshold (exp2 domain)

// K image: [64][128] bf16, row stride 256 B, XOR-swizzled byte offset.
__device__ __forceinline__ int kswz(int row, int col_elem) {
  return row * 256 + ((col_elem * 2) ^ ((row & 15) << 4));
}
// Vt image: [128 d][64 kv] bf16; kv index XORed by ((d>>3)^d)&7 blocks of 8.
__device__ __forceinline__ int vswz(int d, int kv) {
  return (d * 64 + (kv ^ ((((d >> 3) ^ d) & 7) << 3))) * 2;
}

__device__ __forceinline__ unsigned cvt_pk_bf16(float lo, float hi) {
  unsigned r;
  asm("v_cvt_pk_bf16_f32 %0, %1, %2" : "=v"(r) : "v"(lo), "v"(hi));
  return r;
}
__device__ __forceinline__ float as_f(int v) { return __int_as_float(v); }
__device__ __forceinline__ int as_i(float v) { return __float_as_int(v); }

// 2 waves/SIMD = one 512-thread workgroup per CU; 256 VGPRs
__global__ __launch_bounds__(512, 2) void attn_fwd_kernel(
    const short* __restrict__ Q, const short* __restrict__ K,
    const short* __restrict__ V, short* __restrict__ O, float* __restrict__ LSE2,
    int B, int S, int H, int HKV, float c /* scale*log2e */,
    int order_mode, int order_G) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  // buffer layout: K0 @0, K1 @16K, Vt0 @32K, Vt1 @48K
  auto k_lds = [&](int buf) -> char* { return smem + buf * 16384; };
  auto vt_lds = [&](int buf) -> char* { return smem + 32768 + buf * 16384; };

  const int tid = threadIdx.x;
  const int wid = tid >> 6;
  const int lane = tid & 63;
  const int lq = lane & 31;        // this lane's q row (within the wave)
  const int hi2 = lane >> 5;

  const AttnBlock ob = attn_block_order(blockIdx.x, (S + AF_QB - 1) / AF_QB, B * H,
                                        order_G, ATTN_ORDER_FWD_DQ, order_mode);
  const int qblk = ob.blk;
  const int bh = ob.head;
  const int b = bh / H;
  const int h = bh % H;
  const int hkv = h / (H / HKV);

  const int64_t sHD = (int64_t)H * AF_D;
  const int64_t sHkvD = (int64_t)HKV * AF_D;
  const int64_t q_base = (((int64_t)b * S) * H + h) * AF_D;
  const int64_t kv_base = (((int64_t)b * S) * HKV + hkv) * AF_D;

  const int qw0 = qblk * AF_QB + wid * AF_QW;  // this wave's first q row
  const int qrow = qw0 + lq;                   // this lane's q row

  // ---- Q B-fragments: qf[dc] = Q[qrow][dc*16 + hi2*8 .. +8] ----
  bf16x8 qf[8];
  {
    const int64_t rb = q_base + (int64_t)min(qrow, S - 1) * sHD;
#pragma unroll
    for (int dc = 0; dc < 8; ++dc)
      qf[dc] = *reinterpret_cast<const bf16x8*>(&Q[rb + dc * 16 + hi2 * 8]);
  }

  // ---- staging helpers (per thread: one K row-slice + one V row-slice) ----
  // slot: row r = 4*wid + 32*pass, col c = 8*(lane&15) .. but giving each
  // lane-quad {l, l+16, l+32, l+48} rows r..r+3 at one col for the V
  // transpose butterfly: r = 4*wid + (lane>>4), c = 8*(lane&15).
  const int st_r = (lane >> 4);            // 0..3 within the wave's 4 rows
  const int st_c = 8 * (lane & 15);        // 0..120

  const int kv_end = min(S, (qblk + 1) * AF_QB);

  // global row for (pass, tile kv0): kv0 + 4*wid + 32*pass + st_r
  auto ld_tile = [&](int kv0, int pass, bf16x8& kreg, bf16x8& vreg) {
    const int row = min(kv0 + 4 * wid + 32 * pass + st_r, S - 1);
    const int64_t rb = kv_base + (int64_t)row * sHkvD + st_c;
    kreg = *reinterpret_cast<const bf16x8*>(&K[rb]);
    vreg = *reinterpret_cast<const bf16x8*>(&V[rb]);
  };

  auto write_tile = [&](int buf, int pass, bf16x8 kreg, bf16x8 vreg) {
    const int r = 4 * wid + 32 * pass + st_r;  // row within [0,64)
    // K: vectorised swizzled b128 write (conflict-free: 16 slots per row)
    *reinterpret_cast<bf16x8*>(k_lds(buf) + kswz(r, st_c)) = kreg;
    // V: 4x4 dword butterfly across the lane quad {lane^16, lane^32}:
    // lane p=st_r ends with dword p of each quad row = V[r0..r3][c+2p, c+2p+1]
    int dw[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) dw[k] = reinterpret_cast<const int*>(&vreg)[k];
    // bit0 of dword index <-> bit0 of quad pos (xor 16)
    {
      int t0 = __shfl_xor(dw[(st_r & 1) ^ 1], 16);
      int t1 = __shfl_xor(dw[((st_r & 1) ^ 1) | 2], 16);
      if (st_r & 1) { dw[0] = t0; dw[2] = t1; } else { dw[1] = t0; dw[3] = t1; }
    }
    // bit1 of dword index <-> bit1 of quad pos (xor 32)
    {
      int lo = (st_r & 2) ? 0 : 2, hi = lo + 1;
      int t0 = __shfl_xor(dw[lo], 32);
      int t1 = __shfl_xor(dw[hi], 32);
      dw[lo] = t0; dw[hi] = t1;
    }
    // dw[i] now = dword st_r of quad row i = V[row_base+i][c+2*st_r, c+2*st_r+1]
    // byte-transpose 4x(2 bf16) -> 2 columns x 4 rows, then 2x ds_write_b64
    const int r0 = 4 * wid + 32 * pass;  // quad's first kv row
    const int d0 = st_c + 2 * st_r;
#pragma unroll
    for (int e = 0; e < 2; ++e) {
      const int d = d0 + e;
      // column e: bf16 of rows 0..3 = half e of dw[0..3]
      unsigned w01 = e ? (((unsigned)dw[0] >> 16) | ((unsigned)dw[1] & 0xffff0000u))
                       : (((unsigned)dw[0] & 0xffffu) | ((unsigned)dw[1] << 16));
      unsigned w23 = e ? (((unsigned)dw[2] >> 16) | ((unsigned)dw[3] & 0xffff0000u))
                       : (((unsigned)dw[2] & 0xffffu) | ((unsigned)dw[3] << 16));
      int2v pair = {(int)w01, (int)w23};
      *reinterpret_cast<int2v*>(vt_lds(buf) + vswz(d, r0)) = pair;
    }
  };

  // ---- accumulators & softmax state ----
  f32x16 o_acc[4];
#pragma unroll
  for (int dt = 0; dt < 4; ++dt)
#pragma unroll
    for (int r = 0; r < 16; ++r) o_acc[dt][r] = 0.f;
  float m_run = -INFINITY, l_run = 0.f;

  // ---- prologue: stage tile 0; pre-load tile 1 to registers ----
  bf16x8 kreg0, kreg1, vreg0, vreg1;
  ld_tile(0, 0, kreg0, vreg0);
  ld_tile(0, 1, kreg1, vreg1);
  write_tile(0, 0, kreg0, vreg0);
  write_tile(0, 1, kreg1, vreg1);
  if (AF_KVB < kv_end) {
    ld_tile(AF_KVB, 0, kreg0, vreg0);
    ld_tile(AF_KVB, 1, kreg1, vreg1);
  }
  __syncthreads();

  // T14 write-after-barrier: tile t+1 (already in registers) is written
  // right AFTER the barrier — the LDS writes overlap this tile's MFMAs
  // instead of serialising behind them — and tile t+2's loads re-issue
  // immediately into the freed registers, getting the whole compute
  // phase to land (§6 G15; +7-9% over write-before-barrier on the GEMM
  // A/B, the placement this kernel previously used).
  for (int kv0 = 0, cur = 0; kv0 < kv_end; kv0 += AF_KVB, cur ^= 1) {
    const bool have_next = kv0 + AF_KVB < kv_end;
    if (have_next) {
      write_tile(cur ^ 1, 0, kreg0, vreg0);
      write_tile(cur ^ 1, 1, kreg1, vreg1);
      if (kv0 + 2 * AF_KVB < kv_end) {
        ld_tile(kv0 + 2 * AF_KVB, 0, kreg0, vreg0);
        ld_tile(kv0 + 2 * AF_KVB, 1, kreg1, vreg1);
      }
    }

    if (kv0 < qw0 + AF_QW) {  // causal: this wave has work in this tile
      // ---- S^T = K Q^T: two 32x32 tiles over kv ----
      f32x16 st[2];
#pragma unroll
      for (int t2 = 0; t2 < 2; ++t2)
#pragma unroll
        for (int r = 0; r < 16; ++r) st[t2][r] = 0.f;
      __builtin_amdgcn_s_setprio(1);  // favour the MFMA cluster (guide T5)
#pragma unroll
      for (int dc = 0; dc < 8; ++dc) {
#pragma unroll
        for (int t2 = 0; t2 < 2; ++t2) {
          const bf16x8 kf = *reinterpret_cast<const bf16x8*>(
              k_lds(cur) + kswz(t2 * 32 + lq, dc * 16 + hi2 * 8));
          st[t2] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(kf, qf[dc], st[t2], 0, 0, 0);
        }
      }
      __builtin_amdgcn_s_setprio(0);

      // ---- causal / tail mask -> ms (unscaled scores, -inf where masked) ----
      // lane's q row = qrow; score reg r of tile t2 is kv
      //   kv0 + t2*32 + (r&3) + 8*(r>>2) + 4*hi2
      float ms[32];
      const bool need_mask = (kv0 + AF_KVB > qw0) || (kv0 + AF_KVB > S);
#pragma unroll
      for (int t2 = 0; t2 < 2; ++t2)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          float v = st[t2][r];
          if (need_mask) {
            const int kv = kv0 + t2 * 32 + (r & 3) + 8 * (r >> 2) + 4 * hi2;
            if (kv > qrow || kv >= S) v = -INFINITY;
          }
          ms[t2 * 16 + r] = v;
        }

      // ---- in-register row max (+ partner half) ----
      float pmax = ms[0];
#pragma unroll
      for (int i = 1; i < 32; ++i) pmax = fmaxf(pmax, ms[i]);
      {
        int2v sw = __builtin_amdgcn_permlane32_swap(as_i(pmax), as_i(pmax), false, false);
        pmax = fmaxf(pmax, as_f(hi2 ? sw[0] : sw[1]));
      }
      const float rm2 = pmax * c;  // scaled-exp2-domain row max

      // ---- defer-max decision (before exponentiation: the safe order) ----
      float m_new = m_run;
      if (__any(rm2 > m_run + AF_THR)) {
        m_new = fmaxf(m_run, rm2);
        const float alpha = (m_run == -INFINITY) ? 0.f : exp2f(m_run - m_new);
        l_run *= alpha;
        // redistribute alpha to the C-layout rows (reg r -> q row crow(r,hi2))
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int src = (r & 3) + 8 * (r >> 2) + 4 * hi2;
          const float ar = as_f(__builtin_amdgcn_ds_bpermute(src * 4, as_i(alpha)));
#pragma unroll
          for (int dt = 0; dt < 4; ++dt) o_acc[dt][r] *= ar;
        }
        m_run = m_new;
      }

      // ---- P = exp2(ms*c - m_new); row sum; pack to PV A-fragments ----
      float p[32];
      float ps = 0.f;
#pragma unroll
      for (int i = 0; i < 32; ++i) {
        p[i] = exp2f(fmaf(ms[i], c, -m_new));
        ps += p[i];
      }
      {
        int2v sw = __builtin_amdgcn_permlane32_swap(as_i(ps), as_i(ps), false, false);
        ps += as_f(hi2 ? sw[0] : sw[1]);
      }
      l_run += ps;

      // pa[ks] (ks = t2*2 + ksl) = A-frag P[q=lq][kv = ks*16 + hi2*8 + j]
      bf16x8 pa[4];
#pragma unroll
      for (int t2 = 0; t2 < 2; ++t2)
#pragma unroll
        for (int ksl = 0; ksl < 2; ++ksl) {
          const float* pr = &p[t2 * 16 + 8 * ksl];
          const unsigned x1 = cvt_pk_bf16(pr[0], pr[1]);
          const unsigned x2 = cvt_pk_bf16(pr[2], pr[3]);
          const unsigned y1 = cvt_pk_bf16(pr[4], pr[5]);
          const unsigned y2 = cvt_pk_bf16(pr[6], pr[7]);
          const int2v a = __builtin_amdgcn_permlane32_swap((int)x1, (int)y1, false, false);
          const int2v bsw = __builtin_amdgcn_permlane32_swap((int)x2, (int)y2, false, false);
          int w[4] = {a[0], bsw[0], a[1], bsw[1]};
          pa[t2 * 2 + ksl] = *reinterpret_cast<const bf16x8*>(w);
        }

      // ---- O += P V  (B-frags from the transposed V image) ----
      __builtin_amdgcn_s_setprio(1);
#pragma unroll
      for (int dt = 0; dt < 4; ++dt) {
        const int d = dt * 32 + lq;
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) {
          const bf16x8 bv = *reinterpret_cast<const bf16x8*>(
              vt_lds(cur) + vswz(d, ks * 16 + hi2 * 8));
          o_acc[dt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(pa[ks], bv, o_acc[dt], 0, 0, 0);
        }
      }
      __builtin_amdgcn_s_setprio(0);
    }

    __syncthreads();  // one barrier per tile
  }

  // ---- epilogue: redistribute 1/l, normalise, store O and LSE2 ----
  const float invl = (l_run > 0.f) ? 1.f / l_run : 0.f;
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int rq = (r & 3) + 8 * (r >> 2) + 4 * hi2;  // q row of reg r
    const float ir = as_f(__builtin_amdgcn_ds_bpermute(rq * 4, as_i(invl)));
    const int row = qw0 + rq;
    if (row >= S) continue;
    const int64_t rb = q_base + (int64_t)row * sHD;
#pragma unroll
    for (int dt = 0; dt < 4; ++dt) {
      __hip_bfloat16 hv = __float2bfloat16(o_acc[dt][r] * ir);
      O[rb + dt * 32 + lq] = *reinterpret_cast<short*>(&hv);
    }
  }
  if (hi2 == 0 && qrow < S)
    LSE2[((int64_t)b * H + h) * S + qrow] = m_run + log2f(l_run);
}

// ---- block-order state and launch -------------------------------------------
static int g_order_mode = [] {
  const char* e = getenv("LPP_ATTN_ORDER");
  return (e && e[0] == '0') ? 0 : 1;
}();

int attn_order_mode() { return g_order_mode; }

// order_G <= 0: heads per group = ATTN_GROUP_WAVES resident waves of
// workgroups per XCD (32 CUs x one workgroup per CU: 231 VGPRs, 2 waves/SIMD)
// over nblk; the factor is the G sweep's winner (attn_order.h).
void launch_attn_fwd(const at::Tensor& q, const at::Tensor& k, const at::Tensor& v,
                     at::Tensor& o, at::Tensor& lse2, int order_mode, int order_G) {
  const int B = q.size(0), S = q.size(1), H = q.size(2);
  const int HKV = k.size(2);
  const float scale = 1.0f / std::sqrt((float)AF_D);
  const float c = scale * 1.4426950408889634f;  // log2(e)
  const int qblocks = (S + AF_QB - 1) / AF_QB;
  if (order_G <= 0)
    order_G = attn_order_group(ATTN_GROUP_WAVES * ATTN_RESIDENT_PER_XCD, qblocks);
  const size_t lds = 65536;
  hipLaunchKernelGGL(attn_fwd_kernel, dim3(qblocks * B * H), dim3(512), lds,
                     current_stream(), (const short*)q.data_ptr(),
                     (const short*)k.data_ptr(), (const short*)v.data_ptr(),
                     (short*)o.data_ptr(), lse2.data_ptr<float>(), B, S, H, HKV, c,
                     order_mode, order_G);
  LPP_CHECK_HIP(hipGetLastError());
}

}  // namespace lpp

std::vector<at::Tensor> attention_fwd(at::Tensor q, at::Tensor k, at::Tensor v) {
  TORCH_CHECK(q.is_cuda() && q.scalar_type() == at::kBFloat16, "attention_fwd: bf16 only");
  TORCH_CHECK(q.dim() == 4 && q.size(3) == lpp::AF_D, "attention_fwd: [B,S,H,128] required");
  TORCH_CHECK(q.is_contiguous() && k.is_contiguous() && v.is_contiguous());
  const int B = q.size(0), S = q.size(1), H = q.size(2);
  const int HKV = k.size(2);
  TORCH_CHECK(H % HKV == 0);
  auto o = at::empty_like(q);
  auto lse2 = at::empty({B, H, S}, q.options().dtype(at::kFloat));
  lpp::launch_attn_fwd(q, k, v, o, lse2,
                       lpp::attn_order_mode() ? lpp::ATTN_MODE1_FWD : 0, 0);
  return {o, lse2};
}

void attention_set_block_order(int64_t mode) {
  TORCH_CHECK(mode == 0 || mode == 1, "attention_set_block_order: mode 0 or 1");
  lpp::g_order_mode = (int)mode;
}

int64_t attention_get_block_order() { return lpp::g_order_mode; }

// Host only: the (blk, head) pairs of L = 0..n-1 from the header function the
// kernels run.  kind 0 = fwd/dQ, 1 = dK/dV.
at::Tensor attention_block_order(int64_t kind, int64_t nblk, int64_t nheads, int64_t G,
                                 int64_t mode) {
  TORCH_CHECK(kind == 0 || kind == 1, "attention_block_order: kind 0 (fwd/dQ) or 1 (dK/dV)");
  TORCH_CHECK(mode == 0 || mode == 1, "attention_block_order: mode 0 or 1");
  TORCH_CHECK(nblk >= 1 && nheads >= 1 && nblk * nheads < (int64_t)1 << 30 && G >= 1);
  G = std::min(G, nheads);
  const int n = (int)(nblk * nheads);
  auto out = at::empty({n, 2}, at::TensorOptions().dtype(at::kInt));
  int* p = out.data_ptr<int>();
  for (int L = 0; L < n; ++L) {
    const lpp::AttnBlock ob =
        lpp::attn_block_order(L, (int)nblk, (int)nheads, (int)G, (int)kind, (int)mode);
    p[2 * L] = ob.blk;
    p[2 * L + 1] = ob.head;
  }
  return out;
}
