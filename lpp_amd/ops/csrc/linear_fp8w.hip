// FP8 weight-only linear (W8A16) for gfx950 (CDNA4): y[M,out] = x[M,in] @
// dequant(wq, scale)^T for M <= 64 tokens, bf16 x and y, fp32 accumulation.
//
// Weight format (attn_fp8.h, no new rule): wq is e4m3 [out,in], scale fp32
// [out,in/128], one power of two per (output row, block of 128 inputs).  byte *
// scale is exact in bf16, so a weight fragment is turned into bf16 in registers
// (fp8x8_to_bf16, the scale folded into the conversion) and the result is a
// bf16 GEMM over the dequantised weight with no rounding of its own.
//
// The kernel is bound by the weight stream: every byte of wq is loaded exactly
// once, 16 bytes per lane and load, straight into MFMA fragments.
//
// MFMA: v_mfma_f32_16x16x32_bf16 with W as A (16 output rows x 32 k) and x^T as
// B (32 k x 16 tokens), so C holds 16 rows x 16 tokens and lane l ends with
// four consecutive output features (l>>4)*4 .. +3 of token l&15.  1 to 4 token
// tiles (template parameter MT) share each converted W fragment.
//
// k permutation.  A step is 64 consecutive k of a 16-row group.  Lane l (row
// l&15, g = l>>4) loads the 16 bytes at k = 64*step + 16*g .. +15 of its row;
// bytes 0..7 are the A fragment of the step's first MFMA and bytes 8..15 of
// its second.  MFMA h of a step therefore contracts, at its own index
// k' = 8*g + j, the real k = 64*step + 16*g + 8*h + j, and the B fragment of
// lane l is the 16 bytes of x[token l&15] at that same k: one ds_read_b128.
//
// Work split.  A workgroup is 4 waves and owns 64 output rows (4 row groups of
// 16; fewer in the last workgroup) and one K-slice of L blocks of 128.  The
// slice is walked in rounds of 4 blocks: the workgroup stages x[0..16*MT) of
// the round's 512 k in LDS once (rows past M are zeros, written to LDS only),
// and wave w takes block w of the round for all four row groups: 4 scale loads
// ahead of 8 dwordx4 loads, 16 * MT MFMAs.  The next round's weights are loaded
// before the current round's MFMAs.  LDS row of a token is 1024 bytes with its
// 16-byte chunk index XORed by token & 15, so the 16 lanes of a B read cover
// all banks once and no row is padded.  MT <= 2 double-buffers the x stage (one
// barrier per round); MT 3 and 4 keep one buffer (two barriers) and stay at
// 64 KB.
//
// Split-K and its order.  A wave sums its blocks in ascending order (step,
// then h, inside a block); the four waves' partial tiles are summed through
// LDS in wave order; with more than one K-slice each workgroup writes its fp32
// tile to a workspace [S,M,out] and linear_fp8w_combine_kernel adds the
// slices in slice order and rounds once.  No atomics, no hand-off between
// workgroups.  The split (lin_split) is a function of (in, out) alone, a C
// column of an MFMA depends on its own B column alone, and MT changes only how
// many columns ride along: row m's output bits are a function of x[m] and the
// weight, not of M or of the other rows.
//
// linear_fp8w_dequant writes the bf16 [out,in] weight (16 bytes in, 32 out per
// item) for the M > 64 path, which stays on hipBLASLt.
#include "attn_fp8.h"

namespace lpp {

constexpr int LF_THREADS = 256;
constexpr int LF_WAVES = 4;
constexpr int LF_RG = 4;                      // row groups of 16 per workgroup
constexpr int LF_ROWS = 16 * LF_RG;
constexpr int LF_BLK = 128;                   // k per scale block
constexpr int LF_ROUND_K = LF_WAVES * LF_BLK;  // k staged per round
constexpr int LF_TOK_BYTES = LF_ROUND_K * 2;  // LDS bytes of one token's round
constexpr int LF_MAX_M = 64;
constexpr int LF_TARGET_WGS = 512;            // about 2048 waves

constexpr int lf_nbuf(int MT) { return MT <= 2 ? 2 : 1; }
// x stage (reused as the 4 waves' fp32 tiles for the reduction, MT * 16 KB)
constexpr int lf_lds_bytes(int MT) { return lf_nbuf(MT) * MT * 16 * LF_TOK_BYTES; }

// K-slices: L blocks each (a multiple of 4, one per wave and round), S of them,
// the last one shorter when L does not divide in/128.  From (in, out) only.
struct LinSplit {
  int L, S;
};
static LinSplit lin_split(int64_t in, int64_t out) {
  const int64_t nb = in / LF_BLK, nrw = (out + LF_ROWS - 1) / LF_ROWS;
  const int64_t s0 = std::max<int64_t>(1, LF_TARGET_WGS / nrw);
  int64_t L = std::max<int64_t>(LF_WAVES, (nb + s0 - 1) / s0);
  L = (L + LF_WAVES - 1) / LF_WAVES * LF_WAVES;
  return {(int)L, (int)((nb + L - 1) / L)};
}

template <int MT>
__global__ __launch_bounds__(LF_THREADS) void linear_fp8w_kernel(
    const short* __restrict__ x,        // [M,in] bf16
    const uint8_t* __restrict__ wq,     // [out,in] e4m3
    const float* __restrict__ scale,    // [out,in/128]
    short* __restrict__ y,              // [M,out] bf16 (S == 1)
    float* __restrict__ ws,             // [S,M,out] fp32 (S > 1)
    int M, int in, int out, int L) {
  extern __shared__ __attribute__((aligned(16))) char lf_smem[];
  constexpr int NBUF = lf_nbuf(MT);
  constexpr int BUF_BYTES = MT * 16 * LF_TOK_BYTES;
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int n16 = lane & 15, g = lane >> 4;
  const int nb = in / LF_BLK;
  const int row0 = blockIdx.x * LF_ROWS;
  const int nrg = min(LF_RG, (out - row0) / 16);   // >= 1
  const int sb = blockIdx.y * L, se = min(sb + L, nb);  // this slice's blocks

  // lane's byte offset into its row of wq and its row of scale, per row group
  const uint8_t* wrow[LF_RG];
  const float* srow[LF_RG];
#pragma unroll
  for (int rg = 0; rg < LF_RG; ++rg) {
    const int64_t r = row0 + 16 * min(rg, nrg - 1) + n16;   // clamped: never past out
    wrow[rg] = wq + r * in + 16 * g;
    srow[rg] = scale + r * nb;
  }

  f32x4 acc[LF_RG][MT];
#pragma unroll
  for (int rg = 0; rg < LF_RG; ++rg)
#pragma unroll
    for (int t = 0; t < MT; ++t) acc[rg][t] = f32x4{0.f, 0.f, 0.f, 0.f};

  // block blk of this wave: the scale ahead of the two 16-byte loads it scales
  auto load_w = [&](int blk, uint4(&w)[LF_RG][2], float(&sc)[LF_RG]) {
    if (blk >= se) return;
#pragma unroll
    for (int rg = 0; rg < LF_RG; ++rg)
      if (rg < nrg) sc[rg] = srow[rg][blk];
#pragma unroll
    for (int rg = 0; rg < LF_RG; ++rg)
      if (rg < nrg) {
        const uint8_t* p = wrow[rg] + (int64_t)blk * LF_BLK;
        w[rg][0] = *reinterpret_cast<const uint4*>(p);
        w[rg][1] = *reinterpret_cast<const uint4*>(p + 64);
      }
  };
  // x[0..16*MT) of k0 .. k0 + 511 into buffer buf; zeros past M and past the slice
  auto stage_x = [&](int buf, int k0) {
    char* xs = lf_smem + buf * BUF_BYTES;
    const int kend = se * LF_BLK;
    for (int i = tid; i < MT * 16 * 64; i += LF_THREADS) {
      const int tok = i >> 6, ch = i & 63, k = k0 + 8 * ch;
      bf16x8 v = {0, 0, 0, 0, 0, 0, 0, 0};
      if (tok < M && k < kend) v = *reinterpret_cast<const bf16x8*>(x + (int64_t)tok * in + k);
      *reinterpret_cast<bf16x8*>(xs + tok * LF_TOK_BYTES + 16 * (ch ^ (tok & 15))) = v;
    }
  };

  uint4 wc[LF_RG][2] = {}, wn[LF_RG][2] = {};
  float sc[LF_RG] = {}, sn[LF_RG] = {};
  load_w(sb + wid, wc, sc);
  int buf = 0;
  for (int b0 = sb; b0 < se; b0 += LF_WAVES) {
    stage_x(buf, b0 * LF_BLK);
    __syncthreads();
    load_w(b0 + LF_WAVES + wid, wn, sn);
    if (b0 + wid < se) {   // wave-uniform
      const char* xs = lf_smem + buf * BUF_BYTES + n16 * LF_TOK_BYTES;
#pragma unroll
      for (int s = 0; s < 2; ++s) {
        bf16x8 bf[MT][2];
#pragma unroll
        for (int t = 0; t < MT; ++t)
#pragma unroll
          for (int h = 0; h < 2; ++h) {
            const int ch = 16 * wid + 8 * s + 2 * g + h;
            bf[t][h] = *reinterpret_cast<const bf16x8*>(xs + t * 16 * LF_TOK_BYTES +
                                                        16 * (ch ^ n16));
          }
#pragma unroll
        for (int rg = 0; rg < LF_RG; ++rg)
          if (rg < nrg) {   // workgroup-uniform
            const bf16x8 a0 = fp8x8_to_bf16(wc[rg][s].x, wc[rg][s].y, sc[rg]);
            const bf16x8 a1 = fp8x8_to_bf16(wc[rg][s].z, wc[rg][s].w, sc[rg]);
#pragma unroll
            for (int t = 0; t < MT; ++t) {
              acc[rg][t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a0, bf[t][0], acc[rg][t], 0, 0, 0);
              acc[rg][t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a1, bf[t][1], acc[rg][t], 0, 0, 0);
            }
          }
      }
    }
#pragma unroll
    for (int rg = 0; rg < LF_RG; ++rg) {
      wc[rg][0] = wn[rg][0];
      wc[rg][1] = wn[rg][1];
      sc[rg] = sn[rg];
    }
    if (NBUF == 2) buf ^= 1; else __syncthreads();
  }

  // ---- the four waves' tiles, summed in wave order ------------------------------
  __syncthreads();
  f32x4* red = reinterpret_cast<f32x4*>(lf_smem);   // [wave][rg][t][lane]
#pragma unroll
  for (int rg = 0; rg < LF_RG; ++rg)
#pragma unroll
    for (int t = 0; t < MT; ++t) red[((wid * LF_RG + rg) * MT + t) * 64 + lane] = acc[rg][t];
  __syncthreads();
  constexpr int ITEMS = LF_RG * MT * 64;
  for (int i = tid; i < nrg * MT * 64; i += LF_THREADS) {
    f32x4 v = red[i];
#pragma unroll
    for (int w = 1; w < LF_WAVES; ++w) v += red[w * ITEMS + i];
    const int l = i & 63, t = (i >> 6) % MT, rg = (i >> 6) / MT;
    const int tok = 16 * t + (l & 15);
    if (tok >= M) continue;
    const int64_t o = (int64_t)tok * out + row0 + 16 * rg + 4 * (l >> 4);
    if (ws) {
      *reinterpret_cast<f32x4*>(ws + (int64_t)blockIdx.y * M * out + o) = v;
    } else {
      uint2 pk = {cvt_pk_bf16(v[0], v[1]), cvt_pk_bf16(v[2], v[3])};
      *reinterpret_cast<uint2*>(y + o) = pk;
    }
  }
}

// y = bf16(sum over slices, in slice order); n4 = M * out / 4 items of 4 floats
__global__ __launch_bounds__(256) void linear_fp8w_combine_kernel(
    const float* __restrict__ ws, short* __restrict__ y, int64_t n4, int S) {
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += (int64_t)gridDim.x * 256) {
    f32x4 v = reinterpret_cast<const f32x4*>(ws)[i];
    for (int s = 1; s < S; ++s) v += reinterpret_cast<const f32x4*>(ws)[s * n4 + i];
    uint2 pk = {cvt_pk_bf16(v[0], v[1]), cvt_pk_bf16(v[2], v[3])};
    reinterpret_cast<uint2*>(y)[i] = pk;
  }
}

// w[out,in] bf16 = byte * scale; an item is 16 bytes of a row (never across a
// block: 128 % 16 == 0), n16 = out * in / 16 items
__global__ __launch_bounds__(256) void linear_fp8w_dequant_kernel(
    const uint8_t* __restrict__ wq, const float* __restrict__ scale, short* __restrict__ w,
    int64_t n16, int in) {
  const int per_row = in / 16, nb = in / LF_BLK;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n16; i += (int64_t)gridDim.x * 256) {
    const int64_t r = i / per_row;
    const int c = (int)(i - r * per_row);
    const float sc = scale[r * nb + c / 8];
    const uint4 b = reinterpret_cast<const uint4*>(wq)[i];
    bf16x8* dst = reinterpret_cast<bf16x8*>(w) + 2 * i;
    dst[0] = fp8x8_to_bf16(b.x, b.y, sc);
    dst[1] = fp8x8_to_bf16(b.z, b.w, sc);
  }
}

// gfx950 (hipcc -O3), linear_fp8w_kernel<MT> for MT = 1 / 2 / 3 / 4: NumVgprs
// 134 / 126 / 132 / 142 plus 16 / 32 / 48 / 64 AGPRs (the accumulators), 3 / 3 /
// 2 / 2 waves per SIMD, ScratchSize 0 everywhere, dynamic LDS 32 / 64 / 48 /
// 64 KB (no static LDS).  combine 12 VGPRs, dequant 20, neither uses LDS or
// scratch.
template <int MT>
static void launch_linear(const at::Tensor& x, const at::Tensor& wq, const at::Tensor& scale,
                          at::Tensor& y, float* ws, const LinSplit& sp) {
  const int M = x.size(0), in = x.size(1), out = wq.size(0);
  hipLaunchKernelGGL((linear_fp8w_kernel<MT>), dim3((out + LF_ROWS - 1) / LF_ROWS, sp.S),
                     dim3(LF_THREADS), lf_lds_bytes(MT), current_stream(),
                     (const short*)x.data_ptr(), (const uint8_t*)wq.data_ptr(),
                     scale.data_ptr<float>(), (short*)y.data_ptr(), ws, M, in, out, sp.L);
  LPP_CHECK_HIP(hipGetLastError());
}

static bool lin_disjoint(const at::Tensor& a, const at::Tensor& b) {
  const char* ca = (const char*)a.data_ptr();
  const char* cb = (const char*)b.data_ptr();
  return ca + a.nbytes() <= cb || cb + b.nbytes() <= ca;
}

// The checks the two entry points share: the quantised weight and its scales.
static void check_weight(const char* who, const at::Tensor& wq, const at::Tensor& scale) {
  TORCH_CHECK(wq.is_cuda() && wq.scalar_type() == at::kFloat8_e4m3fn && wq.dim() == 2 &&
                  wq.is_contiguous(),
              who, ": wq must be a contiguous float8_e4m3fn CUDA tensor [out,in]");
  const int64_t out = wq.size(0), in = wq.size(1);
  TORCH_CHECK(in >= LF_BLK && in % LF_BLK == 0, who, ": in must be a multiple of 128, got ", in);
  TORCH_CHECK(out >= 16 && out % 16 == 0, who, ": out must be a multiple of 16, got ", out);
  TORCH_CHECK(scale.is_cuda() && scale.device() == wq.device() &&
                  scale.scalar_type() == at::kFloat && scale.is_contiguous(),
              who, ": scale must be a contiguous fp32 tensor on wq's device");
  TORCH_CHECK(scale.dim() == 2 && scale.size(0) == out && scale.size(1) == in / LF_BLK, who,
              ": scale must be [out, in/128] = [", out, ", ", in / LF_BLK, "], got ",
              scale.sizes());
  TORCH_CHECK(wq.numel() < ((int64_t)1 << 40) && out < ((int64_t)1 << 31) - LF_ROWS &&
                  in < ((int64_t)1 << 31),
              who, ": weight too large");
  TORCH_CHECK(lin_disjoint(wq, scale), who, ": wq and scale overlap");
}

}  // namespace lpp

at::Tensor linear_fp8w(at::Tensor x, at::Tensor wq, at::Tensor scale) {
  const char* who = "linear_fp8w";
  lpp::check_weight(who, wq, scale);
  const int64_t out = wq.size(0), in = wq.size(1);
  TORCH_CHECK(x.is_cuda() && x.device() == wq.device() && x.scalar_type() == at::kBFloat16, who,
              ": x must be a bf16 tensor on wq's device");
  TORCH_CHECK(x.dim() == 2 && x.size(1) == in, who, ": x must be [M, in] = [M, ", in, "], got ",
              x.sizes());
  TORCH_CHECK(x.is_contiguous(), who, ": x must be contiguous");
  const int64_t M = x.size(0);
  TORCH_CHECK(M >= 1 && M <= lpp::LF_MAX_M, who, ": M must be 1 .. ", lpp::LF_MAX_M, ", got ", M);
  TORCH_CHECK(lpp::lin_disjoint(x, wq) && lpp::lin_disjoint(x, scale), who,
              ": x overlaps the weight");
  const lpp::LinSplit sp = lpp::lin_split(in, out);
  TORCH_CHECK(sp.S <= 65535, who, ": too many K-slices");
  auto y = at::empty({M, out}, x.options());
  at::Tensor ws;
  if (sp.S > 1) ws = at::empty({(int64_t)sp.S, M, out}, x.options().dtype(at::kFloat));
  float* wsp = sp.S > 1 ? ws.data_ptr<float>() : nullptr;
  switch ((M + 15) / 16) {
    case 1: lpp::launch_linear<1>(x, wq, scale, y, wsp, sp); break;
    case 2: lpp::launch_linear<2>(x, wq, scale, y, wsp, sp); break;
    case 3: lpp::launch_linear<3>(x, wq, scale, y, wsp, sp); break;
    default: lpp::launch_linear<4>(x, wq, scale, y, wsp, sp); break;
  }
  if (sp.S > 1) {
    const int64_t n4 = M * out / 4;
    hipLaunchKernelGGL(lpp::linear_fp8w_combine_kernel, dim3(lpp::grid_for(n4, 256)), dim3(256),
                       0, lpp::current_stream(), wsp, (short*)y.data_ptr(), n4, sp.S);
    LPP_CHECK_HIP(hipGetLastError());
  }
  return y;
}

at::Tensor linear_fp8w_dequant(at::Tensor wq, at::Tensor scale) {
  lpp::check_weight("linear_fp8w_dequant", wq, scale);
  auto w = at::empty(wq.sizes(), wq.options().dtype(at::kBFloat16));
  const int64_t n16 = wq.numel() / 16;
  hipLaunchKernelGGL(lpp::linear_fp8w_dequant_kernel, dim3(lpp::grid_for(n16, 256)), dim3(256), 0,
                     lpp::current_stream(), (const uint8_t*)wq.data_ptr(),
                     scale.data_ptr<float>(), (short*)w.data_ptr(), n16, (int)wq.size(1));
  LPP_CHECK_HIP(hipGetLastError());
  return w;
}
