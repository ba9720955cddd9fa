// MXFP4 weight-only linear (W4A16) for gfx950 (CDNA4): y[M,out] = x[M,in] @
// dequant(wq, scale)^T for M <= 64 tokens, bf16 x and y, fp32 accumulation.
//
// Weight format (OCP microscaling, MXFP4).  wq is uint8 [out,in/2]: element 2i
// of a row in the low nibble of byte i, element 2i+1 in the high nibble; a
// nibble is e2m1 (bit 3 sign, bits 2..1 exponent, bit 0 mantissa), codes 0..7
// being 0, 0.5, 1, 1.5, 2, 3, 4, 6.  scale is uint8 [out,in/32]: one e8m0 byte
// b per (output row, block of 32 inputs), value 2^(b-127), 27 <= b <= 227 by
// contract (ops.quantize_weight_fp4).  code * scale then has 2 significant bits
// and a normal exponent: it is exact in bf16, so a weight fragment is turned
// into bf16 in registers (fp4x8_to_bf16: v_cvt_scalef32_pk_bf16_fp4, the scale
// folded into the conversion) and the result is a bf16 GEMM over the
// dequantised weight with no rounding of its own.
//
// The kernel is bound by the weight stream: every byte of wq is loaded exactly
// once, 16 bytes per lane and load, straight into MFMA fragments.
//
// MFMA: v_mfma_f32_16x16x32_bf16 with W as A (16 output rows x 32 k) and x^T as
// B (32 k x 16 tokens), so C holds 16 rows x 16 tokens and lane l ends with
// four consecutive output features (l>>4)*4 .. +3 of token l&15.  1 to 4 token
// tiles (template parameter MT) share each converted W fragment.
//
// k permutation.  A step is 128 consecutive k of a 16-row group.  Lane l (row
// l&15, g = l>>4) loads the 16 bytes 64*step + 16*g .. +15 of its packed row:
// the 32 consecutive k 128*step + 32*g .. +31, exactly one MX block, so the
// load has one scale byte, scale[row][4*step + g].  Dword h of the load (8
// nibbles) is the A fragment of the step's MFMA h.  MFMA h therefore
// contracts, at its own index k' = 8*g + j, the real k = 128*step + 32*g + 8*h
// + j, and the B fragment of lane l is the 16 bytes of x[token l&15] at that
// same k: one ds_read_b128.  A step is one dwordx4 load, 16 conversions and
// 4 * MT MFMAs per row group.
//
// Work split.  A workgroup is 4 waves and owns 64 output rows (4 row groups of
// 16; fewer in the last workgroup) and one K-slice of L steps.  The slice is
// walked in rounds of 4 steps (512 k): the workgroup stages x[0..16*MT) of the
// round's k in LDS once (rows past M are zeros, written to LDS only), and wave
// w takes step w of the round for all four row groups: 4 scale bytes ahead of
// 4 dwordx4 loads, 16 * MT MFMAs.  The next round's weights are loaded before
// the current round's MFMAs.  The LDS row of a token is 1024 bytes with its
// 16-byte chunk index XORed by token & 15; the 16 lanes of a B read (one g,
// one h: chunk 16*w + 4*g + h of the round, tokens 0..15) then sit at 16
// different chunks of one 256-byte bank period, so they cover all banks once
// and no row is padded.  MT <= 2 double-buffers the x stage (one barrier per
// round) and loads the next round's x into registers before the MFMAs too,
// writing it to the other buffer after them; MT 3 and 4 keep one buffer (two
// barriers, x loaded between them) and stay at 64 KB.  A round of 8 steps
// (1024 k, two per wave, 2 KB per token) was built and timed against this one
// on the MI355X: within 3% at the large shapes up to 16 rows, 10% faster at
// 4096 x 4096, and 1.5 to 2 times slower at 64 rows, where its 128 KB of LDS
// leave one workgroup per CU (profiles/README Round 17).  It was not kept.
//
// Split-K and its order.  A wave sums its steps in ascending order (step, then
// h); the four waves' partial tiles are summed through LDS in wave order; with
// more than one K-slice each workgroup writes its fp32 tile to a workspace
// [S,M,out] and linear_fp4w_combine_kernel adds the slices in slice order and
// rounds once.  No atomics, no hand-off between workgroups.  The split
// (l4_split) is a function of (in, out) alone, a C column of an MFMA depends
// on its own B column alone, and MT changes only how many columns ride along:
// row m's output bits are a function of x[m] and the weight, not of M or of
// the other rows.
//
// linear_fp4w_dequant writes the bf16 [out,in] weight (16 bytes and one scale
// byte in, 64 bytes out per item) for M > 64, which runs on hipBLASLt.
#include "attn_tile.h"

namespace lpp {

typedef __attribute__((ext_vector_type(2))) __bf16 fp4_bf16x2;

constexpr int L4_THREADS = 256;
constexpr int L4_WAVES = 4;
constexpr int L4_RG = 4;                 // row groups of 16 per workgroup
constexpr int L4_ROWS = 16 * L4_RG;
constexpr int L4_STEP = 128;             // k per step: 4 MX blocks, one per lane group
constexpr int L4_MX = 32;                // k per scale byte
constexpr int L4_MAX_M = 64;
constexpr int L4_TARGET_WGS = 512;       // about 2048 waves

constexpr int L4_ROUND = L4_WAVES;                 // steps per round, one per wave
constexpr int L4_TOK_BYTES = L4_ROUND * L4_STEP * 2;   // LDS bytes of one token's round
constexpr int L4_CHUNKS = L4_TOK_BYTES / 16;       // 16-byte chunks of a token's round

constexpr int l4_nbuf(int MT) { return MT <= 2 ? 2 : 1; }
// x stage (reused as the 4 waves' fp32 tiles for the reduction, MT * 16 KB)
constexpr int l4_lds_bytes(int MT) { return l4_nbuf(MT) * MT * 16 * L4_TOK_BYTES; }

// 8 e2m1 nibbles of a dword (element j in nibble j) times 2^(b-127) to bf16x8:
// four v_cvt_scalef32_pk_bf16_fp4, one per byte, the low nibble first; exact.
__device__ __forceinline__ bf16x8 fp4x8_to_bf16(uint32_t w, float scale) {
  const fp4_bf16x2 r[4] = {__builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(w, scale, 0),
                           __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(w, scale, 1),
                           __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(w, scale, 2),
                           __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(w, scale, 3)};
  return __builtin_bit_cast(bf16x8, r);
}
// e8m0 byte to float: b is the float's exponent field (1 <= b <= 254)
__device__ __forceinline__ float e8m0_to_f32(uint32_t b) {
  return __builtin_bit_cast(float, b << 23);
}

// K-slices: L steps of 128 k each (a multiple of 4, a whole round), S of them,
// the last one shorter when L does not divide in/128.  From (in, out) only.
struct L4Split {
  int L, S;
};
static L4Split l4_split(int64_t in, int64_t out) {
  const int64_t ns = in / L4_STEP, nrw = (out + L4_ROWS - 1) / L4_ROWS;
  const int64_t s0 = std::max<int64_t>(1, L4_TARGET_WGS / nrw);
  int64_t L = std::max<int64_t>(L4_ROUND, (ns + s0 - 1) / s0);
  L = (L + L4_ROUND - 1) / L4_ROUND * L4_ROUND;
  return {(int)L, (int)((ns + L - 1) / L)};
}

template <int MT>
__global__ __launch_bounds__(L4_THREADS) void linear_fp4w_kernel(
    const short* __restrict__ x,        // [M,in] bf16
    const uint8_t* __restrict__ wq,     // [out,in/2] e2m1 pairs
    const uint8_t* __restrict__ scale,  // [out,in/32] e8m0
    short* __restrict__ y,              // [M,out] bf16 (S == 1)
    float* __restrict__ ws,             // [S,M,out] fp32 (S > 1)
    int M, int in, int out, int L) {
  extern __shared__ __attribute__((aligned(16))) char l4_smem[];
  constexpr int NBUF = l4_nbuf(MT);
  constexpr int BUF_BYTES = MT * 16 * L4_TOK_BYTES;
  constexpr int XI = MT * 16 * L4_CHUNKS / L4_THREADS;   // x chunks a thread stages per round
  constexpr int XB = NBUF == 2 ? XI : 4;                 // ... and how many it holds at a time
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int n16 = lane & 15, g = lane >> 4;
  const int ns = in / L4_STEP;
  const int row0 = blockIdx.x * L4_ROWS;
  const int nrg = min(L4_RG, (out - row0) / 16);   // >= 1
  const int sb = blockIdx.y * L, se = min(sb + L, ns);  // this slice's steps

  // lane's byte of its packed row and of its scale row at step 0, per row group
  const uint8_t* wrow[L4_RG];
  const uint8_t* srow[L4_RG];
#pragma unroll
  for (int rg = 0; rg < L4_RG; ++rg) {
    const int64_t r = row0 + 16 * min(rg, nrg - 1) + n16;   // clamped: never past out
    wrow[rg] = wq + r * (in / 2) + 16 * g;
    srow[rg] = scale + r * (in / L4_MX) + g;
  }

  f32x4 acc[L4_RG][MT];
#pragma unroll
  for (int rg = 0; rg < L4_RG; ++rg)
#pragma unroll
    for (int t = 0; t < MT; ++t) acc[rg][t] = f32x4{0.f, 0.f, 0.f, 0.f};

  // step st of this wave: the scale bytes ahead of the 16-byte loads they scale
  auto load_w = [&](int st, uint4(&w)[L4_RG], uint32_t(&sc)[L4_RG]) {
    if (st >= se) return;
#pragma unroll
    for (int rg = 0; rg < L4_RG; ++rg)
      if (rg < nrg) sc[rg] = srow[rg][4 * st];
#pragma unroll
    for (int rg = 0; rg < L4_RG; ++rg)
      if (rg < nrg)
        w[rg] = *reinterpret_cast<const uint4*>(wrow[rg] + (int64_t)st * (L4_STEP / 2));
  };
  // x[0..16*MT) of k0 .. k0 + 511, batch jb of a thread's chunks: from memory
  // into registers (zeros past M and past the slice), and from there into
  // buffer buf
  auto load_x = [&](int k0, int jb, bf16x8(&xv)[XB]) {
    const int kend = se * L4_STEP;
#pragma unroll
    for (int j = 0; j < XB; ++j) {
      const int i = tid + (jb * XB + j) * L4_THREADS, tok = i / L4_CHUNKS,
                k = k0 + 8 * (i % L4_CHUNKS);
      xv[j] = bf16x8{0, 0, 0, 0, 0, 0, 0, 0};
      if (tok < M && k < kend) xv[j] = *reinterpret_cast<const bf16x8*>(x + (int64_t)tok * in + k);
    }
  };
  auto store_x = [&](int buf, int jb, const bf16x8(&xv)[XB]) {
    char* xs = l4_smem + buf * BUF_BYTES;
#pragma unroll
    for (int j = 0; j < XB; ++j) {
      const int i = tid + (jb * XB + j) * L4_THREADS, tok = i / L4_CHUNKS, ch = i % L4_CHUNKS;
      *reinterpret_cast<bf16x8*>(xs + tok * L4_TOK_BYTES + 16 * (ch ^ (tok & 15))) = xv[j];
    }
  };

  uint4 wc[L4_RG] = {}, wn[L4_RG] = {};
  uint32_t sc[L4_RG] = {}, sn[L4_RG] = {};
  bf16x8 xv[XB];
  load_w(sb + wid, wc, sc);
#pragma unroll 1
  for (int jb = 0; jb < XI / XB; ++jb) {
    load_x(sb * L4_STEP, jb, xv);
    store_x(0, jb, xv);
  }
  int buf = 0;
  for (int r0 = sb; r0 < se; r0 += L4_ROUND) {
    __syncthreads();
    load_w(r0 + L4_ROUND + wid, wn, sn);
    const bool more = r0 + L4_ROUND < se;   // workgroup-uniform
    // with two buffers the next round's x is loaded before this round's MFMAs
    // and written after them; with one, after the barrier that frees the buffer
    if (NBUF == 2 && more) load_x((r0 + L4_ROUND) * L4_STEP, 0, xv);
    if (r0 + wid < se) {   // wave-uniform
      const char* xs = l4_smem + buf * BUF_BYTES + n16 * L4_TOK_BYTES;
      bf16x8 bf[MT][4];
#pragma unroll
      for (int t = 0; t < MT; ++t)
#pragma unroll
        for (int h = 0; h < 4; ++h) {
          const int ch = 16 * wid + 4 * g + h;
          bf[t][h] = *reinterpret_cast<const bf16x8*>(xs + t * 16 * L4_TOK_BYTES +
                                                      16 * (ch ^ n16));
        }
#pragma unroll
      for (int rg = 0; rg < L4_RG; ++rg)
        if (rg < nrg) {   // workgroup-uniform
          const float f = e8m0_to_f32(sc[rg]);
          const bf16x8 a[4] = {fp4x8_to_bf16(wc[rg].x, f), fp4x8_to_bf16(wc[rg].y, f),
                               fp4x8_to_bf16(wc[rg].z, f), fp4x8_to_bf16(wc[rg].w, f)};
#pragma unroll
          for (int h = 0; h < 4; ++h)
#pragma unroll
            for (int t = 0; t < MT; ++t)
              acc[rg][t] =
                  __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[h], bf[t][h], acc[rg][t], 0, 0, 0);
        }
    }
#pragma unroll
    for (int rg = 0; rg < L4_RG; ++rg) {
      wc[rg] = wn[rg];
      sc[rg] = sn[rg];
    }
    if (NBUF == 2) {
      buf ^= 1;
      if (more) store_x(buf, 0, xv);   // every wave is past this round's barrier: buf is free
    } else if (more) {
      __syncthreads();
#pragma unroll 1   // a batch at a time: holding them all costs MT 4 a wave per SIMD
      for (int jb = 0; jb < XI / XB; ++jb) {
        load_x((r0 + L4_ROUND) * L4_STEP, jb, xv);
        store_x(0, jb, xv);
      }
    }
  }

  // ---- the four waves' tiles, summed in wave order ------------------------------
  __syncthreads();
  f32x4* red = reinterpret_cast<f32x4*>(l4_smem);   // [wave][rg][t][lane]
#pragma unroll
  for (int rg = 0; rg < L4_RG; ++rg)
#pragma unroll
    for (int t = 0; t < MT; ++t) red[((wid * L4_RG + rg) * MT + t) * 64 + lane] = acc[rg][t];
  __syncthreads();
  constexpr int ITEMS = L4_RG * MT * 64;
  for (int i = tid; i < nrg * MT * 64; i += L4_THREADS) {
    f32x4 v = red[i];
#pragma unroll
    for (int w = 1; w < L4_WAVES; ++w) v += red[w * ITEMS + i];
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
__global__ __launch_bounds__(256) void linear_fp4w_combine_kernel(
    const float* __restrict__ ws, short* __restrict__ y, int64_t n4, int S) {
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += (int64_t)gridDim.x * 256) {
    f32x4 v = reinterpret_cast<const f32x4*>(ws)[i];
    for (int s = 1; s < S; ++s) v += reinterpret_cast<const f32x4*>(ws)[s * n4 + i];
    uint2 pk = {cvt_pk_bf16(v[0], v[1]), cvt_pk_bf16(v[2], v[3])};
    reinterpret_cast<uint2*>(y)[i] = pk;
  }
}

// w[out,in] bf16 = code * scale; an item is 16 bytes of a packed row, one MX
// block (32 k, one scale byte), n16 = out * in / 32 items: item i has scale
// byte i
__global__ __launch_bounds__(256) void linear_fp4w_dequant_kernel(
    const uint8_t* __restrict__ wq, const uint8_t* __restrict__ scale, short* __restrict__ w,
    int64_t n16) {
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n16; i += (int64_t)gridDim.x * 256) {
    const float f = e8m0_to_f32(scale[i]);
    const uint4 b = reinterpret_cast<const uint4*>(wq)[i];
    bf16x8* dst = reinterpret_cast<bf16x8*>(w) + 4 * i;
    dst[0] = fp4x8_to_bf16(b.x, f);
    dst[1] = fp4x8_to_bf16(b.y, f);
    dst[2] = fp4x8_to_bf16(b.z, f);
    dst[3] = fp4x8_to_bf16(b.w, f);
  }
}

template <int MT>
static void launch_linear4(const at::Tensor& x, const at::Tensor& wq, const at::Tensor& scale,
                           at::Tensor& y, float* ws, const L4Split& sp) {
  const int M = x.size(0), in = x.size(1), out = wq.size(0);
  hipLaunchKernelGGL((linear_fp4w_kernel<MT>), dim3((out + L4_ROWS - 1) / L4_ROWS, sp.S),
                     dim3(L4_THREADS), l4_lds_bytes(MT), current_stream(),
                     (const short*)x.data_ptr(), (const uint8_t*)wq.data_ptr(),
                     (const uint8_t*)scale.data_ptr(), (short*)y.data_ptr(), ws, M, in, out, sp.L);
  LPP_CHECK_HIP(hipGetLastError());
}

static bool l4_disjoint(const at::Tensor& a, const at::Tensor& b) {
  const char* ca = (const char*)a.data_ptr();
  const char* cb = (const char*)b.data_ptr();
  return ca + a.nbytes() <= cb || cb + b.nbytes() <= ca;
}

// The checks the two entry points share: the packed weight and its scale bytes.
static void check_weight4(const char* who, const at::Tensor& wq, const at::Tensor& scale) {
  TORCH_CHECK(wq.is_cuda() && wq.scalar_type() == at::kByte && wq.dim() == 2 &&
                  wq.is_contiguous(),
              who, ": wq must be a contiguous uint8 CUDA tensor [out,in/2]");
  const int64_t out = wq.size(0), in = 2 * wq.size(1);
  TORCH_CHECK(in >= L4_STEP && in % L4_STEP == 0, who, ": in must be a multiple of 128, got ", in);
  TORCH_CHECK(out >= 16 && out % 16 == 0, who, ": out must be a multiple of 16, got ", out);
  TORCH_CHECK(scale.is_cuda() && scale.device() == wq.device() &&
                  scale.scalar_type() == at::kByte && scale.is_contiguous(),
              who, ": scale must be a contiguous uint8 (e8m0) tensor on wq's device");
  TORCH_CHECK(scale.dim() == 2 && scale.size(0) == out && scale.size(1) == in / L4_MX, who,
              ": scale must be [out, in/32] = [", out, ", ", in / L4_MX, "], got ",
              scale.sizes());
  TORCH_CHECK(wq.numel() < ((int64_t)1 << 40) && out < ((int64_t)1 << 31) - L4_ROWS &&
                  in < ((int64_t)1 << 31),
              who, ": weight too large");
  TORCH_CHECK(l4_disjoint(wq, scale), who, ": wq and scale overlap");
}

}  // namespace lpp

// gfx950 (hipcc -O3), linear_fp4w_kernel<MT> for MT = 1 / 2 / 3 / 4: NumVgprs
// 146 / 180 / 154 / 174 plus 16 / 36 / 52 / 72 AGPRs, 3 / 2 / 2 / 2 waves per
// SIMD, ScratchSize 0 everywhere, dynamic LDS 32 / 64 / 48 / 64 KB (no static
// LDS).  MT 1 and 2 hold the next round's x (16 * MT registers) over the MFMAs;
// at MT 2 that costs the third wave per SIMD, which its 64 KB of LDS (two
// workgroups, 8 waves per CU) did not allow anyway.  combine 12 VGPRs, dequant
// 23, neither uses LDS or scratch.
at::Tensor linear_fp4w(at::Tensor x, at::Tensor wq, at::Tensor scale) {
  const char* who = "linear_fp4w";
  lpp::check_weight4(who, wq, scale);
  const int64_t out = wq.size(0), in = 2 * wq.size(1);
  TORCH_CHECK(x.is_cuda() && x.device() == wq.device() && x.scalar_type() == at::kBFloat16, who,
              ": x must be a bf16 tensor on wq's device");
  TORCH_CHECK(x.dim() == 2 && x.size(1) == in, who, ": x must be [M, in] = [M, ", in, "], got ",
              x.sizes());
  TORCH_CHECK(x.is_contiguous(), who, ": x must be contiguous");
  const int64_t M = x.size(0);
  TORCH_CHECK(M >= 1 && M <= lpp::L4_MAX_M, who, ": M must be 1 .. ", lpp::L4_MAX_M, ", got ", M);
  TORCH_CHECK(lpp::l4_disjoint(x, wq) && lpp::l4_disjoint(x, scale), who,
              ": x overlaps the weight");
  const lpp::L4Split sp = lpp::l4_split(in, out);
  TORCH_CHECK(sp.S <= 65535, who, ": too many K-slices");
  auto y = at::empty({M, out}, x.options());
  at::Tensor ws;
  if (sp.S > 1) ws = at::empty({(int64_t)sp.S, M, out}, x.options().dtype(at::kFloat));
  float* wsp = sp.S > 1 ? ws.data_ptr<float>() : nullptr;
  switch ((M + 15) / 16) {
    case 1: lpp::launch_linear4<1>(x, wq, scale, y, wsp, sp); break;
    case 2: lpp::launch_linear4<2>(x, wq, scale, y, wsp, sp); break;
    case 3: lpp::launch_linear4<3>(x, wq, scale, y, wsp, sp); break;
    default: lpp::launch_linear4<4>(x, wq, scale, y, wsp, sp); break;
  }
  if (sp.S > 1) {
    const int64_t n4 = M * out / 4;
    hipLaunchKernelGGL(lpp::linear_fp4w_combine_kernel, dim3(lpp::grid_for(n4, 256)), dim3(256),
                       0, lpp::current_stream(), wsp, (short*)y.data_ptr(), n4, sp.S);
    LPP_CHECK_HIP(hipGetLastError());
  }
  return y;
}

at::Tensor linear_fp4w_dequant(at::Tensor wq, at::Tensor scale) {
  lpp::check_weight4("linear_fp4w_dequant", wq, scale);
  auto w = at::empty({wq.size(0), 2 * wq.size(1)}, wq.options().dtype(at::kBFloat16));
  const int64_t n16 = wq.numel() / 16;
  hipLaunchKernelGGL(lpp::linear_fp4w_dequant_kernel, dim3(lpp::grid_for(n16, 256)), dim3(256), 0,
                     lpp::current_stream(), (const uint8_t*)wq.data_ptr(),
                     (const uint8_t*)scale.data_ptr(), (short*)w.data_ptr(), n16);
  LPP_CHECK_HIP(hipGetLastError());
  return w;
}
