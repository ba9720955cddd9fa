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
// item) for the default M > 64 path, which stays on hipBLASLt.  The opt-in
// M > 64 path is linear_fp8w_tiled_kernel, described at its definition.
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

// ---- tiled kernel: any M, routed above 64 rows ----------------------------------
// From a few tens to a few hundred rows the GEMM is still bound by the weight
// stream, so the e4m3 bytes are read once per (token tile, K-slice) and turned
// into bf16 on the way into LDS; no bf16 copy of the weight exists anywhere.
//
// Work split.  256 threads, 4 waves in a 2x2 grid (wr = wave>>1 output half, wt
// = wave&1 token half).  A workgroup owns 128 tokens x 128 output rows and one
// K-slice; a wave owns 64 x 64 as 2x2 accumulators of v_mfma_f32_32x32x16_bf16
// with W as A (32 rows x 16 k) and x^T as B (16 k x 32 tokens): the skinny
// kernel's orientation, so lane l ends with token l&31 and runs of 4 consecutive
// output features (crow32), stored as 8-byte packets (16-byte ones into the
// workspace).  A wave whose 64 x 64 lies wholly past M or past out runs no
// MFMA, a wave-uniform choice.
//
// K loop.  A step is 64 k, half a scale block, so a (row, step) pair has one
// scale.  Per step a thread loads two 16-byte pieces of wq (rows tid>>2 and
// +64, bytes 16*(tid&3) .. +15 of the step) with their scales and four bf16x8
// packets of x (tokens tid>>3 + 32p, chunk tid&7); the weight bytes become bf16
// in registers (fp8x8_to_bf16, exact) and both go to LDS as 16-byte writes.  A
// weight byte is converted once per workgroup.  The loads of step t+1 are
// issued before the MFMAs of step t, converted and written after them into the
// other buffer; one barrier per step.  A stage is 16 KB of W and 16 KB of x,
// 64 KB double-buffered, two workgroups per CU.
//
// LDS layout (lt_off).  Rows (an output row's or a token's 64 k) are 128 bytes,
// 8 chunks of 16; chunk c of row r sits at chunk c ^ ((r >> 1) & 7).  The swizzle
// takes (r >> 1), not the low bits r & 7 of the first design: with 128-byte
// rows, rows r and r + 8 would otherwise fall on the same 16 bytes of the
// 256-byte bank period and the 16 lanes of a ds_read_b128 phase (rows r0 .. r0 +
// 15, one k chunk) would conflict two ways.  With (r >> 1) those 16 lanes give
// 16 different (r & 1, chunk) places, and so do the 16 lanes of each staging
// write (4 rows x 4 pieces of W, 2 rows x 8 chunks of x).
//
// Edges.  Tokens past M are zeros in LDS only, never loaded (their lanes load
// row M - 1 instead, which keeps the loads free of branches) and never stored;
// rows past out load from row out - 1 and store nothing.
//
// Split over K.  lt_slices() picks S from (in, out, number of token tiles) so
// that tiles * S is about 512, two resident workgroups on each of the 256 CUs,
// with at least 4 blocks (8 steps) in a slice; slice s takes nb / S blocks of
// 128, the first nb % S slices one more.  The first rule (256 workgroups, the
// workspace kept below the weight bytes) lost to this one in a sweep of forced
// slice counts on the MI355X (profiles/README Round 16): a step waits for its
// global loads longer than its 16 MFMAs take, one step of prefetch does not
// cover that, and a second workgroup on the CU does; the workspace traffic
// costs less than the idle CUs.  A thread sums ascending k inside
// its slice; with S > 1 linear_fp8w_combine_kernel adds the slices in slice
// order and rounds once.  No atomics, no hand-off: the same call returns the
// same bits every time, but the bits of a row may depend on M through S.
//
// The epilogue stores straight from the accumulators (a lane's 8-byte packets
// of one token lie `out` elements apart from its neighbour's); y is M * out * 2
// bytes against in * out of weight, so it was left unstaged.
constexpr int LT_TILE = 128;                       // tokens and output rows per workgroup
constexpr int LT_STEP = 64;                        // k per step
constexpr int LT_IMG = LT_TILE * LT_STEP * 2;      // one staged operand, 16 KB
constexpr int LT_LDS = 4 * LT_IMG;                 // W and x, two buffers
constexpr int LT_TARGET_WGS = 512;                 // two per CU

__host__ __device__ __forceinline__ int lt_off(int row, int ch) {
  return 128 * row + 16 * (ch ^ ((row >> 1) & 7));
}

static int lt_slices(int64_t in, int64_t out, int64_t ntt) {
  const int64_t nb = in / LF_BLK, tiles = (out + LT_TILE - 1) / LT_TILE * ntt;
  const int64_t s = std::min((2 * LT_TARGET_WGS / tiles + 1) / 2, nb / 4);   // nearest
  return (int)std::max<int64_t>(1, std::min<int64_t>(s, 65535));
}

__global__ __launch_bounds__(LF_THREADS) void linear_fp8w_tiled_kernel(
    const short* __restrict__ x,        // [M,in] bf16
    const uint8_t* __restrict__ wq,     // [out,in] e4m3
    const float* __restrict__ scale,    // [out,in/128]
    short* __restrict__ y,              // [M,out] bf16 (S == 1)
    float* __restrict__ ws,             // [S,M,out] fp32 (S > 1)
    int M, int in, int out, int S) {
  extern __shared__ __attribute__((aligned(16))) char lt_smem[];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);   // a scalar: uniform branches
  const int wr = wid >> 1, wt = wid & 1, l31 = lane & 31, hi = lane >> 5;
  const int nb = in / LF_BLK;
  const int row0 = blockIdx.x * LT_TILE, tok0 = blockIdx.y * LT_TILE;
  // this slice: blocks b0 .. b0 + nblk - 1, two steps each
  const int s = blockIdx.z, bq = nb / S, brem = nb % S;
  const int b0 = s * bq + min(s, brem), nsteps = 2 * (bq + (s < brem ? 1 : 0));
  const int64_t k0 = (int64_t)b0 * LF_BLK;

  // staging roles
  const int wrow = tid >> 2, wpc = tid & 3, xtok = tid >> 3, xch = tid & 7;
  const uint8_t* wp[2];
  const float* sp[2];
#pragma unroll
  for (int p = 0; p < 2; ++p) {
    const int64_t r = min(row0 + wrow + 64 * p, out - 1);   // clamped: never past out
    wp[p] = wq + r * in + k0 + 16 * wpc;
    sp[p] = scale + r * nb + b0;
  }
  const short* xp[4];
  bool xin[4];
#pragma unroll
  for (int p = 0; p < 4; ++p) {
    const int tok = tok0 + xtok + 32 * p;
    xin[p] = tok < M;
    xp[p] = x + (int64_t)min(tok, M - 1) * in + k0 + 8 * xch;
  }
  const int w_off = lt_off(wrow, 2 * wpc), x_off = lt_off(xtok, xch);
  // fragment reads: row l31 of a 32-row sub-tile, chunk 2 * kk + hi
  const int a_base = lt_off(64 * wr + l31, hi), b_base = lt_off(64 * wt + l31, hi);
  // a wave whose 64 x 64 holds no real row or no real token only stages
  const bool active = row0 + 64 * wr < out && tok0 + 64 * wt < M;

  f32x16 acc[2][2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

  uint4 wv[2];
  float sc[2];
  bf16x8 xv[4];
  auto load_g = [&](int t) {
#pragma unroll
    for (int p = 0; p < 2; ++p) {
      sc[p] = sp[p][t >> 1];
      wv[p] = *reinterpret_cast<const uint4*>(wp[p] + t * LT_STEP);
    }
#pragma unroll
    for (int p = 0; p < 4; ++p)   // a token past M reads row M - 1 and is zeroed in store_l
      xv[p] = *reinterpret_cast<const bf16x8*>(xp[p] + t * LT_STEP);
  };
  auto store_l = [&](int buf) {
    char* wi = lt_smem + buf * 2 * LT_IMG;
    char* xi = wi + LT_IMG;
#pragma unroll
    for (int p = 0; p < 2; ++p) {
      *reinterpret_cast<bf16x8*>(wi + w_off + 64 * 128 * p) =
          fp8x8_to_bf16(wv[p].x, wv[p].y, sc[p]);
      *reinterpret_cast<bf16x8*>(wi + (w_off ^ 16) + 64 * 128 * p) =
          fp8x8_to_bf16(wv[p].z, wv[p].w, sc[p]);
    }
#pragma unroll
    for (int p = 0; p < 4; ++p)
      *reinterpret_cast<bf16x8*>(xi + x_off + 32 * 128 * p) =
          xin[p] ? xv[p] : bf16x8{0, 0, 0, 0, 0, 0, 0, 0};
  };

  load_g(0);
  store_l(0);
  __syncthreads();
  for (int t = 0; t < nsteps; ++t) {
    const bool more = t + 1 < nsteps;
    load_g(more ? t + 1 : t);   // branch-free, so the loads stay in flight over the MFMAs
    const char* wi = lt_smem + (t & 1) * 2 * LT_IMG;
    const char* xi = wi + LT_IMG;
#pragma unroll
    for (int kk = 0; active && kk < 4; ++kk) {
      bf16x8 a[2], b[2];
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        a[i] = *reinterpret_cast<const bf16x8*>(wi + (a_base ^ (32 * kk)) + 32 * 128 * i);
        b[i] = *reinterpret_cast<const bf16x8*>(xi + (b_base ^ (32 * kk)) + 32 * 128 * i);
      }
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
          acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[i], b[j], acc[i][j], 0, 0, 0);
    }
    if (more) store_l((t + 1) & 1);
    __syncthreads();
  }

  float* wsl = ws ? ws + (int64_t)s * M * out : nullptr;
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int tok = tok0 + 64 * wt + 32 * j + l31;
      if (!active || tok >= M) continue;
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const int row = row0 + 64 * wr + 32 * i + 8 * g + 4 * hi;   // crow32(4 * g, hi)
        if (row >= out) continue;                                   // out % 16 == 0: all 4 or none
        const int64_t o = (int64_t)tok * out + row;
        const f32x16& c = acc[i][j];
        if (wsl) {
          *reinterpret_cast<f32x4*>(wsl + o) = f32x4{c[4 * g], c[4 * g + 1], c[4 * g + 2], c[4 * g + 3]};
        } else {
          uint2 pk = {cvt_pk_bf16(c[4 * g], c[4 * g + 1]), cvt_pk_bf16(c[4 * g + 2], c[4 * g + 3])};
          *reinterpret_cast<uint2*>(y + o) = pk;
        }
      }
    }
}

// gfx950 (hipcc -O3), linear_fp8w_kernel<MT> for MT = 1 / 2 / 3 / 4: NumVgprs
// 134 / 126 / 132 / 142 plus 16 / 32 / 48 / 64 AGPRs (the accumulators), 3 / 3 /
// 2 / 2 waves per SIMD, ScratchSize 0 everywhere, dynamic LDS 32 / 64 / 48 /
// 64 KB (no static LDS).  combine 12 VGPRs, dequant 20, neither uses LDS or
// scratch.  linear_fp8w_tiled_kernel: NumVgprs 136 plus 64 AGPRs (the 2x2
// accumulators), 2 waves per SIMD (which the 64 KB of dynamic LDS, two
// workgroups per CU, allow anyway), ScratchSize 0, no static LDS.
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

// ... and the activations, after check_weight: bf16 [M,in], M >= 1, beside the weight.
static void check_x(const char* who, const at::Tensor& x, const at::Tensor& wq,
                    const at::Tensor& scale) {
  TORCH_CHECK(x.is_cuda() && x.device() == wq.device() && x.scalar_type() == at::kBFloat16, who,
              ": x must be a bf16 tensor on wq's device");
  TORCH_CHECK(x.dim() == 2 && x.size(1) == wq.size(1), who, ": x must be [M, in] = [M, ",
              wq.size(1), "], got ", x.sizes());
  TORCH_CHECK(x.is_contiguous(), who, ": x must be contiguous");
  TORCH_CHECK(x.size(0) >= 1, who, ": M must be at least 1, got ", x.size(0));
  TORCH_CHECK(lin_disjoint(x, wq) && lin_disjoint(x, scale), who, ": x overlaps the weight");
}

}  // namespace lpp

at::Tensor linear_fp8w(at::Tensor x, at::Tensor wq, at::Tensor scale) {
  const char* who = "linear_fp8w";
  lpp::check_weight(who, wq, scale);
  const int64_t out = wq.size(0), in = wq.size(1);
  lpp::check_x(who, x, wq, scale);
  const int64_t M = x.size(0);
  TORCH_CHECK(M <= lpp::LF_MAX_M, who, ": M must be 1 .. ", lpp::LF_MAX_M, ", got ", M);
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

at::Tensor linear_fp8w_tiled(at::Tensor x, at::Tensor wq, at::Tensor scale, int64_t slices) {
  const char* who = "linear_fp8w_tiled";
  lpp::check_weight(who, wq, scale);
  lpp::check_x(who, x, wq, scale);
  const int64_t M = x.size(0), out = wq.size(0), in = wq.size(1), nb = in / lpp::LF_BLK;
  const int64_t ntt = (M + lpp::LT_TILE - 1) / lpp::LT_TILE;
  TORCH_CHECK(ntt <= 65535, who, ": too many rows, M = ", M);
  TORCH_CHECK(slices >= 0 && slices <= nb, who, ": slices must be 0 (the rule) or 1 .. in/128 = ",
              nb, ", got ", slices);
  TORCH_CHECK(slices <= 65535, who, ": too many K-slices");
  const int S = slices ? (int)slices : lpp::lt_slices(in, out, ntt);
  auto y = at::empty({M, out}, x.options());
  at::Tensor ws;
  if (S > 1) ws = at::empty({(int64_t)S, M, out}, x.options().dtype(at::kFloat));
  float* wsp = S > 1 ? ws.data_ptr<float>() : nullptr;
  hipLaunchKernelGGL(lpp::linear_fp8w_tiled_kernel,
                     dim3((out + lpp::LT_TILE - 1) / lpp::LT_TILE, ntt, S), dim3(lpp::LF_THREADS),
                     lpp::LT_LDS, lpp::current_stream(), (const short*)x.data_ptr(),
                     (const uint8_t*)wq.data_ptr(), scale.data_ptr<float>(), (short*)y.data_ptr(),
                     wsp, (int)M, (int)in, (int)out, S);
  LPP_CHECK_HIP(hipGetLastError());
  if (S > 1) {
    const int64_t n4 = M * out / 4;
    hipLaunchKernelGGL(lpp::linear_fp8w_combine_kernel, dim3(lpp::grid_for(n4, 256)), dim3(256),
                       0, lpp::current_stream(), wsp, (short*)y.data_ptr(), n4, S);
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
