// Extend attention for gfx950 (CDNA4), bf16, D=128: Sq new tokens per batch
// row at per-row positions over the ragged slot KV cache (chunked prefill,
// prefix reuse, draft verification).  Row n sits at cache row rows[n] with
// p = positions[n] tokens cached and len = q_lens[n] valid new tokens; token
// i < len is rotated at p + i, its k/v land in cache[row, p + i], and its
// output attends keys 0 .. p + i of the row.
//
// Two launches plus a combine, ordered by the stream alone (no hand-off
// between workgroups, no atomics, no spin-waits):
//
//   append     one workgroup per (token, row): RoPE of q into the bf16 scratch
//              q_rot, RoPE of k_new into the cache, v_new into the cache, all
//              in 16-byte packets, and lengths[row] = p + len.  The rotation
//              is attention_decode.hip's expression, so a token appended here
//              and one appended by decode round alike.
//   attention  reads only q_rot and the cache: after the append nothing in it
//              needs to know which keys are new.
//
// Row space of the attention kernel: one (batch row, kv head) pair owns
// R = Sq * REP rows, token-major and head-minor: row r is token r / REP, head
// hkv * REP + r % REP - the memory order of q_rot[n, :, hkv*REP:(hkv+1)*REP, :].
// A wave's 32 rows are 32 / REP tokens of REP consecutive 256-byte rows, its
// causal bound spans 32 / REP keys, and a staged K/V tile serves the whole
// group once: a 32-token chunk at REP = 8 fills a 256-row workgroup.
//
// The tile loop is the forward's (attention_fwd.hip) on the helpers of
// attn_tile.h: swapped mfma_32x32x16(K, Q) so a lane holds one row's scores,
// in-register max and sum with one permlane32_swap, pack_pair to the PV
// A-fragments, one attn_off<32> image each for K and V (row reads and
// ds_read_b64_tr_b16), attn_tile_pipeline with one barrier per 64-key tile,
// defer-max decided before the exponentiation, attn_exp2.
//
// Mask: key kv is visible to row r iff r < len * REP and kv <= p + r / REP.
// No key at or past p + len is addressed: tile loads clamp to key p + len - 1.
//
// Split over keys: below kExtendSplitRows rows the keys are cut into chunks of
// C keys; workgroup (block, chunk) writes unnormalised fp32 O, m and l of its
// valid rows to a workspace and the combine kernel reduces a row's
// (p + token) / C + 1 chunks in chunk order.  At or above the threshold one
// workgroup walks all keys and stores bf16 O.  Threshold and C depend on
// (Sq, REP) alone, and every workgroup's work is a function of its own batch
// row, so a batch row's output bits depend on its data, its position, its
// q_len and the call's (Sq, REP) - not on N, the other rows, their order or
// max_len.
//
// FP8 cache (attn_fp8.h: e4m3 rows, one power-of-two fp32 scale per (slot, kv
// head, token) in k_scale / v_scale [slots,Hkv,Tmax]) is the template
// parameter FP8 of the append and the attention kernel.  The append quantises:
// the 8 lanes that hold a head's row agree on its amax, and the rotated bf16 K
// row and the V row leave as 128 bytes and a scale.  The attention kernel
// differs in ld_tile alone: 8 bytes and the key's scale become the bf16x8 that
// write_tile stages, exactly, so the LDS images, the tile loop, the mask, the
// split path and the combine are the bf16 ones.
//
// Paged cache (attn_paged.h: a pool of 64-key pages under a block table) is the
// template parameter PAGED of the same two kernels.  A page is one key tile
// and every tile starts at a multiple of 64, so a tile's page id is
// workgroup-uniform: ld_tile adds the page's base (SGPRs) where the slot
// layout adds the row's and stays otherwise as it is.  attn_tile_pipeline
// issues the loads of tile t + 1 a whole compute phase ahead, and a table
// load in front of them would put its latency on that path; so the entry of
// tile t + 1 is fetched (one scalar load) together with the global loads of
// tile t and is long there when ld_tile comes for it.  The key index is
// clamped to p + len - 1 before the lookup, as for the loads themselves.  The
// append looks up the page of its own token: a chunk that crosses a page
// boundary lands in two pages.
#include "attention.h"
#include "attn_fp8.h"
#include "attn_paged.h"

namespace lpp {

constexpr int AE_QW = 32;               // rows per wave
constexpr int AE_QB = 256;              // rows per workgroup (8 waves)
constexpr int AE_KVB = ATTN_TILE_ROWS;  // keys per tile
constexpr float AE_THR = 8.0f;          // defer-max threshold (exp2 domain)
enum { AE_K, AE_V, AE_IMAGES };         // LDS images (64 KB): K, V
constexpr int AE_LDS_BYTES = attn_lds_bytes(AE_IMAGES);
// C and the split threshold: the sweep of profiles/README.md, Round 11.  They
// may depend on (Sq, REP) only, so they are the choice of least regret over
// N = 1 .. 8 rows: C = 256 is best for one row, C = 1024 for eight.
constexpr int kExtendChunk = 512;        // C: keys per split workgroup
constexpr int kExtendSplitRows = 2048;   // R below this takes the split path
constexpr int kExtendAppendThreads = 256;
constexpr float kExtendMinM = -1e30f;    // combine's empty running max (finite)

// Row metadata shared by the three kernels.  A row whose cache row, position
// or length is out of range is skipped: nothing read, nothing written, o = 0.
struct ExtendRow {
  int64_t r;
  int p, len;
  bool ok;
};
__device__ __forceinline__ ExtendRow extend_row(const int64_t* positions, const int64_t* q_lens,
                                                const int64_t* rows, int n, int uniform_pos,
                                                int Sq, int slots, int max_len) {
  const int64_t p = positions ? positions[n] : (int64_t)uniform_pos;
  const int64_t len = q_lens ? q_lens[n] : (int64_t)Sq;
  const int64_t r = rows ? rows[n] : (int64_t)n;
  ExtendRow d;
  d.ok = r >= 0 && r < slots && p >= 0 && p < max_len && len >= 1 && len <= Sq &&
         p + len <= max_len;
  d.r = r;
  d.p = (int)p;
  d.len = (int)len;
  return d;
}

__device__ __forceinline__ unsigned short ae_bf16_bits(float x) {
  return __builtin_bit_cast(unsigned short, __float2bfloat16(x));
}

// ---- append -------------------------------------------------------------------
// grid (Sq, N).  A work item is one head's dim octet oct and its rotation
// partner: dims oct*8 .. +7 and 64 + oct*8 .. +7, two packets in, two out.
// Tokens past a row's length (and skipped rows) leave the cache alone and zero
// their q_rot, so the attention kernel never loads an uninitialised row.
// FP8: the 8 lanes of a head (consecutive idx, so one iteration and one aligned
// lane group) reduce the row's amax with three xor shuffles; V rows are work
// items of the same loop, unrotated.
template <bool FP8, bool PAGED>
__global__ __launch_bounds__(kExtendAppendThreads) LPP_NO_PACKED_F32 void attn_extend_append_kernel(
    const short* __restrict__ q,      // [N,Sq,H,128]
    const short* __restrict__ k_new,  // [N,Sq,Hkv,128]
    const short* __restrict__ v_new,
    std::conditional_t<FP8, uint8_t, short>* k_cache,  // [slots,Tmax,Hkv,128]
    std::conditional_t<FP8, uint8_t, short>* v_cache,
    float* k_scale,                   // [slots,Hkv,Tmax] (FP8)
    float* v_scale,
    const float* __restrict__ cos_t,  // [Smax,64]
    const float* __restrict__ sin_t,
    const int64_t* __restrict__ positions, const int64_t* __restrict__ q_lens,
    const int64_t* __restrict__ rows, int64_t* lengths,
    short* __restrict__ q_rot,        // [N,Sq,H,128]
    PageTable pt,                     // PAGED: the caches are the pool, slots the table's rows
    int uniform_pos, int max_len, int slots, int Tmax, int Sq, int H, int Hkv) {
  constexpr int HALF = ATTN_D / 2;
  const int i = blockIdx.x, n = blockIdx.y, tid = threadIdx.x;
  const ExtendRow row = extend_row(positions, q_lens, rows, n, uniform_pos, Sq, slots, max_len);
  const bool valid = row.ok && i < row.len;
  const int64_t tok = (int64_t)n * Sq + i;
  const short* qt = q + tok * H * ATTN_D;
  short* qo = q_rot + tok * H * ATTN_D;
  if (!valid) {
    const bf16x8 z = {0, 0, 0, 0, 0, 0, 0, 0};
    for (int idx = tid; idx < H * (ATTN_D / 8); idx += kExtendAppendThreads)
      reinterpret_cast<bf16x8*>(qo)[idx] = z;
    return;
  }
  const int pos = row.p + i;                       // < max_len <= min(Tmax, Smax)
  const short* kt = k_new + tok * Hkv * ATTN_D;
  const short* vt = v_new + tok * Hkv * ATTN_D;
  // kv head 0 of this token's row, in the slot or in the page of pos
  const KvRun run = kv_run<PAGED>(pt, row.r, Tmax, Hkv, 0, pos);
  const int64_t dst = run.kv + (int64_t)pos * Hkv * ATTN_D;
  const float* cr = cos_t + (int64_t)pos * HALF;
  const float* sr = sin_t + (int64_t)pos * HALF;

  // FP8: amax over the head's 8 lanes, this lane's two octets quantised and
  // stored, the scale by one lane
  [[maybe_unused]] auto store_row_fp8 = [&](const bf16x8& lo, const bf16x8& hi, auto* out,
                                            float* scale, int oct) LPP_NO_PACKED_F32 {
    float x[16], amax = 0.f;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      x[e] = bf16_to_f32(lo[e]);
      x[8 + e] = bf16_to_f32(hi[e]);
    }
#pragma unroll
    for (int e = 0; e < 16; ++e) amax = fmaxf(amax, fabsf(x[e]));
#pragma unroll
    for (int off = 1; off < 8; off <<= 1) amax = fmaxf(amax, __shfl_xor(amax, off));
    const int ex = fp8_row_exp(amax);
    const float inv = fp8_pow2(-ex);
    uint32_t w[4];
#pragma unroll
    for (int e = 0; e < 4; ++e)
      w[e] = fp8_pack2(__fmul_rn(x[4 * e], inv), __fmul_rn(x[4 * e + 1], inv)) |
             fp8_pack2(__fmul_rn(x[4 * e + 2], inv), __fmul_rn(x[4 * e + 3], inv)) << 16;
    *reinterpret_cast<uint2*>(out + oct * 8) = make_uint2(w[0], w[1]);
    *reinterpret_cast<uint2*>(out + HALF + oct * 8) = make_uint2(w[2], w[3]);
    if (oct == 0) *scale = fp8_pow2(ex);
  };

  constexpr int KV_ITEMS = FP8 ? 2 : 1;            // FP8: V rows are items of this loop
  for (int idx = tid; idx < (H + KV_ITEMS * Hkv) * 8; idx += kExtendAppendThreads) {
    const int head = idx >> 3, oct = idx & 7;
    const bool is_q = head < H;
    const bool is_v = FP8 && head >= H + Hkv;
    const int hk = head - H - (is_v ? Hkv : 0);    // kv head (!is_q)
    const short* src = is_q ? qt + head * ATTN_D : (is_v ? vt : kt) + hk * ATTN_D;
    const bf16x8 lo = *reinterpret_cast<const bf16x8*>(src + oct * 8);
    const bf16x8 hi = *reinterpret_cast<const bf16x8*>(src + HALF + oct * 8);
    // scale of (kv head hk, pos): kv heads are a page or a row apart
    [[maybe_unused]] const int64_t so = run.scale + hk * (int64_t)Tmax + pos;
    if (!is_q && !run.ok) continue;  // a table entry outside the pool: not stored
    if constexpr (FP8) {
      if (is_v) {
        store_row_fp8(lo, hi, v_cache + dst + hk * ATTN_D, v_scale + so, oct);
        continue;
      }
    }
    float cs[8], sn[8];
    *reinterpret_cast<float4*>(&cs[0]) = *reinterpret_cast<const float4*>(cr + oct * 8);
    *reinterpret_cast<float4*>(&cs[4]) = *reinterpret_cast<const float4*>(cr + oct * 8 + 4);
    *reinterpret_cast<float4*>(&sn[0]) = *reinterpret_cast<const float4*>(sr + oct * 8);
    *reinterpret_cast<float4*>(&sn[4]) = *reinterpret_cast<const float4*>(sr + oct * 8 + 4);
    bf16x8 olo, ohi;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const float a = bf16_to_f32(lo[e]), b = bf16_to_f32(hi[e]);
      olo[e] = (short)ae_bf16_bits(__fsub_rn(__fmul_rn(a, cs[e]), __fmul_rn(b, sn[e])));
      ohi[e] = (short)ae_bf16_bits(__fadd_rn(__fmul_rn(b, cs[e]), __fmul_rn(a, sn[e])));
    }
    if constexpr (FP8) {
      if (!is_q) {
        store_row_fp8(olo, ohi, k_cache + dst + hk * ATTN_D, k_scale + so, oct);
        continue;
      }
    }
    short* out;
    if constexpr (FP8) out = qo + head * ATTN_D;
    else out = is_q ? qo + head * ATTN_D : k_cache + dst + hk * ATTN_D;
    *reinterpret_cast<bf16x8*>(out + oct * 8) = olo;
    *reinterpret_cast<bf16x8*>(out + HALF + oct * 8) = ohi;
  }
  if constexpr (!FP8)
    for (int idx = tid; run.ok && idx < Hkv * (ATTN_D / 8); idx += kExtendAppendThreads)
      reinterpret_cast<bf16x8*>(v_cache + dst)[idx] = reinterpret_cast<const bf16x8*>(vt)[idx];
  if (lengths && i == 0 && tid == 0) lengths[row.r] = (int64_t)row.p + row.len;
}

// ---- attention ------------------------------------------------------------------
// grid (row blocks, chunks (1 when !SPLIT), N * Hkv), 512 threads, heaviest
// row block first.  2 waves/SIMD = one 512-thread workgroup per CU.
template <int REP, bool SPLIT, bool FP8, bool PAGED>
__global__ __launch_bounds__(512, 2) LPP_NO_PACKED_F32 void attn_extend_kernel(
    const short* __restrict__ Qr,  // q_rot [N,Sq,H,128]
    const std::conditional_t<FP8, uint8_t, short>* __restrict__ Kc,  // [slots,Tmax,Hkv,128]
    const std::conditional_t<FP8, uint8_t, short>* __restrict__ Vc,
    const float* __restrict__ Ks,  // [slots,Hkv,Tmax] (FP8)
    const float* __restrict__ Vs,
    short* __restrict__ O,         // [N,Sq,H,128]             (!SPLIT)
    float* __restrict__ WsO,       // [N*Hkv,J,R,128] fp32     (SPLIT)
    float* __restrict__ WsML,      // [N*Hkv,J,R,2]: m, l      (SPLIT)
    const int64_t* __restrict__ positions, const int64_t* __restrict__ q_lens,
    const int64_t* __restrict__ rows, PageTable pt, int uniform_pos, int max_len, int slots,
    int Tmax, int Sq, int Hkv, int J, int C, float c /* scale*log2e */) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  auto k_lds = [&](int buf) -> char* { return attn_img(smem, AE_K, buf); };
  auto v_lds = [&](int buf) -> char* { return attn_img(smem, AE_V, buf); };

  const int tid = threadIdx.x;
  const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);  // wave-uniform: scalar
  const int lane = tid & 63;
  const int lq = lane & 31;  // this lane's row (within the wave)
  const int hi2 = lane >> 5;

  const int blk = gridDim.x - 1 - blockIdx.x;  // long causal rows first
  const int j = blockIdx.y;
  const int nh = blockIdx.z, n = nh / Hkv, hkv = nh % Hkv;
  const int H = Hkv * REP, R = Sq * REP;
  const int64_t sHD = (int64_t)H * ATTN_D;
  const int64_t sHkvD = (int64_t)Hkv * ATTN_D;

  const ExtendRow row = extend_row(positions, q_lens, rows, n, uniform_pos, Sq, slots, max_len);
  const int r0 = blk * AE_QB;               // first row of this block
  const int rv = row.ok ? row.len * REP : 0;  // valid rows of this (n, kv head)

  // memory offset of row r: token r / REP, head hkv*REP + r % REP
  // (carries the kernel's target attribute: a lambda with other target
  // features is not inlined, and the call costs 64 bytes of scratch)
  auto row_off = [&](int r) LPP_NO_PACKED_F32 -> int64_t {
    return ((int64_t)n * Sq + r / REP) * sHD + (int64_t)(hkv * REP + r % REP) * ATTN_D;
  };

  if (r0 >= rv) {  // no valid row here (workgroup-uniform): o = 0
    if constexpr (!SPLIT) {
      const bf16x8 z = {0, 0, 0, 0, 0, 0, 0, 0};
      for (int idx = tid; idx < AE_QB * (ATTN_D / 8); idx += 512) {
        const int r = r0 + (idx >> 4);
        if (r < R) *reinterpret_cast<bf16x8*>(&O[row_off(r) + 8 * (idx & 15)]) = z;
      }
    }
    return;
  }
  const int p = row.p;
  // keys this block sees: 0 .. bound of its last valid row
  int kv_end = p + (min(r0 + AE_QB, rv) - 1) / REP + 1;
  int kv_begin = 0;
  if constexpr (SPLIT) {
    kv_begin = j * C;
    if (kv_begin >= kv_end) return;  // chunk starts past the last visible key
    kv_end = min(kv_end, kv_begin + C);
  }
  const int kv_last = p + row.len - 1;  // last key of the row: loads clamp here

  const int qw0 = r0 + wid * AE_QW;  // this wave's first row
  const int qrow = qw0 + lq;         // this lane's row
  const int bound = qrow < rv ? p + qrow / REP : -1;  // last visible key
  // wave-uniform: smallest bound (first row), largest (last valid row; -1: the
  // wave has no valid row and only stages), and whether it has invalid rows
  const int wb_min = p + qw0 / REP;
  const int wb_max = qw0 < rv ? p + (min(qw0 + AE_QW, rv) - 1) / REP : -1;
  const bool w_partial = qw0 + AE_QW > rv;

  // ---- Q B-fragments: qf[dc] = q_rot[row][dc*16 + hi2*8 .. +8] ----
  bf16x8 qf[8];
  {
    const int64_t rb = row_off(min(qrow, R - 1));
#pragma unroll
    for (int dc = 0; dc < 8; ++dc)
      qf[dc] = *reinterpret_cast<const bf16x8*>(&Qr[rb + dc * 16 + hi2 * 8]);
  }

  // ---- staging (per thread and pass: one K row-slice + one V row-slice) ----
  const int st_r = (lane >> 4);
  const int st_c = 8 * (lane & 15);
  const int st_off[2] = {attn_stage_off<32>(wid, 0, lane), attn_stage_off<32>(wid, 1, lane)};
  // key 0 of the row; PAGED: of the page of the tile ld_tile loads (run_cur) and
  // of the tile it will be asked for next (run_nxt), which is one tile on.  This
  // leans on attn_tile_pipeline's order of ld calls, stated at its definition.
  KvRun run_cur = kv_run<PAGED>(pt, row.r, Tmax, Hkv, hkv, kv_begin);
  [[maybe_unused]] KvRun run_nxt = run_cur;

  auto ld_tile = [&](int kv0, int pass, bf16x8& kreg, bf16x8& vreg) {
    if constexpr (PAGED) {
      if (pass == 0) {
        // tiles come in order (attn_tile_pipeline): take the entry fetched with
        // the tile before, fetch the next one alongside this tile's loads
        run_cur = run_nxt;
        run_nxt = kv_run<PAGED>(pt, row.r, Tmax, Hkv, hkv, min(kv0 + AE_KVB, kv_last));
      }
    }
    const int key = min(kv0 + stage_row(wid, pass, st_r), kv_last);
    const int64_t rb = run_cur.kv + (int64_t)key * sHkvD + st_c;
    if constexpr (FP8) {
      // the same 8 dims as 8 bytes, times the key's scale: exact in bf16
      const int64_t so = run_cur.scale + key;
      const uint2 kb = *reinterpret_cast<const uint2*>(&Kc[rb]);
      const uint2 vb = *reinterpret_cast<const uint2*>(&Vc[rb]);
      kreg = fp8x8_to_bf16(kb.x, kb.y, Ks[so]);
      vreg = fp8x8_to_bf16(vb.x, vb.y, Vs[so]);
    } else {
      kreg = *reinterpret_cast<const bf16x8*>(&Kc[rb]);
      vreg = *reinterpret_cast<const bf16x8*>(&Vc[rb]);
    }
  };
  auto write_tile = [&](int buf, int /*kv0*/, int pass, bf16x8 kreg, bf16x8 vreg) {
    stage_chunk(k_lds(buf), st_off[pass], kreg);
    stage_chunk(v_lds(buf), st_off[pass], vreg);
  };

  // ---- accumulators & softmax state ----
  f32x16 o_acc[4];
#pragma unroll
  for (int dt = 0; dt < 4; ++dt)
#pragma unroll
    for (int r = 0; r < 16; ++r) o_acc[dt][r] = 0.f;
  float m_run = -INFINITY, l_run = 0.f;

  attn_tile_pipeline<AE_KVB>(kv_begin, kv_end, ld_tile, write_tile, [&](int kv0, int cur) {
    // no row of this wave sees this tile (a scalar branch: the transposed
    // reads below need every lane active)
    if (kv0 > wb_max) return;
    // ---- S^T = K Q^T: two 32x32 tiles over keys ----
    f32x16 st[2];
#pragma unroll
    for (int t2 = 0; t2 < 2; ++t2)
#pragma unroll
      for (int r = 0; r < 16; ++r) st[t2][r] = 0.f;
    __builtin_amdgcn_s_setprio(1);
#pragma unroll
    for (int dc = 0; dc < 8; ++dc) {
#pragma unroll
      for (int t2 = 0; t2 < 2; ++t2) {
        const bf16x8 kf = read_row_frag(k_lds(cur), attn_row_off32(lane, t2, dc));
        st[t2] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(kf, qf[dc], st[t2], 0, 0, 0);
      }
    }
    __builtin_amdgcn_s_setprio(0);

    // ---- mask -> ms (unscaled scores, -inf where masked) ----
    // score reg r of tile t2 is key kv0 + t2*32 + crow32(r, hi2); keys past
    // kv_last (clamped loads) are past every bound
    float ms[32];
    const bool need_mask = (kv0 + AE_KVB - 1 > wb_min) || w_partial;
#pragma unroll
    for (int t2 = 0; t2 < 2; ++t2)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        float v = st[t2][r];
        if (need_mask) {
          const int kv = kv0 + t2 * 32 + crow32(r, hi2);
          if (kv > bound) v = -INFINITY;
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
    const float rm2 = pmax * c;

    // ---- defer-max decision (before exponentiation: the safe order) ----
    float m_new = m_run;
    if (__any(rm2 > m_run + AE_THR)) {
      m_new = fmaxf(m_run, rm2);
      const float alpha = (m_run == -INFINITY) ? 0.f : exp2f(m_run - m_new);
      l_run *= alpha;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const float ar =
            as_f(__builtin_amdgcn_ds_bpermute(crow32(r, hi2) * 4, as_i(alpha)));
#pragma unroll
        for (int dt = 0; dt < 4; ++dt) o_acc[dt][r] *= ar;
      }
      m_run = m_new;
    }

    // ---- P = exp2(ms*c - m_new); row sum; pack to PV A-fragments ----
    // A row that has seen no key yet (an invalid row, or one whose bound lies
    // before this chunk) has m_new = -inf and every ms = -inf; it subtracts 0
    // instead and gets p = exp2(-inf) = 0.
    float pr[32];
    float ps = 0.f;
    const float m_sub = (m_new == -INFINITY) ? 0.f : m_new;
#pragma unroll
    for (int i = 0; i < 32; ++i) {
      pr[i] = attn_exp2(fmaf(ms[i], c, -m_sub));
      ps += pr[i];
    }
    {
      int2v sw = __builtin_amdgcn_permlane32_swap(as_i(ps), as_i(ps), false, false);
      ps += as_f(hi2 ? sw[0] : sw[1]);
    }
    l_run += ps;

    bf16x8 pa[4];
    pack_pair(&pr[0], &pa[0]);
    pack_pair(&pr[16], &pa[2]);

    // ---- O += P V  (B-frags: transposed reads of the V image) ----
    __builtin_amdgcn_s_setprio(1);
#pragma unroll
    for (int dt = 0; dt < 4; ++dt) {
#pragma unroll
      for (int ks = 0; ks < 4; ++ks) {
        const bf16x8 bv = read_tr_frag(v_lds(cur), attn_tr_off32(lane, dt, ks, 0),
                                       attn_tr_off32(lane, dt, ks, 1));
        o_acc[dt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(pa[ks], bv, o_acc[dt], 0, 0, 0);
      }
    }
    __builtin_amdgcn_s_setprio(0);
  });

  if constexpr (SPLIT) {
    // ---- partials of the valid rows: unnormalised O, m, l ----
    const int64_t wb = ((int64_t)nh * J + j) * R;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int rr = qw0 + crow32(r, hi2);
      if (rr >= rv) continue;
      float* dst = WsO + (wb + rr) * ATTN_D;
#pragma unroll
      for (int dt = 0; dt < 4; ++dt) dst[dt * 32 + lq] = o_acc[dt][r];
    }
    if (hi2 == 0 && qrow < rv) {
      float* ml = WsML + (wb + qrow) * 2;
      ml[0] = m_run;
      ml[1] = l_run;
    }
  } else {
    // ---- redistribute 1/l, normalise, store O; invalid rows (l = 0) store 0 ----
    const float invl = (l_run > 0.f) ? 1.f / l_run : 0.f;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int rq = crow32(r, hi2);
      const float ir = as_f(__builtin_amdgcn_ds_bpermute(rq * 4, as_i(invl)));
      const int rr = qw0 + rq;
      if (rr >= R) continue;
      const int64_t rb = row_off(rr);
#pragma unroll
      for (int dt = 0; dt < 4; ++dt) O[rb + dt * 32 + lq] = f32_to_bf16(o_acc[dt][r] * ir);
    }
  }
}

// o[row, :] = sum_j O_j 2^(m_j - M) / sum_j l_j 2^(m_j - M) over the row's
// (p + token) / C + 1 chunks, in chunk order; every one of them holds a key
// the row sees, so every m_j is finite.  grid (R, N * Hkv), thread = dim.
__global__ __launch_bounds__(ATTN_D) LPP_NO_PACKED_F32 void attn_extend_combine_kernel(
    const float* __restrict__ WsO, const float* __restrict__ WsML,
    const int64_t* __restrict__ positions, const int64_t* __restrict__ q_lens,
    const int64_t* __restrict__ rows, short* __restrict__ O, int uniform_pos, int max_len,
    int slots, int Sq, int Hkv, int rep, int J, int C) {
  const int r = blockIdx.x, nh = blockIdx.y, d = threadIdx.x;
  const int n = nh / Hkv, hkv = nh % Hkv;
  const int R = Sq * rep, t = r / rep;
  const ExtendRow row = extend_row(positions, q_lens, rows, n, uniform_pos, Sq, slots, max_len);
  short* on = O + (((int64_t)n * Sq + t) * (Hkv * rep) + hkv * rep + r % rep) * ATTN_D;
  if (!row.ok || t >= row.len) {
    on[d] = 0;
    return;
  }
  const int nj = (row.p + t) / C + 1;  // <= J: p + t < max_len <= J*C
  float mx = kExtendMinM, lv = 0.f, a = 0.f;
  for (int jj = 0; jj < nj; ++jj) {
    const int64_t wr = ((int64_t)nh * J + jj) * R + r;
    const float mj = WsML[wr * 2];
    const float mn = fmaxf(mx, mj);
    const float f0 = exp2f(mx - mn), f1 = exp2f(mj - mn);
    a = a * f0 + WsO[wr * ATTN_D + d] * f1;
    lv = lv * f0 + WsML[wr * 2 + 1] * f1;
    mx = mn;
  }
  on[d] = f32_to_bf16(a / lv);
}

// Workgroup shape: 8 waves x 32 rows = 256 rows, one workgroup per CU, chosen
// over 4 waves x 2 workgroups: a staged K/V tile then serves twice the rows
// (half the LDS writes and global reads per row, and a whole 32-token chunk at
// REP = 8 in one workgroup), and the tile pipeline's staging (two passes of
// 512 threads) is used as it stands.  The accumulators, the scores and P of a
// 32-row wave need the 256-VGPR budget either way, so two workgroups of 4
// waves would share one CU only at half the registers.
// gfx950 (hipcc -O3): NumVgprs 204 for SPLIT=false at every REP, 206 (REP 1,
// 2) and 207 (REP 4, 8) for SPLIT=true; all ScratchSize 0, 2 waves/SIMD, 64 KB
// LDS, and the same figures for the FP8 instantiations (the conversion needs no
// register the bf16 load did not hold).  Append 48 VGPRs (FP8: 65), combine 12,
// no LDS, no scratch.  PAGED: 205 for SPLIT=false, 207 (REP 1, 2) and 208
// (REP 4, 8) for SPLIT=true, bf16 and FP8 alike, 6 to 9 more SGPRs (the two
// page bases), ScratchSize 0, 2 waves/SIMD; append 48 (FP8: 62).  The three kernels
// are LPP_NO_PACKED_F32: with packed fp32 the compiler pairs fp32 operations
// into v_pk_* instructions (274 in this file) and takes 208 / 210 VGPRs
// (append 58, combine 14) for the same arithmetic.  Nothing fails
// with packed fp32 on; the figures of profiles/README.md, Round 11, are of
// this machine code, and the packed form was not timed.
template <int REP, bool FP8, bool PAGED>
static void launch_extend(const at::Tensor& q_rot, const at::Tensor& k_cache,
                          const at::Tensor& v_cache, const float* k_scale,
                          const float* v_scale, at::Tensor& o, const int64_t* positions,
                          const int64_t* q_lens, const int64_t* rows, const PageTable& pt,
                          int slots, int uniform_pos, int max_len, int C, bool split) {
  const int N = q_rot.size(0), Sq = q_rot.size(1), H = q_rot.size(2);
  const int Hkv = H / REP, R = Sq * REP;
  const int Tmax = k_cache.size(1);
  const int nblk = (R + AE_QB - 1) / AE_QB;
  auto stream = current_stream();
  const short* qp = (const short*)q_rot.data_ptr();
  using cache_t = std::conditional_t<FP8, uint8_t, short>;
  const cache_t* kp = (const cache_t*)k_cache.data_ptr();
  const cache_t* vp = (const cache_t*)v_cache.data_ptr();
  const float c = attn_scale().c;
  if (!split) {
    hipLaunchKernelGGL((attn_extend_kernel<REP, false, FP8, PAGED>), dim3(nblk, 1, N * Hkv),
                       dim3(512), AE_LDS_BYTES, stream, qp, kp, vp, k_scale, v_scale,
                       (short*)o.data_ptr(), nullptr, nullptr, positions, q_lens, rows, pt,
                       uniform_pos, max_len, slots, Tmax, Sq, Hkv, 1, 0, c);
    LPP_CHECK_HIP(hipGetLastError());
    return;
  }
  const int J = (max_len + C - 1) / C;
  TORCH_CHECK(J <= 65535, "attention_extend: too many key chunks");
  auto ws_o = at::empty({(int64_t)N * Hkv, J, R, ATTN_D}, q_rot.options().dtype(at::kFloat));
  auto ws_ml = at::empty({(int64_t)N * Hkv, J, R, 2}, q_rot.options().dtype(at::kFloat));
  hipLaunchKernelGGL((attn_extend_kernel<REP, true, FP8, PAGED>), dim3(nblk, J, N * Hkv),
                     dim3(512), AE_LDS_BYTES, stream, qp, kp, vp, k_scale, v_scale, nullptr,
                     ws_o.data_ptr<float>(), ws_ml.data_ptr<float>(), positions, q_lens, rows, pt,
                     uniform_pos, max_len, slots, Tmax, Sq, Hkv, J, C, c);
  LPP_CHECK_HIP(hipGetLastError());
  hipLaunchKernelGGL(attn_extend_combine_kernel, dim3(R, N * Hkv), dim3(ATTN_D), 0, stream,
                     ws_o.data_ptr<float>(), ws_ml.data_ptr<float>(), positions, q_lens, rows,
                     (short*)o.data_ptr(), uniform_pos, max_len, slots, Sq, Hkv, REP, J, C);
  LPP_CHECK_HIP(hipGetLastError());
}

// True when [a, a + na) and [b, b + nb) (bytes) share no address.
static bool extend_disjoint(const void* a, size_t na, const void* b, size_t nb) {
  const char* ca = (const char*)a;
  const char* cb = (const char*)b;
  return ca + na <= cb || cb + nb <= ca;
}

static int64_t extend_chunk(int64_t chunk) {
  if (chunk == 0) return kExtendChunk;
  TORCH_CHECK(chunk == 64 || chunk == 128 || chunk == 256 || chunk == 512 || chunk == 1024,
              "attention_extend: chunk must be 0, 64, 128, 256, 512 or 1024");
  return chunk;
}

// attention_extend (FP8 = false, no scales) and attention_extend_fp8; PAGED
// with a block table (int32 [table_rows, max_pages]: the caches are a pool of
// 64-key pages and rows / lengths / N count table rows).
template <bool FP8, bool PAGED>
static at::Tensor extend(const char* who, const at::Tensor& q, const at::Tensor& k_new,
                         const at::Tensor& v_new, at::Tensor& k_cache, at::Tensor& v_cache,
                         at::Tensor* k_scale, at::Tensor* v_scale, const at::Tensor& cos_t,
                         const at::Tensor& sin_t, const c10::optional<at::Tensor>& positions,
                         const c10::optional<at::Tensor>& q_lens,
                         const c10::optional<at::Tensor>& rows,
                         const c10::optional<at::Tensor>& lengths, int64_t uniform_pos,
                         int64_t max_len, int64_t chunk, int64_t split,
                         const c10::optional<at::Tensor>& block_table) {
  using cache_t = std::conditional_t<FP8, uint8_t, short>;
  TORCH_CHECK(q.is_cuda() && q.scalar_type() == at::kBFloat16, who, ": bf16 CUDA q required");
  TORCH_CHECK(q.dim() == 4 && q.size(1) >= 1 && q.size(3) == ATTN_D, who,
              ": q must be [N,Sq,H,128]");
  const int64_t N = q.size(0), Sq = q.size(1), H = q.size(2);
  TORCH_CHECK(k_new.dim() == 4 && k_new.size(0) == N && k_new.size(1) == Sq &&
                  k_new.size(3) == ATTN_D && v_new.sizes() == k_new.sizes(),
              who, ": k_new/v_new must be [N,Sq,Hkv,128]");
  const int64_t Hkv = k_new.size(2);
  TORCH_CHECK(Hkv >= 1 && H % Hkv == 0, who, ": H must be a multiple of Hkv");
  TORCH_CHECK(k_cache.dim() == 4 && k_cache.size(2) == Hkv && k_cache.size(3) == ATTN_D &&
                  v_cache.sizes() == k_cache.sizes(),
              who, ": caches must be [slots,Tmax,Hkv,128]");
  for (const at::Tensor* t : {&k_new, &v_new, (const at::Tensor*)&k_cache,
                              (const at::Tensor*)&v_cache})
    TORCH_CHECK(t->is_cuda() && t->is_contiguous() && t->device() == q.device() &&
                    t->scalar_type() == (FP8 && (t == &k_cache || t == &v_cache)
                                             ? at::kFloat8_e4m3fn
                                             : at::kBFloat16),
                who, ": k/v tensors must be contiguous bf16", FP8 ? " (the caches e4m3)" : "",
                " on q's device");
  TORCH_CHECK(q.is_contiguous(), who, ": q must be contiguous");
  for (const at::Tensor* t : {&cos_t, &sin_t})
    TORCH_CHECK(t->is_cuda() && t->scalar_type() == at::kFloat && t->is_contiguous() &&
                    t->dim() == 2 && t->size(1) == ATTN_D / 2 && t->device() == q.device(),
                who, ": cos/sin must be contiguous fp32 [Smax,64]");
  TORCH_CHECK(cos_t.size(0) == sin_t.size(0), who, ": cos/sin length mismatch");
  const int64_t Tmax = k_cache.size(1);
  int64_t slots = k_cache.size(0), row_tokens = Tmax;  // rows of the cache, tokens of a row
  PageTable pt{nullptr, 0, 0};
  if constexpr (PAGED) {
    const at::Tensor& t = *block_table;
    TORCH_CHECK(Tmax == kPageTokens, who, ": a paged cache is [num_pages,", kPageTokens,
                ",Hkv,128], got ", Tmax, " tokens per page");
    TORCH_CHECK(t.is_cuda() && t.device() == q.device() && t.scalar_type() == at::kInt &&
                    t.is_contiguous() && t.dim() == 2 && t.size(0) >= 1 && t.size(1) >= 1,
                who, ": block_table must be a contiguous int32 [table_rows,max_pages] on q's "
                     "device");
    TORCH_CHECK(slots >= 1 && slots < ((int64_t)1 << 31) / kPageTokens &&
                    t.size(0) < ((int64_t)1 << 31) && t.size(1) < ((int64_t)1 << 31) / kPageTokens,
                who, ": pool or block_table out of range");
    pt = PageTable{t.data_ptr<int>(), (int)t.size(1), (int)slots};
    slots = t.size(0);
    row_tokens = t.size(1) * kPageTokens;
    // read by every launch while the append writes the caches and lengths
    std::vector<const at::Tensor*> written = {&k_cache, &v_cache};
    if (lengths.has_value()) written.push_back(&lengths.value());
    if constexpr (FP8) written.insert(written.end(), {k_scale, v_scale});
    for (const at::Tensor* u : written)
      TORCH_CHECK(lpp::extend_disjoint(t.data_ptr(), t.nbytes(), u->data_ptr(), u->nbytes()), who,
                  ": block_table must not alias lengths, the scales or the caches");
  }
  TORCH_CHECK(max_len >= 1 && max_len <= row_tokens && max_len <= cos_t.size(0), who,
              ": max_len ", max_len, " must be in [1, min(", PAGED ? "max_pages * 64" : "Tmax",
              ", rope table)]");
  TORCH_CHECK(k_cache.numel() < ((int64_t)1 << 40) && q.numel() < ((int64_t)1 << 40) &&
                  N <= 65535 && N * Hkv <= 65535 && Sq * H < ((int64_t)1 << 30),
              who, ": shape out of range");  // grid y/z limits; 64-bit offsets beyond
  TORCH_CHECK(split >= -1 && split <= 1, who, ": split must be -1, 0 or 1");
  const int64_t C = lpp::extend_chunk(chunk);

  auto check_index = [&](const c10::optional<at::Tensor>& t, int64_t numel, const char* name) {
    if (!t.has_value()) return;
    TORCH_CHECK(t->is_cuda() && t->device() == q.device() &&
                    t->scalar_type() == at::kLong && t->is_contiguous() && t->dim() == 1 &&
                    t->numel() == numel,
                who, ": ", name, " must be a contiguous int64 [", numel, "] on q's device");
  };
  check_index(positions, N, "positions");
  check_index(q_lens, N, "q_lens");
  check_index(rows, N, "rows");
  check_index(lengths, slots, "lengths");
  if (!rows.has_value()) TORCH_CHECK(N <= slots, who, ": N > slots needs rows");
  if (!positions.has_value())
    TORCH_CHECK(uniform_pos >= 0 && uniform_pos + (q_lens.has_value() ? 1 : Sq) <= max_len, who,
                ": uniform_pos out of range");
  if (lengths.has_value())
    // the attention kernel and the combine read the metadata after the append
    // stored lengths[r]
    for (const c10::optional<at::Tensor>* t : {&positions, &q_lens, &rows})
      if (t->has_value())
        TORCH_CHECK(lpp::extend_disjoint((*t)->data_ptr(), (*t)->nbytes(), lengths->data_ptr(),
                                         lengths->nbytes()),
                    who, ": positions/q_lens/rows must not alias lengths");
  for (const at::Tensor* cc : {&k_cache, &v_cache})
    for (const at::Tensor* t : {&q, &k_new, &v_new})
      TORCH_CHECK(lpp::extend_disjoint(cc->data_ptr(), cc->nbytes(), t->data_ptr(), t->nbytes()),
                  who, ": q/k_new/v_new must not alias the caches");
  TORCH_CHECK(lpp::extend_disjoint(k_cache.data_ptr(), k_cache.nbytes(), v_cache.data_ptr(),
                                   v_cache.nbytes()),
              who, ": k_cache and v_cache must not alias");
  float* ksp = nullptr;
  float* vsp = nullptr;
  if constexpr (FP8) {
    for (const at::Tensor* t : {k_scale, v_scale}) {
      TORCH_CHECK(t->is_cuda() && t->device() == q.device() && t->scalar_type() == at::kFloat &&
                      t->is_contiguous() && t->dim() == 3 && t->size(0) == k_cache.size(0) &&
                      t->size(1) == Hkv && t->size(2) == Tmax,
                  who, ": k_scale/v_scale must be contiguous fp32 [slots,Hkv,Tmax] on q's device");
      // written by the append while later launches read every other argument
      std::vector<const at::Tensor*> others = {&q, &k_new, &v_new, &k_cache, &v_cache, &cos_t,
                                               &sin_t};
      for (const c10::optional<at::Tensor>* u : {&positions, &q_lens, &rows, &lengths})
        if (u->has_value()) others.push_back(&u->value());
      if (t == v_scale) others.push_back(k_scale);
      for (const at::Tensor* u : others)
        TORCH_CHECK(lpp::extend_disjoint(t->data_ptr(), t->nbytes(), u->data_ptr(), u->nbytes()),
                    who, ": k_scale/v_scale must not alias another argument");
    }
    ksp = k_scale->data_ptr<float>();
    vsp = v_scale->data_ptr<float>();
  }

  auto o = at::empty_like(q);
  if (N == 0) return o;
  const int64_t* pp = positions.has_value() ? positions->data_ptr<int64_t>() : nullptr;
  const int64_t* qp = q_lens.has_value() ? q_lens->data_ptr<int64_t>() : nullptr;
  const int64_t* rp = rows.has_value() ? rows->data_ptr<int64_t>() : nullptr;
  int64_t* lp = lengths.has_value() ? lengths->data_ptr<int64_t>() : nullptr;
  const int rep = (int)(H / Hkv);
  TORCH_CHECK(rep == 1 || rep == 2 || rep == 4 || rep == 8, who,
              ": H/Hkv must be 1, 2, 4 or 8, got ", rep);  // before the cache is written

  auto q_rot = at::empty_like(q);
  hipLaunchKernelGGL((lpp::attn_extend_append_kernel<FP8, PAGED>), dim3((unsigned)Sq, (unsigned)N),
                     dim3(lpp::kExtendAppendThreads), 0, lpp::current_stream(),
                     (const short*)q.data_ptr(), (const short*)k_new.data_ptr(),
                     (const short*)v_new.data_ptr(), (cache_t*)k_cache.data_ptr(),
                     (cache_t*)v_cache.data_ptr(), ksp, vsp, cos_t.data_ptr<float>(),
                     sin_t.data_ptr<float>(), pp, qp, rp, lp, (short*)q_rot.data_ptr(), pt,
                     (int)uniform_pos, (int)max_len, (int)slots, (int)Tmax, (int)Sq, (int)H,
                     (int)Hkv);
  LPP_CHECK_HIP(hipGetLastError());

  const bool do_split = split < 0 ? Sq * rep < lpp::kExtendSplitRows : split == 1;
#define LPP_EXTEND_REP(RR)                                                                  \
  case RR:                                                                                  \
    lpp::launch_extend<RR, FP8, PAGED>(q_rot, k_cache, v_cache, ksp, vsp, o, pp, qp, rp,    \
                                       pt, (int)slots, (int)uniform_pos, (int)max_len,      \
                                       (int)C, do_split);                                   \
    break
  switch (rep) {
    LPP_EXTEND_REP(1);
    LPP_EXTEND_REP(2);
    LPP_EXTEND_REP(4);
    LPP_EXTEND_REP(8);
    default:
      TORCH_CHECK(false, who, ": H/Hkv must be 1, 2, 4 or 8, got ", rep);
  }
#undef LPP_EXTEND_REP
  return o;
}

}  // namespace lpp

using lpp::ATTN_D;

// Keys per split workgroup: the compiled-in C (chunk = 0) or a checked override.
int64_t attention_extend_chunk(int64_t chunk) { return lpp::extend_chunk(chunk); }

// chunk: 0 = the compiled-in C, or one of 64 .. 1024 (tests, the C sweep of
// scripts/extend_bench.py).  split: -1 = by the row count (Sq * H/Hkv below
// kExtendSplitRows), 0 / 1 force the direct / the split path.  Results differ
// in the last bits between chunk sizes and paths, never between calls of one.
// block_table: the paged layout (attn_paged.h); the same paths and bits.
at::Tensor attention_extend(at::Tensor q, at::Tensor k_new, at::Tensor v_new,
                            at::Tensor k_cache, at::Tensor v_cache, at::Tensor cos_t,
                            at::Tensor sin_t, c10::optional<at::Tensor> positions,
                            c10::optional<at::Tensor> q_lens, c10::optional<at::Tensor> rows,
                            c10::optional<at::Tensor> lengths, int64_t uniform_pos,
                            int64_t max_len, int64_t chunk, int64_t split,
                            c10::optional<at::Tensor> block_table) {
  const char* who = "attention_extend";
  if (block_table.has_value())
    return lpp::extend<false, true>(who, q, k_new, v_new, k_cache, v_cache, nullptr, nullptr,
                                    cos_t, sin_t, positions, q_lens, rows, lengths, uniform_pos,
                                    max_len, chunk, split, block_table);
  return lpp::extend<false, false>(who, q, k_new, v_new, k_cache, v_cache, nullptr, nullptr,
                                   cos_t, sin_t, positions, q_lens, rows, lengths, uniform_pos,
                                   max_len, chunk, split, block_table);
}

// The same over e4m3 caches with per-(slot, kv head, token) scales.
at::Tensor attention_extend_fp8(at::Tensor q, at::Tensor k_new, at::Tensor v_new,
                                at::Tensor k_cache, at::Tensor v_cache, at::Tensor k_scale,
                                at::Tensor v_scale, at::Tensor cos_t, at::Tensor sin_t,
                                c10::optional<at::Tensor> positions,
                                c10::optional<at::Tensor> q_lens,
                                c10::optional<at::Tensor> rows,
                                c10::optional<at::Tensor> lengths, int64_t uniform_pos,
                                int64_t max_len, int64_t chunk, int64_t split,
                                c10::optional<at::Tensor> block_table) {
  const char* who = "attention_extend_fp8";
  if (block_table.has_value())
    return lpp::extend<true, true>(who, q, k_new, v_new, k_cache, v_cache, &k_scale, &v_scale,
                                   cos_t, sin_t, positions, q_lens, rows, lengths, uniform_pos,
                                   max_len, chunk, split, block_table);
  return lpp::extend<true, false>(who, q, k_new, v_new, k_cache, v_cache, &k_scale, &v_scale,
                                  cos_t, sin_t, positions, q_lens, rows, lengths, uniform_pos,
                                  max_len, chunk, split, block_table);
}
