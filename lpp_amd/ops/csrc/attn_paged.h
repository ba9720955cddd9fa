// Paged KV cache: where a key's row lives, in the slot layout and in the paged
// one, for the decode and extend attention kernels (gfx950).
//
// Slot layout: k/v [slots, Tmax, Hkv, 128], scales [slots, Hkv, Tmax]; key t of
// cache row r is cache[r, t].
// Paged layout: the pool k/v [num_pages, 64, Hkv, 128], scales [num_pages, Hkv,
// 64], and block_table int32 [table_rows, max_pages]; key t of table row r is
// cache[block_table[r, t >> 6], t & 63].
//
// A page holds kPageTokens = 64 keys: one extend tile, two 32-key steps of the
// MFMA decode kernels, so the keys a wave touches in one step or tile share a
// page and the page id is wave-uniform.  kv_run() therefore answers for a run
// of keys, not for one: it returns the offset of the run's (virtual) key 0, and
// the caller adds key * Hkv * 128 (or key, for a scale) per lane exactly as it
// does in the slot layout, for every key of the page that holds `key`.  The
// table entry is read with a scalar load and the base formed in SGPRs; the
// per-lane address arithmetic does not know which layout it runs on.
//
// Whatever the table holds, nothing outside the pool is addressed: an id
// outside [0, num_pages) is clamped for loads, and KvRun::ok tells a store to
// stay away.
#pragma once

#include "attention.h"

namespace lpp {

constexpr int kPageTokens = ATTN_TILE_ROWS;  // keys per page
constexpr int kPageShift = 6;
static_assert(kPageTokens == 1 << kPageShift, "a page is one 64-key tile");

struct PageTable {
  const int* table;  // [table_rows, max_pages]; null in the slot layout
  int max_pages;
  int num_pages;
};

struct KvRun {
  int64_t kv;     // element offset of key 0 in k_cache / v_cache, kv head included
  int64_t scale;  // offset of key 0 in k_scale / v_scale
  bool ok;        // the page exists: stores may go ahead
};

// The run of keys that holds `key` (wave-uniform; key < max_pages * 64 when
// PAGED) of row r, kv head hkv.  T is the cache's second dimension.
template <bool PAGED>
__device__ __forceinline__ KvRun kv_run(const PageTable& pt, int64_t r, int T, int Hkv, int hkv,
                                        int key) {
  KvRun run;
  if constexpr (!PAGED) {
    run.kv = ((r * T) * (int64_t)Hkv + hkv) * ATTN_D;
    run.scale = (r * Hkv + hkv) * (int64_t)T;
    run.ok = true;
  } else {
    const int ukey = __builtin_amdgcn_readfirstlane(key);
    const int id =
        __builtin_amdgcn_readfirstlane(pt.table[r * pt.max_pages + (ukey >> kPageShift)]);
    run.ok = (unsigned)id < (unsigned)pt.num_pages;
    const int64_t page = id < 0 ? 0 : (id < pt.num_pages ? id : pt.num_pages - 1);
    const int key0 = ukey & ~(kPageTokens - 1);  // first key of the page
    run.kv = ((page * kPageTokens - key0) * Hkv + hkv) * ATTN_D;
    run.scale = (page * Hkv + hkv) * kPageTokens - key0;
  }
  return run;
}

// The runs of a decode wave's KPW consecutive keys from wave0 (KPW 32, 64 or
// 128: one or two pages), looked up once, ahead of the key loop.  The key is
// clamped to p before the lookup: no table entry past the page of key p is read.
template <bool PAGED, int KPW>
struct DecodeRuns {
  static constexpr int N = PAGED && KPW > kPageTokens ? KPW / kPageTokens : 1;
  static_assert(N <= 2, "a wave's keys span at most two pages");
  KvRun run[N];

  __device__ __forceinline__ DecodeRuns(const PageTable& pt, int64_t r, int T, int Hkv, int hkv,
                                        int wave0, int p) {
#pragma unroll
    for (int i = 0; i < N; ++i) {
      const int key = wave0 + i * kPageTokens;
      run[i] = kv_run<PAGED>(pt, r, T, Hkv, hkv, key < p ? key : p);
    }
  }
  // of the step that starts off keys into the wave's range (wave0 + off <= p)
  __device__ __forceinline__ const KvRun& at(int off) const {
    if constexpr (N == 1) return run[0];
    else return off >= kPageTokens ? run[1] : run[0];
  }
};

}  // namespace lpp
