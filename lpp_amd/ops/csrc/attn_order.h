// Block order of the causal attention kernels (forward, dQ, dK/dV).
//
// The kernels launch a 1-D grid of n = nblk * nheads workgroups and map the
// linear id L to (causal block, head) through attn_block_order().
// Workgroups are observed to be dealt round-robin over the 8 XCDs (ids L and
// L+8 share an XCD and its L2), which costs the plain
// (blk = L % nblk, head = L / nblk) order twice:
//   - locality: a head's causal blocks land on all 8 XCDs, so every L2
//     fetches every head's K/V (Q/dO for dK/dV) - 8x the traffic needed;
//   - balance: a causal block's work grows linearly with its index (fwd/dQ:
//     block x runs x+1 KV steps; dK/dV: block x runs nblk-x q steps) and label
//     k gets the same blocks of every head, e.g. {k, k+8} = 2k+10 units per
//     head for fwd/dQ at nblk=16, a 1.41x max/mean skew.
// Measured on MI355X (profiles/README.md, Round 3) the first is worth ~1.7x
// per kernel, the second a few percent.
//
// Mode 1 fixes both.  Label k's ids, taken in increasing L, walk one
// contiguous chunk of a virtual order j (the bijective XCD remap, valid for
// any n); the virtual order runs through groups of G whole heads,
// block-major and heaviest block first inside a group.  Every label
// therefore works through whole heads (one L2 serves a head), starts its
// heavy blocks first and fills the tail with the lightest ones.  Placement
// is a speed matter only: which workgroup computes which tile changes, the
// tile's arithmetic does not, and no result depends on where a block lands.
//
// The same function runs on the host (attention_block_order binding, tests)
// and on the device, so the tested order is the launched order.
#pragma once

#if defined(__HIP__) || defined(__CUDACC__)
#define LPP_HD __host__ __device__
#else
#define LPP_HD
#endif

namespace lpp {

constexpr int ATTN_XCDS = 8;

enum AttnOrderKind : int {
  ATTN_ORDER_FWD_DQ = 0,  // larger blk = more work
  ATTN_ORDER_DKDV = 1,    // larger blk = less work
};

struct AttnBlock {
  int blk;
  int head;
};

// L in [0, nblk*nheads) -> (blk, head).  mode 0: legacy order, exactly the
// dispatch order of a dim3(nblk, nheads) grid.  mode 1: XCD-chunked,
// heavy-first, G heads per group (the last group may be short).
LPP_HD inline AttnBlock attn_block_order(int L, int nblk, int nheads, int G, int kind,
                                         int mode) {
  if (mode == 0) return {L % nblk, L / nblk};
  const int n = nblk * nheads;
  const int xcd = L % ATTN_XCDS;
  const int q = n / ATTN_XCDS, r = n % ATTN_XCDS;
  const int j = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + L / ATTN_XCDS;
  if (G < 1) G = 1;
  if (G > nheads) G = nheads;
  const int grp = j / (G * nblk), rem = j % (G * nblk);
  const int Gl = G < nheads - grp * G ? G : nheads - grp * G;
  const int rank = rem / Gl;  // rank-th most work
  return {kind == ATTN_ORDER_FWD_DQ ? nblk - 1 - rank : rank, grp * G + rem % Gl};
}

// Resident workgroups per XCD: 32 CUs x one 512-thread workgroup per CU.  All
// three attention kernels need more than 128 VGPRs, so they run at
// 2 waves/SIMD, which one 8-wave workgroup fills.
constexpr int ATTN_RESIDENT_PER_XCD = 32;
// The launches size a group to span this many resident waves of workgroups.
// Measured, not derived (G sweeps at B=4, S=4096, H=64, profiles/README.md
// Round 4): fwd and dQ (nblk 16) are best at G = 8, dK/dV (nblk 32) at G = 4,
// i.e. 4 waves each; the one-wave G is 7-9% slower, the two-wave G 0.4-2%.
constexpr int ATTN_GROUP_WAVES = 4;

// Heads per group: the groups that `resident_per_xcd` workgroups span, rounded
// up to whole heads.
inline int attn_order_group(int resident_per_xcd, int nblk) {
  const int g = (resident_per_xcd + nblk - 1) / nblk;
  return g < 1 ? 1 : g;
}

// The order each kernel runs under process mode 1: the measured winner per
// kernel (profiles/README.md, Round 3).  0 = that kernel keeps the legacy order.
constexpr int ATTN_MODE1_FWD = 1;
constexpr int ATTN_MODE1_DQ = 1;
constexpr int ATTN_MODE1_DKDV = 1;

}  // namespace lpp
