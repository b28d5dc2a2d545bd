// search1.hip — the reduction of the one-ply search: the best child of every
// STAR group (fnnue_best_children_device, include/fnnue.h), i.e. the chess rule
// of the backend's move work (backend.cpp fill_roots) on the device.
//
// A group averages about 35 children and has at most 219 records, so a wave
// per group would idle half its lanes: 32 lanes (half a wave) share a group.
// Each lane folds the children lane, lane + 32, ... into one 64-bit key
//   rank (2 mate in one, 1 everything else, 0 a child the mover has lost by
//   playing: FNNUE_END_WON) << 62 | (value + 2^29) << 32 | ~index
// (|value| <= 2^28: the sum of two int32 over 16), so that the largest key is
// the first maximum whatever lane saw it; five xor-shuffles inside the half
// wave leave it in every lane, and lanes 0-5 store one dword each of the
// 24-byte record.  No atomics, no LDS, no host synchronisation.
// The k best children of every group (fnnue_topk_children_device, MultiPV):
// topk_children_kernel below, the same key ranked by counting in LDS.
// The second reduction of the two-ply search (fnnue_best_replies_device):
// best_replies_kernel below, the same shape over the children's own records;
// vbest_replies_kernel with the variants' five ranks (fnnue_vbest_replies_device).
// The k best lines of every ply at two plies (fnnue_topk_replies_device):
// topk_replies_kernel, the second reduction's key ranked by counting in LDS.
#include <hip/hip_runtime.h>

#include "builder.h"

namespace fnnue {

namespace {

constexpr uint32_t kGroupLanes = 32, kBlock = 256;
static_assert(sizeof(fnnue_best) == 24, "fnnue_best is six dwords");

// A child's key by the rule of the backend's move work (backend.cpp
// fill_roots): lost at once (rank 0, worth 0), no legal move and decided
// (check, exploded king, the variant's rule: rank 2), no legal move alone
// (worth 0), anything else its negated evaluation.  Never 0 (~index).
__device__ __forceinline__ unsigned long long child_key(const int32_t* __restrict__ psqt,
                                                        const int32_t* __restrict__ positional,
                                                        const uint8_t* __restrict__ end, uint32_t o, uint32_t c) {
  const uint32_t x = o + c;
  const uint32_t f = end[x];
  uint32_t rank = 1;
  int32_t v = 0;
  if (f & kFinalWon) {
    rank = 0;
  } else if (f & (kFinalNoMoves | kFinalDraw)) {
    // mate in one / stalemate or a drawn record (kFinalDraw: worth 0 like a stalemate; a mate stays a mate)
    rank = ((f & kFinalNoMoves) && (f & (kFinalCheck | kFinalExtinct | kFinalVariant))) ? 2u : 1u;
  } else {
    v = (int32_t)-(((long long)psqt[x] + (long long)positional[x]) / 16);
  }
  return (unsigned long long)rank << 62 | (unsigned long long)(uint32_t)(v + (1 << 29)) << 32 | (0xFFFFFFFFu - c);
}
__device__ __forceinline__ uint32_t key_kind(unsigned long long key) {
  const uint32_t rank = (uint32_t)(key >> 62);
  return rank == 2 ? FNNUE_BEST_MATE : rank == 0 ? FNNUE_BEST_LOST : FNNUE_BEST_CP;
}

// kOwnTerms (the two-ply search's children): a group without a child stores its
// own first record's terms as they are instead of zeros (fnnue_best_replies).
template <bool kOwnTerms>
__global__ __launch_bounds__(kBlock) void best_children_kernel(
    const int32_t* __restrict__ psqt, const int32_t* __restrict__ positional, const uint8_t* __restrict__ end,
    const uint16_t* __restrict__ moves, const uint32_t* __restrict__ off, uint32_t ngroups, uint32_t npos,
    uint32_t* __restrict__ out) {
  const uint64_t t = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
  const uint32_t g = (uint32_t)(t / kGroupLanes), lane = (uint32_t)(t % kGroupLanes);
  const bool live = g < ngroups;  // no early return: the shuffles below run with the whole wave
  uint32_t o = 0, e = 0;
  if (live) {
    e = min(off[g + 1], npos);
    o = min(off[g], e);
  }
  const uint32_t nrec = e - o;
  unsigned long long key = 0;  // 0: no child (a child's key is never 0: ~index)
  for (uint32_t c = 1 + lane; c < nrec; c += kGroupLanes) {
    const unsigned long long k = child_key(psqt, positional, end, o, c);
    key = k > key ? k : key;
  }
#pragma unroll
  for (int m = kGroupLanes / 2; m >= 1; m >>= 1) {
    const unsigned long long other = (unsigned long long)__shfl_xor((long long)key, m, kGroupLanes);
    key = other > key ? other : key;
  }
  const uint32_t best = key ? 0xFFFFFFFFu - (uint32_t)key : 0u;
  const int32_t value = (int32_t)((uint32_t)(key >> 32) & 0x3FFFFFFFu) - (1 << 29);
  uint32_t w = 0;
  if (nrec) {  // an empty group: all zero
    const uint32_t kind = !best ? FNNUE_BEST_NONE : key_kind(key);
    switch (lane) {
      case 0: w = best ? 0u - (uint32_t)psqt[o + best] : kOwnTerms ? (uint32_t)psqt[o] : 0u; break;  // negated, wrapping
      case 1: w = best ? 0u - (uint32_t)positional[o + best] : kOwnTerms ? (uint32_t)positional[o] : 0u; break;
      case 2: w = kind == FNNUE_BEST_CP ? (uint32_t)value : 0u; break;
      case 3: w = nrec - 1; break;
      case 4: w = best; break;
      case 5: w = (best && moves ? (uint32_t)moves[o + best] : 0u) | kind << 16 | (uint32_t)end[o] << 24; break;
      default: break;
    }
  }
  if (live && lane < 6) out[(size_t)g * 6 + lane] = w;
}

// ---- the k best children per group (fnnue_topk_children_device, MultiPV) ----
// The same half wave per group and the same key, extended to a total order:
// the keys of a group are unique (~index), so the number of keys larger than a
// child's own is its place in the descending order.  Rank by counting: each
// half wave stages its keys once in LDS; every lane keeps up to kTopkRegs keys
// of its own in registers (children lane + 1, lane + 33, ...: static indexing)
// and reads each key of the group by a same-address ds_read_b64 (a broadcast:
// no bank conflict), counting those above its own.  A child whose count is
// below the group's slot count writes its own 20-byte line at that slot.  No
// sorting network, no dependent reduction rounds, and the cost does not depend
// on the slot count.  Groups beyond kTopkFast children (variant nets, hand-made
// input) recompute every key from global memory instead: correct, not fast.
constexpr uint32_t kTopkRegs = 8, kTopkFast = kGroupLanes * kTopkRegs, kTopkGroups = kBlock / kGroupLanes;
static_assert(sizeof(fnnue_line) == 20, "fnnue_line is five dwords");
static_assert(kTopkFast >= FNNUE_MAX_CHILDREN, "every chess ply takes the fast path");

__device__ __forceinline__ void write_line(uint32_t* __restrict__ lines, uint64_t slot, unsigned long long key,
                                           const int32_t* __restrict__ psqt, const int32_t* __restrict__ positional,
                                           const uint16_t* __restrict__ moves, uint32_t o) {
  const uint32_t c = 0xFFFFFFFFu - (uint32_t)key;
  const uint32_t kind = key_kind(key);
  const int32_t value = (int32_t)((uint32_t)(key >> 32) & 0x3FFFFFFFu) - (1 << 29);
  uint32_t* w = lines + slot * 5;
  w[0] = 0u - (uint32_t)psqt[o + c];  // negated, wrapping
  w[1] = 0u - (uint32_t)positional[o + c];
  w[2] = kind == FNNUE_BEST_CP ? (uint32_t)value : 0u;
  w[3] = c;
  w[4] = (moves ? (uint32_t)moves[o + c] : 0u) | kind << 16;
}

__global__ __launch_bounds__(kBlock) void topk_children_kernel(
    const int32_t* __restrict__ psqt, const int32_t* __restrict__ positional, const uint8_t* __restrict__ end,
    const uint16_t* __restrict__ moves, const uint32_t* __restrict__ off, uint32_t ngroups, uint32_t npos,
    const uint32_t* __restrict__ line_off, uint32_t uniform_k, uint32_t* __restrict__ lines, uint64_t lines_cap) {
  __shared__ unsigned long long staged[kTopkGroups][kTopkFast];
  const uint32_t hw = threadIdx.x / kGroupLanes, lane = threadIdx.x % kGroupLanes;
  const uint64_t g64 = (uint64_t)blockIdx.x * kTopkGroups + hw;
  const bool live = g64 < ngroups;  // no early return: the barrier below runs with the whole block
  const uint32_t g = (uint32_t)g64;
  uint32_t o = 0, e = 0;
  uint64_t lo = 0, k = 0;  // the group's slots [lo, lo + k), cut at lines_cap
  if (live) {
    e = min(off[g + 1], npos);
    o = min(off[g], e);
    if (line_off) {
      lo = line_off[g];
      const uint64_t hi = line_off[g + 1];
      k = hi > lo ? hi - lo : 0;
    } else {
      lo = (uint64_t)g * uniform_k;
      k = uniform_k;
    }
    k = lo < lines_cap ? min(k, lines_cap - lo) : 0;
  }
  const uint32_t nrec = e - o;
  const uint32_t nkids = nrec && k ? nrec - 1 : 0;  // nothing to rank without a slot
  const bool fast = nkids <= kTopkFast;
  unsigned long long key[kTopkRegs];
#pragma unroll
  for (uint32_t i = 0; i < kTopkRegs; ++i) {
    const uint32_t q = lane + kGroupLanes * i;  // child q + 1
    key[i] = 0;
    if (fast && q < nkids) {
      key[i] = child_key(psqt, positional, end, o, q + 1);
      staged[hw][q] = key[i];
    }
  }
  __syncthreads();
  if (fast) {
    uint32_t above[kTopkRegs];
#pragma unroll
    for (uint32_t i = 0; i < kTopkRegs; ++i) above[i] = 0;
    for (uint32_t q = 0; q < nkids; ++q) {
      const unsigned long long other = staged[hw][q];  // the same address in every lane of the half wave
#pragma unroll
      for (uint32_t i = 0; i < kTopkRegs; ++i) above[i] += other > key[i] ? 1u : 0u;
    }
#pragma unroll
    for (uint32_t i = 0; i < kTopkRegs; ++i)
      if (key[i] && above[i] < k) write_line(lines, lo + above[i], key[i], psqt, positional, moves, o);
  } else {
    for (uint32_t c = 1 + lane; c < nrec; c += kGroupLanes) {
      const unsigned long long mine = child_key(psqt, positional, end, o, c);
      uint32_t above = 0;
      for (uint32_t q = 1; q < nrec; ++q) above += child_key(psqt, positional, end, o, q) > mine ? 1u : 0u;
      if (above < k) write_line(lines, lo + above, mine, psqt, positional, moves, o);
    }
  }
  // slots beyond the group's children: all zero (an empty group writes nothing)
  if (nrec)
    for (uint64_t j = (uint64_t)nkids + lane; j < k; j += kGroupLanes) {
      uint32_t* w = lines + (lo + j) * 5;
      w[0] = w[1] = w[2] = w[3] = w[4] = 0u;
    }
}

__global__ __launch_bounds__(kBlock) void gather_parents_kernel(const int32_t* __restrict__ psqt,
                                                                const int32_t* __restrict__ positional,
                                                                const uint32_t* __restrict__ off, uint32_t ngroups,
                                                                uint32_t npos, int32_t* __restrict__ ps_out,
                                                                int32_t* __restrict__ po_out) {
  const uint32_t g = blockIdx.x * kBlock + threadIdx.x;
  if (g >= ngroups) return;
  const uint32_t o = off[g];
  const bool ok = o < npos && o < off[g + 1];
  ps_out[g] = ok ? psqt[o] : 0;
  po_out[g] = ok ? positional[o] : 0;
}

// ---- the second reduction of the two-ply search (fnnue_best_replies_device) ----
// The first reduction's shape: 32 lanes per ply, each folding the children
// lane + 1, lane + 33, ... into one key
//   rank (3 mate in one, 2 a value: a stalemating move is worth 0, 1 the reply
//   mates) << 62 | (value + 2^29) << 32 | ~index,   value = -b_c.value
// from the child's end flags and its own depth-1 record b_c, and summing the
// children's nodes beside it; five xor-shuffles leave the largest key and the
// sum in every lane; lanes 0-7 store one dword each of the 32-byte record.
// Child c of group g is child_best[base + c - 1], base = off[g] - g when every
// group has its own record (the search), else base[g] (hand-made input: the
// count of the children of the groups before, child_counts_kernel and a scan).
static_assert(sizeof(fnnue_best2) == 32, "fnnue_best2 is eight dwords");

// The variants' scores (vbest_replies_kernel below explains them).
constexpr uint32_t kScoreLost = 0, kScoreMated = 1, kScoreValue = 1u << 29, kScoreWins = 1u << 30,
                   kScoreMate = (1u << 30) + 1;

// The key of child c from its end byte f and its own depth-1 record b: the one
// function behind both reductions and the ranking (topk_replies_kernel), so
// that slot 0 of a ply's lines is its fnnue_best2 by construction.
template <bool kVariant>
__device__ __forceinline__ unsigned long long reply_key(uint32_t f, const uint32_t* __restrict__ b, uint32_t c) {
  constexpr uint32_t kDeciding = kFinalCheck | kFinalExtinct | kFinalVariant;
  const uint32_t kind = (b[5] >> 16) & 0xFFu;
  if constexpr (kVariant) {
    uint32_t score;
    if (f & kFinalWon) score = kScoreLost;
    else if (f & (kFinalNoMoves | kFinalDraw)) score = ((f & kFinalNoMoves) && (f & kDeciding)) ? kScoreMate : kScoreValue;
    else if (kind == FNNUE_BEST_LOST) score = kScoreWins;
    else if (kind == FNNUE_BEST_MATE) score = kScoreMated;
    else score = (uint32_t)(kScoreValue - (int32_t)b[2]);
    return (unsigned long long)score << 32 | (0xFFFFFFFFu - c);
  } else {
    uint32_t rank = 2;
    int32_t v = 0;
    if (f & (kFinalNoMoves | kFinalDraw)) {  // a drawn record (kFinalDraw) ranks as a stalemating move; a mate stays a mate
      rank = ((f & kFinalNoMoves) && (f & kDeciding)) ? 3u : 2u;
    } else {
      if (kind == FNNUE_BEST_MATE) rank = 1;
      else v = -(int32_t)b[2];
    }
    return (unsigned long long)rank << 62 | (unsigned long long)(uint32_t)(v + (1 << 29)) << 32 | (0xFFFFFFFFu - c);
  }
}
// What a key says about its child: the FNNUE_BEST_* kind and the value (FNNUE_BEST_CP only, else 0).
template <bool kVariant>
__device__ __forceinline__ uint32_t reply_kind(unsigned long long key) {
  if constexpr (kVariant) {
    const uint32_t score = (uint32_t)(key >> 32);
    return score == kScoreLost ? FNNUE_BEST_LOST : score == kScoreMated ? FNNUE_BEST_MATED
           : score >= kScoreWins ? FNNUE_BEST_MATE : FNNUE_BEST_CP;
  } else {
    const uint32_t rank = (uint32_t)(key >> 62);
    return rank == 3 ? FNNUE_BEST_MATE : rank == 1 ? FNNUE_BEST_MATED : FNNUE_BEST_CP;
  }
}
template <bool kVariant>
__device__ __forceinline__ uint32_t reply_value(unsigned long long key) {
  if constexpr (kVariant) return (uint32_t)(key >> 32) - kScoreValue;
  else return (uint32_t)((int32_t)((uint32_t)(key >> 32) & 0x3FFFFFFFu) - (1 << 29));
}

__global__ __launch_bounds__(kBlock) void child_counts_kernel(const uint32_t* __restrict__ off, uint32_t ngroups,
                                                              uint32_t npos, uint32_t* __restrict__ cnt) {
  const uint32_t g = blockIdx.x * kBlock + threadIdx.x;
  if (g > ngroups) return;
  uint32_t n = 0;
  if (g < ngroups) {
    const uint32_t e = min(off[g + 1], npos), o = min(off[g], e);
    n = e - o ? e - o - 1 : 0;
  }
  cnt[g] = n;
}

__global__ __launch_bounds__(kBlock) void best_replies_kernel(
    const uint8_t* __restrict__ end, const uint16_t* __restrict__ moves, const uint32_t* __restrict__ off,
    uint32_t ngroups, uint32_t npos, const uint32_t* __restrict__ child_best, const uint32_t* __restrict__ base_of,
    uint32_t* __restrict__ out) {
  const uint64_t t = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
  const uint32_t g = (uint32_t)(t / kGroupLanes), lane = (uint32_t)(t % kGroupLanes);
  const bool live = g < ngroups;  // no early return: the shuffles below run with the whole wave
  uint32_t o = 0, e = 0, base = 0;
  if (live) {
    e = min(off[g + 1], npos);
    o = min(off[g], e);
    base = base_of ? base_of[g] : o - g;
  }
  const uint32_t nrec = e - o;
  unsigned long long key = 0;  // 0: no child (a child's key is never 0: ~index)
  uint32_t nodes = 0;
  for (uint32_t c = 1 + lane; c < nrec; c += kGroupLanes) {
    const uint32_t* b = child_best + (size_t)(base + c - 1) * 6;
    nodes += b[3];
    const unsigned long long k = reply_key<false>(end[o + c], b, c);
    key = k > key ? k : key;
  }
#pragma unroll
  for (int m = kGroupLanes / 2; m >= 1; m >>= 1) {
    const unsigned long long other = (unsigned long long)__shfl_xor((long long)key, m, kGroupLanes);
    key = other > key ? other : key;
    nodes += (uint32_t)__shfl_xor((int)nodes, m, kGroupLanes);
  }
  uint32_t w = 0;
  if (nrec) {  // an empty group: all zero
    const uint32_t best = key ? 0xFFFFFFFFu - (uint32_t)key : 0u;
    const uint32_t rank = (uint32_t)(key >> 62);
    const int32_t value = (int32_t)((uint32_t)(key >> 32) & 0x3FFFFFFFu) - (1 << 29);
    const bool one = best && (end[o + best] & (kFinalNoMoves | kFinalDraw));  // the pv ends at the child
    const uint32_t kind = !best ? FNNUE_BEST_NONE : rank == 3 ? FNNUE_BEST_MATE : rank == 1 ? FNNUE_BEST_MATED : FNNUE_BEST_CP;
    const uint32_t pv_len = !best ? 0u : one ? 1u : 2u;
    const uint32_t* b = child_best + (size_t)(base + (best ? best - 1 : 0)) * 6;  // read only with a best child
    switch (lane) {
      case 0: w = !best ? 0u : one ? 0u - b[0] : b[0]; break;  // a one-move pv: the child's own terms, negated (wrapping)
      case 1: w = !best ? 0u : one ? 0u - b[1] : b[1]; break;
      case 2: w = kind == FNNUE_BEST_CP ? (uint32_t)value : 0u; break;
      case 3: w = nrec - 1 + nodes; break;
      case 4: w = best; break;
      case 5: w = best && !one ? b[4] : 0u; break;
      case 6: w = (best && moves ? (uint32_t)moves[o + best] : 0u) | (best && !one ? (b[5] & 0xFFFFu) << 16 : 0u); break;
      case 7: w = kind | (uint32_t)end[o] << 8 | pv_len << 16; break;
      default: break;
    }
  }
  if (live && lane < 8) out[(size_t)g * 8 + lane] = w;
}

// ---- the second reduction with the variant ranks (fnnue_vbest_replies_device) ----
// best_replies_kernel's shape with five ranks: a child its side to move has
// already won (FNNUE_END_WON: the mover lost by playing it) below everything,
// and a child whose every reply loses at once (b_c.kind == FNNUE_BEST_LOST)
// between the values and the mate in one.  Only the middle rank has a value, so
// rank and value share one 32-bit score
//   0 lost, 1 the reply mates, value + 2^29 (|value| <= 2^28: 2^28 .. 3 * 2^28),
//   2^30 every reply loses, 2^30 + 1 mate in one
// and the key is score << 32 | ~index: the whole 32-bit child index stays in
// the key, the tie-break (the lower index) sits in the one 64-bit comparison,
// and a group may have as many children as its 32-bit offsets can describe
// (npos <= 2^32 - 1, which the callers check: at most 2^32 - 2 children).
// (the constants sit above reply_key.)

__global__ __launch_bounds__(kBlock) void vbest_replies_kernel(
    const uint8_t* __restrict__ end, const uint16_t* __restrict__ moves, const uint32_t* __restrict__ off,
    uint32_t ngroups, uint32_t npos, const uint32_t* __restrict__ child_best, const uint32_t* __restrict__ base_of,
    uint32_t* __restrict__ out) {
  const uint64_t t = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
  const uint32_t g = (uint32_t)(t / kGroupLanes), lane = (uint32_t)(t % kGroupLanes);
  const bool live = g < ngroups;  // no early return: the shuffles below run with the whole wave
  uint32_t o = 0, e = 0, base = 0;
  if (live) {
    e = min(off[g + 1], npos);
    o = min(off[g], e);
    base = base_of ? base_of[g] : o - g;
  }
  const uint32_t nrec = e - o;
  unsigned long long key = 0;  // 0: no child (a child's key is never 0: ~index)
  uint32_t nodes = 0;
  for (uint32_t c = 1 + lane; c < nrec; c += kGroupLanes) {
    const uint32_t* b = child_best + (size_t)(base + c - 1) * 6;
    nodes += b[3];
    const unsigned long long k = reply_key<true>(end[o + c], b, c);
    key = k > key ? k : key;
  }
#pragma unroll
  for (int m = kGroupLanes / 2; m >= 1; m >>= 1) {
    const unsigned long long other = (unsigned long long)__shfl_xor((long long)key, m, kGroupLanes);
    key = other > key ? other : key;
    nodes += (uint32_t)__shfl_xor((int)nodes, m, kGroupLanes);
  }
  uint32_t w = 0;
  if (nrec) {  // an empty group: all zero
    const uint32_t best = key ? 0xFFFFFFFFu - (uint32_t)key : 0u;
    const uint32_t score = (uint32_t)(key >> 32);
    const bool one = best && (end[o + best] & (kFinalWon | kFinalNoMoves | kFinalDraw));  // the pv ends at the child
    const uint32_t kind = !best                 ? FNNUE_BEST_NONE
                          : score == kScoreLost ? FNNUE_BEST_LOST
                          : score == kScoreMated ? FNNUE_BEST_MATED
                          : score >= kScoreWins ? FNNUE_BEST_MATE
                                                : FNNUE_BEST_CP;
    const uint32_t pv_len = !best ? 0u : one ? 1u : 2u;
    const uint32_t* b = child_best + (size_t)(base + (best ? best - 1 : 0)) * 6;  // read only with a best child
    switch (lane) {
      case 0: w = !best ? 0u : one ? 0u - b[0] : b[0]; break;  // a one-move pv: the child's own terms, negated (wrapping)
      case 1: w = !best ? 0u : one ? 0u - b[1] : b[1]; break;
      case 2: w = kind == FNNUE_BEST_CP ? score - kScoreValue : 0u; break;
      case 3: w = nrec - 1 + nodes; break;
      case 4: w = best; break;
      case 5: w = best && !one ? b[4] : 0u; break;
      case 6: w = (best && moves ? (uint32_t)moves[o + best] : 0u) | (best && !one ? (b[5] & 0xFFFFu) << 16 : 0u); break;
      case 7: w = kind | (uint32_t)end[o] << 8 | pv_len << 16; break;
      default: break;
    }
  }
  if (live && lane < 8) out[(size_t)g * 8 + lane] = w;
}

// ---- the k best lines per ply of the two-ply search (fnnue_topk_replies_device, MultiPV) ----
// topk_children_kernel's ranking applied to the second reduction's keys
// (reply_key): 32 lanes per ply, up to kTopkFast children staged once in LDS as
// 64-bit keys, every lane counting the keys above each of its own (at most
// kTopkRegs, in registers) by same-address ds_read_b64 broadcasts; a child whose
// count is below the ply's slot count writes its own 28-byte line at that slot.
// A ply with more children (crazyhouse, hand-made input) recomputes the keys
// from global memory.  Slots beyond the children are zeroed; an empty group or
// one without a slot writes nothing; nothing is written at or beyond lines_cap.
static_assert(sizeof(fnnue_line2) == 28, "fnnue_line2 is seven dwords");

template <bool kVariant>
__device__ __forceinline__ void write_line2(uint32_t* __restrict__ lines, uint64_t slot, unsigned long long key,
                                            const uint8_t* __restrict__ end, const uint16_t* __restrict__ moves,
                                            const uint32_t* __restrict__ child_best, uint32_t o, uint32_t base) {
  const uint32_t c = 0xFFFFFFFFu - (uint32_t)key;
  const uint32_t kind = reply_kind<kVariant>(key);
  const uint32_t* b = child_best + (size_t)(base + c - 1) * 6;
  const bool one = end[o + c] & (kVariant ? (kFinalWon | kFinalNoMoves | kFinalDraw) : (kFinalNoMoves | kFinalDraw));  // the pv ends at the child
  uint32_t* w = lines + slot * 7;
  w[0] = one ? 0u - b[0] : b[0];  // a one-move pv: the child's own terms, negated (wrapping)
  w[1] = one ? 0u - b[1] : b[1];
  w[2] = kind == FNNUE_BEST_CP ? reply_value<kVariant>(key) : 0u;
  w[3] = c;
  w[4] = one ? 0u : b[4];
  w[5] = (moves ? (uint32_t)moves[o + c] : 0u) | (one ? 0u : (b[5] & 0xFFFFu) << 16);
  w[6] = kind | (one ? 1u : 2u) << 8;
}

template <bool kVariant>
__global__ __launch_bounds__(kBlock) void topk_replies_kernel(
    const uint8_t* __restrict__ end, const uint16_t* __restrict__ moves, const uint32_t* __restrict__ off,
    uint32_t ngroups, uint32_t npos, const uint32_t* __restrict__ child_best, const uint32_t* __restrict__ base_of,
    const uint32_t* __restrict__ line_off, uint32_t uniform_k, uint32_t* __restrict__ lines, uint64_t lines_cap) {
  __shared__ unsigned long long staged[kTopkGroups][kTopkFast];
  const uint32_t hw = threadIdx.x / kGroupLanes, lane = threadIdx.x % kGroupLanes;
  const uint64_t g64 = (uint64_t)blockIdx.x * kTopkGroups + hw;
  const bool live = g64 < ngroups;  // no early return: the barrier below runs with the whole block
  const uint32_t g = (uint32_t)g64;
  uint32_t o = 0, e = 0, base = 0;
  uint64_t lo = 0, k = 0;  // the group's slots [lo, lo + k), cut at lines_cap
  if (live) {
    e = min(off[g + 1], npos);
    o = min(off[g], e);
    base = base_of ? base_of[g] : o - g;
    if (line_off) {
      lo = line_off[g];
      const uint64_t hi = line_off[g + 1];
      k = hi > lo ? hi - lo : 0;
    } else {
      lo = (uint64_t)g * uniform_k;
      k = uniform_k;
    }
    k = lo < lines_cap ? min(k, lines_cap - lo) : 0;
  }
  const uint32_t nrec = e - o;
  const uint32_t nkids = nrec && k ? nrec - 1 : 0;  // nothing to rank without a slot
  const bool fast = nkids <= kTopkFast;
  unsigned long long key[kTopkRegs];
#pragma unroll
  for (uint32_t i = 0; i < kTopkRegs; ++i) {
    const uint32_t q = lane + kGroupLanes * i;  // child q + 1
    key[i] = 0;
    if (fast && q < nkids) {
      key[i] = reply_key<kVariant>(end[o + q + 1], child_best + (size_t)(base + q) * 6, q + 1);
      staged[hw][q] = key[i];
    }
  }
  __syncthreads();
  if (fast) {
    uint32_t above[kTopkRegs];
#pragma unroll
    for (uint32_t i = 0; i < kTopkRegs; ++i) above[i] = 0;
    for (uint32_t q = 0; q < nkids; ++q) {
      const unsigned long long other = staged[hw][q];  // the same address in every lane of the half wave
#pragma unroll
      for (uint32_t i = 0; i < kTopkRegs; ++i) above[i] += other > key[i] ? 1u : 0u;
    }
#pragma unroll
    for (uint32_t i = 0; i < kTopkRegs; ++i)
      if (key[i] && above[i] < k) write_line2<kVariant>(lines, lo + above[i], key[i], end, moves, child_best, o, base);
  } else {
    for (uint32_t c = 1 + lane; c < nrec; c += kGroupLanes) {
      const unsigned long long mine = reply_key<kVariant>(end[o + c], child_best + (size_t)(base + c - 1) * 6, c);
      uint64_t above = 0;
      for (uint32_t q = 1; q < nrec && above < k; ++q)
        above += reply_key<kVariant>(end[o + q], child_best + (size_t)(base + q - 1) * 6, q) > mine ? 1u : 0u;
      if (above < k) write_line2<kVariant>(lines, lo + above, mine, end, moves, child_best, o, base);
    }
  }
  // slots beyond the group's children: all zero (an empty group writes nothing)
  if (nrec)
    for (uint64_t j = (uint64_t)nkids + lane; j < k; j += kGroupLanes) {
      uint32_t* w = lines + (lo + j) * 7;
      w[0] = w[1] = w[2] = w[3] = w[4] = w[5] = w[6] = 0u;
    }
}

}  // namespace

hipError_t launch_best_children(const int32_t* d_psqt, const int32_t* d_positional, const uint8_t* d_end,
                                const uint16_t* d_moves, const uint32_t* d_off, uint32_t ngroups, uint32_t npos,
                                fnnue_best* d_out, hipStream_t s) {
  if (ngroups == 0) return hipSuccess;
  const uint64_t threads = (uint64_t)ngroups * kGroupLanes;
  hipLaunchKernelGGL(best_children_kernel<false>, dim3((uint32_t)((threads + kBlock - 1) / kBlock)), dim3(kBlock), 0, s,
                     d_psqt, d_positional, d_end, d_moves, d_off, ngroups, npos, reinterpret_cast<uint32_t*>(d_out));
  return hipGetLastError();
}

hipError_t launch_best_children_own(const int32_t* d_psqt, const int32_t* d_positional, const uint8_t* d_end,
                                    const uint16_t* d_moves, const uint32_t* d_off, uint32_t ngroups, uint32_t npos,
                                    fnnue_best* d_out, hipStream_t s) {
  if (ngroups == 0) return hipSuccess;
  const uint64_t threads = (uint64_t)ngroups * kGroupLanes;
  hipLaunchKernelGGL(best_children_kernel<true>, dim3((uint32_t)((threads + kBlock - 1) / kBlock)), dim3(kBlock), 0, s,
                     d_psqt, d_positional, d_end, d_moves, d_off, ngroups, npos, reinterpret_cast<uint32_t*>(d_out));
  return hipGetLastError();
}

hipError_t launch_child_counts(const uint32_t* d_off, uint32_t ngroups, uint32_t npos, uint32_t* d_cnt, hipStream_t s) {
  hipLaunchKernelGGL(child_counts_kernel, dim3((ngroups + 1 + kBlock - 1) / kBlock), dim3(kBlock), 0, s, d_off, ngroups,
                     npos, d_cnt);
  return hipGetLastError();
}

hipError_t launch_best_replies(const uint8_t* d_end, const uint16_t* d_moves, const uint32_t* d_off, uint32_t ngroups,
                               uint32_t npos, const fnnue_best* d_child_best, const uint32_t* d_base,
                               fnnue_best2* d_out, hipStream_t s) {
  if (ngroups == 0) return hipSuccess;
  const uint64_t threads = (uint64_t)ngroups * kGroupLanes;
  hipLaunchKernelGGL(best_replies_kernel, dim3((uint32_t)((threads + kBlock - 1) / kBlock)), dim3(kBlock), 0, s, d_end,
                     d_moves, d_off, ngroups, npos, reinterpret_cast<const uint32_t*>(d_child_best), d_base,
                     reinterpret_cast<uint32_t*>(d_out));
  return hipGetLastError();
}

hipError_t launch_vbest_replies(const uint8_t* d_end, const uint16_t* d_moves, const uint32_t* d_off, uint32_t ngroups,
                                uint32_t npos, const fnnue_best* d_child_best, const uint32_t* d_base,
                                fnnue_best2* d_out, hipStream_t s) {
  if (ngroups == 0) return hipSuccess;
  const uint64_t threads = (uint64_t)ngroups * kGroupLanes;
  hipLaunchKernelGGL(vbest_replies_kernel, dim3((uint32_t)((threads + kBlock - 1) / kBlock)), dim3(kBlock), 0, s, d_end,
                     d_moves, d_off, ngroups, npos, reinterpret_cast<const uint32_t*>(d_child_best), d_base,
                     reinterpret_cast<uint32_t*>(d_out));
  return hipGetLastError();
}

hipError_t launch_topk_children(const int32_t* d_psqt, const int32_t* d_positional, const uint8_t* d_end,
                                const uint16_t* d_moves, const uint32_t* d_off, uint32_t ngroups, uint32_t npos,
                                const uint32_t* d_line_off, uint32_t uniform_k, fnnue_line* d_lines, size_t lines_cap,
                                hipStream_t s) {
  if (ngroups == 0) return hipSuccess;
  hipLaunchKernelGGL(topk_children_kernel, dim3((uint32_t)(((uint64_t)ngroups + kTopkGroups - 1) / kTopkGroups)), dim3(kBlock), 0, s, d_psqt,
                     d_positional, d_end, d_moves, d_off, ngroups, npos, d_line_off, uniform_k,
                     reinterpret_cast<uint32_t*>(d_lines), (uint64_t)lines_cap);
  return hipGetLastError();
}

hipError_t launch_topk_replies(bool vranks, const uint8_t* d_end, const uint16_t* d_moves, const uint32_t* d_off,
                               uint32_t ngroups, uint32_t npos, const fnnue_best* d_child_best, const uint32_t* d_base,
                               const uint32_t* d_line_off, uint32_t uniform_k, fnnue_line2* d_lines, size_t lines_cap,
                               hipStream_t s) {
  if (ngroups == 0) return hipSuccess;
  const dim3 grid((uint32_t)(((uint64_t)ngroups + kTopkGroups - 1) / kTopkGroups));
  const uint32_t* kb = reinterpret_cast<const uint32_t*>(d_child_best);
  uint32_t* out = reinterpret_cast<uint32_t*>(d_lines);
  if (vranks)
    hipLaunchKernelGGL(topk_replies_kernel<true>, grid, dim3(kBlock), 0, s, d_end, d_moves, d_off, ngroups, npos, kb,
                       d_base, d_line_off, uniform_k, out, (uint64_t)lines_cap);
  else
    hipLaunchKernelGGL(topk_replies_kernel<false>, grid, dim3(kBlock), 0, s, d_end, d_moves, d_off, ngroups, npos, kb,
                       d_base, d_line_off, uniform_k, out, (uint64_t)lines_cap);
  return hipGetLastError();
}

hipError_t launch_gather_parents(const int32_t* d_psqt, const int32_t* d_positional, const uint32_t* d_off,
                                 uint32_t ngroups, uint32_t npos, int32_t* d_ps_out, int32_t* d_po_out,
                                 hipStream_t s) {
  if (ngroups == 0) return hipSuccess;
  hipLaunchKernelGGL(gather_parents_kernel, dim3((ngroups + kBlock - 1) / kBlock), dim3(kBlock), 0, s, d_psqt,
                     d_positional, d_off, ngroups, npos, d_ps_out, d_po_out);
  return hipGetLastError();
}

}  // namespace fnnue
