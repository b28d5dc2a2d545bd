// quiesce.hip — capture quiescence below the device search's leaves (ABI 3.13;
// the rule: include/fnnue.h, the design: DESIGN.md §4.21).
//
// A level-synchronous capture tree.  The frontier is a dense array of boards;
// per level
//   capture_count_kernel  one thread per node: its legal captures (a node
//                         without one forms no group and costs no evaluation)
//   two exclusive scans   the nodes' first records and their group numbers
//   capture_write_kernel  one thread per record of the STAR groups [node, its
//                         captures]: the node's captures regenerated up to the
//                         record's own (write_children_record_kernel's form),
//                         the packed record, its move code, the child's board
//                         as the next frontier, the group's offset
//   the STAR evaluation   fnnue_eval_groups_device over the level
//   quiet_leaves_kernel   one thread per node: its children's static results
// and, from the deepest level up,
//   quiet_reduce_kernel   one thread per node (a group is a handful of records):
//                         stand pat against the negated results of its captures,
//                         the first maximum wins.
// No end flags, no checks, no mates inside the tree: the plain rule.  With
// "quiescence checks" (ABI 3.14) the generators and the results'
// kernels run in their checks form (the template argument CHK): a node in check
// lists all its legal moves and may not stand pat, a node in check without one
// is mated, mate values lose one ply per level on the way up, and the children
// of the last level, whose boards the plain form does not keep, are written and
// probed for mates by mate_probe_kernel.  Each level's size is read
// back once; a level above FNNUE_QUIESCE_RECORDS makes the host cut down the slice
// of the root frontier it works on and redo it (one root's own tree is never cut).
// The variants (ABI 3.15) run the same levels with generators
// of their own (vcapture_count / vcapture_write / vprobe over a rule set): the
// variant's legality, fnnue_vpos records, and positions the variant's rule has
// ended decided on the way down and at the horizon.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdlib>
#include <utility>
#include <vector>

#include "board.h"
#include "builder.h"
#include "chess_rules.h"
#include "internal.h"
#include "search_steps.h"
#include "vboard.h"

namespace fnnue {

namespace {

constexpr uint32_t kGenBlock = 64, kBlock = 256;
static_assert(sizeof(fnnue_quiet) == 20, "fnnue_quiet is five dwords");

// The legal captures of b in for_each_legal's order (the order of the ply's
// children, restricted to captures): own pieces by square; a pawn's captures by
// square (promotions Q, R, B, N), then en passant.  Castling and pushes take
// nothing.  f(move) returns false to stop early.
template <class F>
__device__ void for_each_capture(const DBoard& b, F&& f) {
  const int us = b.stm, them = us ^ 1;
  const uint64_t occ = b.bc[0] | b.bc[1], own = colour(b, us), opp = colour(b, them);
  const int rank7 = us == WHITE ? 6 : 1, down = us == WHITE ? -8 : 8;
  auto emit = [&](int from, int to, int promo) -> bool {
    const DMove m{from, to, promo, 0};
    return !legal(b, m) || f(m);
  };
  for (uint64_t pcs = own; pcs; pcs &= pcs - 1) {
    const int s = lsb(pcs);
    const uint64_t sm = 1ull << s;
    if (b.bt[PAWN] & sm) {
      const bool promo = (s >> 3) == rank7;
      for (uint64_t a = pawn_att(us, s) & opp; a; a &= a - 1) {
        const int t = lsb(a);
        if (promo) {
          for (int p = QUEEN; p >= KNIGHT; --p)
            if (!emit(s, t, p)) return;
        } else if (!emit(s, t, 0)) {
          return;
        }
      }
      // en passant takes the pawn behind the square (an en-passant square without one takes nothing)
      if (b.ep >= 0 && b.ep < 64 && (pawn_att(us, s) & (1ull << b.ep)) && b.ep + down >= 0 && b.ep + down < 64 &&
          (opp & b.bt[PAWN] & (1ull << (b.ep + down))) && !emit(s, b.ep, 0))
        return;
      continue;
    }
    uint64_t targets;
    if (b.bt[KNIGHT] & sm) targets = knight_att(s);
    else if (b.bt[BISHOP] & sm) targets = bishop_att(s, occ);
    else if (b.bt[ROOK] & sm) targets = rook_att(s, occ);
    else if (b.bt[QUEEN] & sm) targets = bishop_att(s, occ) | rook_att(s, occ);
    else targets = king_att(s);
    for (uint64_t t = targets & opp; t; t &= t - 1)
      if (!emit(s, lsb(t), 0)) return;
  }
}

__device__ __forceinline__ int32_t static_value(int32_t ps, int32_t po) {
  return (int32_t)(((long long)ps + (long long)po) / 16);
}

__device__ __forceinline__ fnnue_quiet stand_pat(int32_t ps, int32_t po) {
  fnnue_quiet q;
  q.psqt = ps;
  q.positional = po;
  q.value = static_value(ps, po);
  q.nodes = 0;
  q.move = 0;
  q.len = 0;
  q.reserved = 0;
  return q;
}

// A decided (mate) result in the checks form: psqt 0, positional 16 * value.
__device__ __forceinline__ fnnue_quiet decided(int32_t v, uint32_t nodes, uint16_t move, uint8_t len) {
  fnnue_quiet q;
  q.psqt = 0;
  q.positional = 16 * v;
  q.value = v;
  q.nodes = nodes;
  q.move = move;
  q.len = len;
  q.reserved = FNNUE_QUIET_DECIDED;
  return q;
}

// Has b's side to move a legal move?
__device__ __forceinline__ bool any_legal(const DBoard& b) {
  bool any = false;
  for_each_legal(b, [&](const DMove&) -> bool {
    any = true;
    return false;
  });
  return any;
}

// The node flags of the checks form.
constexpr uint8_t kNodeInCheck = 1, kNodeMated = 2;

// cnt[i]: the records of node i's group (1 + its captures, 0 without a capture),
// has[i]: whether it forms one.  active (optional): nodes with 0 stay as they are.
template <bool CHK>
__global__ __launch_bounds__(kGenBlock) void capture_count_kernel(const DBoard* __restrict__ states,
                                                                  const uint8_t* __restrict__ active, uint32_t n,
                                                                  uint32_t* __restrict__ cnt,
                                                                  uint32_t* __restrict__ has,
                                                                  uint8_t* __restrict__ flag,
                                                                  fnnue_quiet* __restrict__ above,
                                                                  unsigned long long* __restrict__ evasions) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  uint32_t c = 0;
  uint8_t fl = 0;
  if (!active || active[i]) {
    const DBoard b = states[i];
    auto count = [&](const DMove&) -> bool {
      ++c;
      return true;
    };
    if constexpr (CHK) {
      // checks form: a node in check counts all its legal moves; without one it
      // is mated, and its result in the level above (written before this kernel
      // on the same stream) becomes the mate value
      if (in_check(b)) {
        fl = kNodeInCheck;
        for_each_legal(b, count);
        if (!c) {
          fl |= kNodeMated;
          above[i] = decided(-FNNUE_VALUE_MATE, 0, 0, 0);
        } else if (evasions) {
          atomicAdd(evasions, (unsigned long long)c);
          atomicAdd(evasions + 1, 1ull);
        }
      } else {
        for_each_capture(b, count);
      }
    } else {
      for_each_capture(b, count);
    }
  }
  if constexpr (CHK) flag[i] = fl;
  cnt[i] = c ? c + 1 : 0;
  has[i] = c ? 1 : 0;
}

// The checks form's horizon: the boards that are not expanded (the children of
// the last level, the roots at depth 0).  A side in check without a legal move
// is mated at every depth; one that has a move stands pat here.
__global__ __launch_bounds__(kGenBlock) void mate_probe_kernel(const DBoard* __restrict__ states, uint32_t n,
                                                               fnnue_quiet* __restrict__ res) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const DBoard b = states[i];
  if (in_check(b) && !any_legal(b)) res[i] = decided(-FNNUE_VALUE_MATE, 0, 0, 0);
}

// One thread per record: record r belongs to the last node i with roff[i] <= r
// (nodes without a group repeat their successor's offset); r - roff[i] = 0 is
// the node itself, k > 0 its k-th capture.  Child k of node i is entry
// roff[i] - gidx[i] + k - 1 of the next frontier.
// Checks form: a node in check (flag) regenerates its legal moves instead.
template <bool CHK>
__global__ __launch_bounds__(kGenBlock) void capture_write_kernel(
    const DBoard* __restrict__ states, uint32_t n, const uint32_t* __restrict__ roff,
    const uint32_t* __restrict__ gidx, uint32_t total, uint32_t ngroups, fnnue_pos* __restrict__ out,
    uint16_t* __restrict__ moves, uint32_t* __restrict__ goff, DBoard* __restrict__ next,
    const uint8_t* __restrict__ flag) {
  const uint32_t r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= total) return;
  uint32_t lo = 0, hi = n;  // roff[lo] <= r < roff[hi]
  while (hi - lo > 1) {
    const uint32_t mid = (lo + hi) >> 1;
    if (roff[mid] <= r) lo = mid;
    else hi = mid;
  }
  const uint32_t k = r - roff[lo], g = gidx[lo];
  const DBoard b = states[lo];
  DBoard c = b;
  uint16_t mv = 0;
  if (k) {
    uint32_t j = 0;
    auto take = [&](const DMove& m) -> bool {
      if (++j < k) return true;
      do_move(c, m);
      mv = (uint16_t)((uint32_t)m.from | (uint32_t)m.to << 6 | (uint32_t)m.promo << 12);
      return false;
    };
    if constexpr (CHK) {
      if (flag[lo] & kNodeInCheck) for_each_legal(b, take);  // no castling out of check: the code needs no flag
      else for_each_capture(b, take);
    } else {
      for_each_capture(b, take);
    }
    if (next) next[r - g - 1] = c;
  } else {
    goff[g] = r;
  }
  if (r == total - 1) goff[ngroups] = total;
  out[r] = pack(c);
  moves[r] = mv;
}

// The children of every group as results of their own: standing pat on the
// level's evaluation (the deepest level stays so; the others are reduced over).
__global__ __launch_bounds__(kBlock) void quiet_leaves_kernel(const uint32_t* __restrict__ roff,
                                                              const uint32_t* __restrict__ gidx, uint32_t n,
                                                              const int32_t* __restrict__ ps,
                                                              const int32_t* __restrict__ po,
                                                              fnnue_quiet* __restrict__ res) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const uint32_t o = roff[i], e = roff[i + 1];
  if (e <= o) return;
  const uint32_t base = o - gidx[i] - 1;
  for (uint32_t k = 1; k < e - o; ++k) res[base + k] = stand_pat(ps[o + k], po[o + k]);
}

// Node i's result by the rule: candidate 0 is standing pat (what node[i] holds),
// the captures follow in order, a later one replaces the current only when it
// is strictly greater.  Terms negated with int32 wrap-around, as fnnue_best's.
// Checks form: a node in check has no candidate 0 (its first evasion is), and a
// decided child result moves one ply toward zero when it is negated.  ZERO (the
// variants): a decided draw stays 0 and stays decided.
template <bool CHK, bool ZERO = false>
__global__ __launch_bounds__(kBlock) void quiet_reduce_kernel(const uint32_t* __restrict__ roff,
                                                              const uint32_t* __restrict__ gidx, uint32_t n,
                                                              const uint16_t* __restrict__ moves,
                                                              const fnnue_quiet* __restrict__ child,
                                                              fnnue_quiet* __restrict__ node,
                                                              const uint8_t* __restrict__ flag) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const uint32_t o = roff[i], e = roff[i + 1];
  if (e <= o) return;
  const uint32_t base = o - gidx[i] - 1;
  fnnue_quiet best = node[i];
  uint32_t nodes = 0;
  bool have = true;
  if constexpr (CHK) have = !(flag[i] & kNodeInCheck);
  for (uint32_t k = 1; k < e - o; ++k) {
    const fnnue_quiet ch = child[base + k];
    nodes += 1u + ch.nodes;
    if constexpr (CHK) {
      if (ch.reserved & FNNUE_QUIET_DECIDED) {
        int32_t v = ch.value > 0 ? -(ch.value - 1) : -(ch.value + 1);
        if constexpr (ZERO) v = ch.value ? v : 0;
        if (!have || v > best.value) best = decided(v, 0, moves[o + k], (uint8_t)(ch.len + 1));
        have = true;
        continue;
      }
    }
    const int32_t v = -ch.value;
    if (!have || v > best.value) {
      best.psqt = (int32_t)(0u - (uint32_t)ch.psqt);
      best.positional = (int32_t)(0u - (uint32_t)ch.positional);
      best.value = v;
      best.move = moves[o + k];
      best.len = (uint8_t)(ch.len + 1);
      if constexpr (CHK) best.reserved = 0;
    }
    have = true;
  }
  best.nodes = nodes;
  node[i] = best;
}

// The roots of the search's form: leaf d is record off[map[d].x] + map[d].y of
// the parents' STAR groups (child_states_device's map).
__global__ __launch_bounds__(kBlock) void leaf_init_kernel(const uint2* __restrict__ map,
                                                           const uint32_t* __restrict__ off,
                                                           const uint8_t* __restrict__ end,
                                                           const int32_t* __restrict__ ps,
                                                           const int32_t* __restrict__ po, uint32_t nleaf,
                                                           fnnue_quiet* __restrict__ res,
                                                           uint8_t* __restrict__ active) {
  const uint32_t d = blockIdx.x * blockDim.x + threadIdx.x;
  if (d >= nleaf) return;
  const uint2 m = map[d];
  const uint32_t r = off[m.x] + m.y;
  res[d] = stand_pat(ps[r], po[r]);
  active[d] = (end[r] & (kFinalNoMoves | kFinalDraw)) ? 0 : 1;
}

// Checks form: a decided leaf at search depth p counts its plies from the
// searched ply, p further from the mate value.  ZERO (the variants): a decided
// draw is written as (0, 0).
template <bool CHK, bool ZERO = false>
__global__ __launch_bounds__(kBlock) void leaf_scatter_kernel(const uint2* __restrict__ map,
                                                              const uint32_t* __restrict__ off,
                                                              const uint8_t* __restrict__ active,
                                                              const fnnue_quiet* __restrict__ res, uint32_t nleaf,
                                                              int32_t* __restrict__ ps, int32_t* __restrict__ po,
                                                              int32_t p) {
  const uint32_t d = blockIdx.x * blockDim.x + threadIdx.x;
  if (d >= nleaf || !active[d]) return;
  const uint2 m = map[d];
  const uint32_t r = off[m.x] + m.y;
  if constexpr (CHK) {
    if (res[d].reserved & FNNUE_QUIET_DECIDED) {
      const int32_t v = res[d].value;
      ps[r] = 0;
      if constexpr (ZERO) po[r] = v ? 16 * (v > 0 ? v - p : v + p) : 0;
      else po[r] = 16 * (v > 0 ? v - p : v + p);
      return;
    }
  }
  ps[r] = res[d].psqt;
  po[r] = res[d].positional;
}

// The roots of fnnue_quiesce_device: the plies themselves.
__global__ __launch_bounds__(kBlock) void node_init_kernel(const int32_t* __restrict__ ps,
                                                           const int32_t* __restrict__ po, uint32_t n,
                                                           fnnue_quiet* __restrict__ res) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) res[i] = stand_pat(ps[i], po[i]);
}

__global__ __launch_bounds__(kGenBlock) void pack_boards_kernel(const DBoard* __restrict__ states, uint32_t n,
                                                                fnnue_pos* __restrict__ out) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) out[i] = pack(states[i]);
}

// ---- the variants (ABI 3.15) ----
// The generators over a variant's boards, records and rules; everything behind
// them (scans, quiet_leaves, quiet_reduce, the roots' kernels) is the chess
// tree's in its decided-aware form, whatever the checks setting: a position the
// variant's rule has ended is decided with checks off too.
// R: the rule set.  VBoardRules: crazyhouse and atomic on vboard.h's boards
// (the board says which); PlainQRules<V>: kingofthehill, racingkings and
// threecheck on DBoard boards (threecheck's counters in bt[0], spent by
// do_move_v as in vchild_states_device).
struct VBoardRules {
  using Board = vb::VBoard;
  using Move = vb::VMove;
  __device__ static int over(const Board& b) { return vb::over_state(b); }
  __device__ static bool check(const Board& b) { return vb::quiet_check(b); }
  template <class F>
  __device__ static void legal_moves(const Board& b, F&& f) { vb::for_each_legal(b, f); }
  template <class F>
  __device__ static void captures(const Board& b, F&& f) { vb::for_each_capture(b, f); }
  __device__ static void play(Board& c, const Move& m) { vb::do_move(c, m); }
  __device__ static uint16_t code(const Board& b, const Move& m) { return vb::move_code(b, m); }
  __device__ static fnnue_vpos pack(const Board& b) { return vb::pack(b); }
};
template <int V>
struct PlainQRules {
  using Board = DBoard;
  using Move = DMove;
  __device__ static int over(const Board& b) { return plain_over_state<V>(b); }
  __device__ static bool check(const Board& b) { return plain_quiet_check<V>(b); }
  template <class F>
  __device__ static void legal_moves(const Board& b, F&& f) { for_each_legal<V>(b, f); }
  template <class F>
  __device__ static void captures(const Board& b, F&& f) { for_each_capture<V>(b, f); }
  __device__ static void play(Board& c, const Move& m) { do_move_v<V>(c, m); }
  // no castling out of check, and no capture castles: the code needs no flag
  __device__ static uint16_t code(const Board&, const Move& m) {
    return (uint16_t)((uint32_t)m.from | (uint32_t)m.to << 6 | (uint32_t)m.promo << 12);
  }
  __device__ static fnnue_vpos pack(const Board& b) {  // the chess record, empty pockets
    const fnnue_pos p = fnnue::pack(b);
    uint32_t q[12];
    memcpy(q, &p, sizeof(p));
    q[9] = q[10] = q[11] = 0;
    fnnue_vpos v;
    memcpy(&v, q, sizeof(v));
    return v;
  }
};

__device__ __forceinline__ int32_t over_value(int over) {
  return over == FNNUE_VQ_LOST ? -FNNUE_VALUE_MATE : over == FNNUE_VQ_WON ? FNNUE_VALUE_MATE : 0;
}

// capture_count_kernel over R: a node the variant's rule has ended, like a
// mated one, counts nothing and has its result in the level above overwritten.
template <class R, bool CHK>
__global__ __launch_bounds__(kGenBlock) void vcapture_count_kernel(const typename R::Board* __restrict__ states,
                                                                   const uint8_t* __restrict__ active, uint32_t n,
                                                                   uint32_t* __restrict__ cnt,
                                                                   uint32_t* __restrict__ has,
                                                                   uint8_t* __restrict__ flag,
                                                                   fnnue_quiet* __restrict__ above,
                                                                   unsigned long long* __restrict__ evasions) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  uint32_t c = 0;
  uint8_t fl = 0;
  if (!active || active[i]) {
    const typename R::Board b = states[i];
    auto count = [&](const typename R::Move&) -> bool {
      ++c;
      return true;
    };
    const int over = R::over(b);
    bool chk = false;
    if constexpr (CHK) chk = !over && R::check(b);
    if (over) {
      fl = kNodeMated;
      above[i] = decided(over_value(over), 0, 0, 0);
    } else if (chk) {
      fl = kNodeInCheck;
      R::legal_moves(b, count);
      if (!c) {
        fl |= kNodeMated;
        above[i] = decided(-FNNUE_VALUE_MATE, 0, 0, 0);
      } else if (evasions) {
        atomicAdd(evasions, (unsigned long long)c);
        atomicAdd(evasions + 1, 1ull);
      }
    } else {
      R::captures(b, count);
    }
  }
  flag[i] = fl;
  cnt[i] = c ? c + 1 : 0;
  has[i] = c ? 1 : 0;
}

// The horizon (the children of the last level, the roots at depth 0): over and,
// in the checks form, mated positions are decided at every depth.
template <class R, bool CHK>
__global__ __launch_bounds__(kGenBlock) void vprobe_kernel(const typename R::Board* __restrict__ states, uint32_t n,
                                                           fnnue_quiet* __restrict__ res) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const typename R::Board b = states[i];
  const int over = R::over(b);
  if (over) {
    res[i] = decided(over_value(over), 0, 0, 0);
    return;
  }
  if constexpr (CHK) {
    if (!R::check(b)) return;
    bool any = false;
    R::legal_moves(b, [&](const typename R::Move&) -> bool {
      any = true;
      return false;
    });
    if (!any) res[i] = decided(-FNNUE_VALUE_MATE, 0, 0, 0);
  }
}

// capture_write_kernel over R: fnnue_vpos records, variant move codes (a node
// in check may be answered by a drop), the children's boards always kept (the
// horizon is probed whatever the checks setting).
template <class R>
__global__ __launch_bounds__(kGenBlock) void vcapture_write_kernel(
    const typename R::Board* __restrict__ states, uint32_t n, const uint32_t* __restrict__ roff,
    const uint32_t* __restrict__ gidx, uint32_t total, uint32_t ngroups, fnnue_vpos* __restrict__ out,
    uint16_t* __restrict__ moves, uint32_t* __restrict__ goff, typename R::Board* __restrict__ next,
    const uint8_t* __restrict__ flag) {
  const uint32_t r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= total) return;
  uint32_t lo = 0, hi = n;  // roff[lo] <= r < roff[hi]
  while (hi - lo > 1) {
    const uint32_t mid = (lo + hi) >> 1;
    if (roff[mid] <= r) lo = mid;
    else hi = mid;
  }
  const uint32_t k = r - roff[lo], g = gidx[lo];
  const typename R::Board b = states[lo];
  typename R::Board c = b;
  uint16_t mv = 0;
  if (k) {
    uint32_t j = 0;
    auto take = [&](const typename R::Move& m) -> bool {
      if (++j < k) return true;
      R::play(c, m);
      mv = R::code(b, m);
      return false;
    };
    if (flag[lo] & kNodeInCheck) R::legal_moves(b, take);
    else R::captures(b, take);
    next[r - g - 1] = c;
  } else {
    goff[g] = r;
  }
  if (r == total - 1) goff[ngroups] = total;
  out[r] = R::pack(c);
  moves[r] = mv;
}

template <class R>
__global__ __launch_bounds__(kGenBlock) void vpack_boards_kernel(const typename R::Board* __restrict__ states,
                                                                 uint32_t n, fnnue_vpos* __restrict__ out) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) out[i] = R::pack(states[i]);
}

inline dim3 grid_for(size_t n, uint32_t bs) { return dim3((uint32_t)((n + bs - 1) / bs)); }

using W = BuilderScratch;
using detail::fail;
using detail::hip_fail;

// The trace's phases: an event where each starts, the differences summed at the end (QuiesceStats::timed only).
struct Marks {
  enum { kRoots, kGen, kEval, kReduce, kEnd };
  bool on = false;
  hipStream_t s = nullptr;
  std::vector<std::pair<int, hipEvent_t>> marks;
  void mark(int phase) {
    if (!on) return;
    hipEvent_t ev = nullptr;
    if (hipEventCreate(&ev) != hipSuccess || hipEventRecord(ev, s) != hipSuccess) on = false;
    if (ev) marks.emplace_back(phase, ev);
  }
  void report(QuiesceStats* st) {
    if (on && st && !marks.empty() && hipEventSynchronize(marks.back().second) == hipSuccess) {
      double* const ms[kEnd] = {&st->roots_ms, &st->gen_ms, &st->eval_ms, &st->reduce_ms};
      for (size_t i = 0; i + 1 < marks.size(); ++i) {
        float t = 0;
        if (marks[i].first < kEnd && hipEventElapsedTime(&t, marks[i].second, marks[i + 1].second) == hipSuccess)
          *ms[marks[i].first] += t;
      }
    }
  }
  ~Marks() {
    for (auto& m : marks) (void)hipEventDestroy(m.second);
  }
};

// One rule set's kernels in one checks form, as launches over untyped boards
// and records: what the host's levels need to know about the rules.
struct Gen {
  size_t board_bytes = 0, record_bytes = 0;
  bool variant = false;  // fnnue_vpos records through the variant evaluator
  bool checks = false;   // nodes in check list their evasions (the trace counts them)
  // per node a flag byte, the last level's boards kept and probed, decided results on the way down:
  // the checks form of chess, every form of a variant
  bool decided = false;
  void (*count)(const void* states, const uint8_t* active, uint32_t n, uint32_t* cnt, uint32_t* has, uint8_t* flag,
                fnnue_quiet* above, unsigned long long* evasions, hipStream_t s) = nullptr;
  void (*write)(const void* states, uint32_t n, const uint32_t* roff, const uint32_t* gidx, uint32_t total,
                uint32_t ngroups, void* out, uint16_t* moves, uint32_t* goff, void* next, const uint8_t* flag,
                hipStream_t s) = nullptr;
  void (*probe)(const void* states, uint32_t n, fnnue_quiet* res, hipStream_t s) = nullptr;
  void (*pack)(const void* states, uint32_t n, void* out, hipStream_t s) = nullptr;
  void (*reduce)(const uint32_t* roff, const uint32_t* gidx, uint32_t n, const uint16_t* moves,
                 const fnnue_quiet* child, fnnue_quiet* node, const uint8_t* flag, hipStream_t s) = nullptr;
  void (*scatter)(const uint2* map, const uint32_t* off, const uint8_t* active, const fnnue_quiet* res, uint32_t nleaf,
                  int32_t* ps, int32_t* po, int32_t p, hipStream_t s) = nullptr;
};

template <bool CHK>
Gen chess_gen() {
  Gen g;
  g.board_bytes = sizeof(DBoard);
  g.record_bytes = sizeof(fnnue_pos);
  g.checks = g.decided = CHK;
  g.count = [](const void* states, const uint8_t* active, uint32_t n, uint32_t* cnt, uint32_t* has, uint8_t* flag,
               fnnue_quiet* above, unsigned long long* evasions, hipStream_t s) {
    hipLaunchKernelGGL(capture_count_kernel<CHK>, grid_for(n, kGenBlock), dim3(kGenBlock), 0, s,
                       static_cast<const DBoard*>(states), active, n, cnt, has, flag, above, evasions);
  };
  g.write = [](const void* states, uint32_t n, const uint32_t* roff, const uint32_t* gidx, uint32_t total,
               uint32_t ngroups, void* out, uint16_t* moves, uint32_t* goff, void* next, const uint8_t* flag,
               hipStream_t s) {
    hipLaunchKernelGGL(capture_write_kernel<CHK>, grid_for(total, kGenBlock), dim3(kGenBlock), 0, s,
                       static_cast<const DBoard*>(states), n, roff, gidx, total, ngroups, static_cast<fnnue_pos*>(out),
                       moves, goff, static_cast<DBoard*>(next), flag);
  };
  g.probe = [](const void* states, uint32_t n, fnnue_quiet* res, hipStream_t s) {
    hipLaunchKernelGGL(mate_probe_kernel, grid_for(n, kGenBlock), dim3(kGenBlock), 0, s,
                       static_cast<const DBoard*>(states), n, res);
  };
  g.pack = [](const void* states, uint32_t n, void* out, hipStream_t s) {
    hipLaunchKernelGGL(pack_boards_kernel, grid_for(n, kGenBlock), dim3(kGenBlock), 0, s,
                       static_cast<const DBoard*>(states), n, static_cast<fnnue_pos*>(out));
  };
  g.reduce = [](const uint32_t* roff, const uint32_t* gidx, uint32_t n, const uint16_t* moves, const fnnue_quiet* child,
                fnnue_quiet* node, const uint8_t* flag, hipStream_t s) {
    hipLaunchKernelGGL(quiet_reduce_kernel<CHK>, grid_for(n, kBlock), dim3(kBlock), 0, s, roff, gidx, n, moves, child,
                       node, flag);
  };
  g.scatter = [](const uint2* map, const uint32_t* off, const uint8_t* active, const fnnue_quiet* res, uint32_t nleaf,
                 int32_t* ps, int32_t* po, int32_t p, hipStream_t s) {
    hipLaunchKernelGGL(leaf_scatter_kernel<CHK>, grid_for(nleaf, kBlock), dim3(kBlock), 0, s, map, off, active, res,
                       nleaf, ps, po, CHK ? p : 0);
  };
  return g;
}

template <class R, bool CHK>
Gen variant_gen() {
  using Board = typename R::Board;
  Gen g;
  g.board_bytes = sizeof(Board);
  g.record_bytes = sizeof(fnnue_vpos);
  g.variant = g.decided = true;
  g.checks = CHK;
  g.count = [](const void* states, const uint8_t* active, uint32_t n, uint32_t* cnt, uint32_t* has, uint8_t* flag,
               fnnue_quiet* above, unsigned long long* evasions, hipStream_t s) {
    hipLaunchKernelGGL((vcapture_count_kernel<R, CHK>), grid_for(n, kGenBlock), dim3(kGenBlock), 0, s,
                       static_cast<const Board*>(states), active, n, cnt, has, flag, above, evasions);
  };
  g.write = [](const void* states, uint32_t n, const uint32_t* roff, const uint32_t* gidx, uint32_t total,
               uint32_t ngroups, void* out, uint16_t* moves, uint32_t* goff, void* next, const uint8_t* flag,
               hipStream_t s) {
    hipLaunchKernelGGL(vcapture_write_kernel<R>, grid_for(total, kGenBlock), dim3(kGenBlock), 0, s,
                       static_cast<const Board*>(states), n, roff, gidx, total, ngroups, static_cast<fnnue_vpos*>(out),
                       moves, goff, static_cast<Board*>(next), flag);
  };
  g.probe = [](const void* states, uint32_t n, fnnue_quiet* res, hipStream_t s) {
    hipLaunchKernelGGL((vprobe_kernel<R, CHK>), grid_for(n, kGenBlock), dim3(kGenBlock), 0, s,
                       static_cast<const Board*>(states), n, res);
  };
  g.pack = [](const void* states, uint32_t n, void* out, hipStream_t s) {
    hipLaunchKernelGGL(vpack_boards_kernel<R>, grid_for(n, kGenBlock), dim3(kGenBlock), 0, s,
                       static_cast<const Board*>(states), n, static_cast<fnnue_vpos*>(out));
  };
  g.reduce = [](const uint32_t* roff, const uint32_t* gidx, uint32_t n, const uint16_t* moves, const fnnue_quiet* child,
                fnnue_quiet* node, const uint8_t* flag, hipStream_t s) {
    hipLaunchKernelGGL((quiet_reduce_kernel<true, true>), grid_for(n, kBlock), dim3(kBlock), 0, s, roff, gidx, n, moves,
                       child, node, flag);
  };
  g.scatter = [](const uint2* map, const uint32_t* off, const uint8_t* active, const fnnue_quiet* res, uint32_t nleaf,
                 int32_t* ps, int32_t* po, int32_t p, hipStream_t s) {
    hipLaunchKernelGGL((leaf_scatter_kernel<true, true>), grid_for(nleaf, kBlock), dim3(kBlock), 0, s, map, off, active,
                       res, nleaf, ps, po, p);
  };
  return g;
}

template <class R>
Gen variant_gen(bool checks) {
  return checks ? variant_gen<R, true>() : variant_gen<R, false>();
}

// The rules' kernels; false: a variant without a capture tree (none the searches serve).
bool gen_for(SearchRules r, bool checks, Gen* g) {
  switch (r.variant) {
    case kVariantChess: *g = checks ? chess_gen<true>() : chess_gen<false>(); return true;
    case kVariantCrazyhouse:
    case kVariantAtomic: *g = variant_gen<VBoardRules>(checks); return true;
    case kVariantKingOfTheHill: *g = variant_gen<PlainQRules<kVariantKingOfTheHill>>(checks); return true;
    case kVariantRacingKings: *g = variant_gen<PlainQRules<kVariantRacingKings>>(checks); return true;
    case kVariantThreeCheck: *g = variant_gen<PlainQRules<kVariantThreeCheck>>(checks); return true;
    default: return false;
  }
}

inline const void* board_at(const Gen& g, const void* boards, size_t i) {
  return static_cast<const char*>(boards) + i * g.board_bytes;
}

// One slice [a, b) of the root frontier through every level and back.
// *overflow: a level passed the budget (nothing of the slice is reduced then).
// In the decided form the mated and finished roots and nodes are written on the way down.
int quiesce_slice(fnnue_ctx* ctx, W& ws, const Gen& gen, const void* roots, const uint8_t* active, size_t a, size_t b,
                  fnnue_quiet* res0, int depth, size_t budget, hipStream_t s, QuiesceStats* st, Marks& tm,
                  size_t* overflow) {
  *overflow = 0;
  const void* cur = board_at(gen, roots, a);
  const uint8_t* cur_active = active ? active + a : nullptr;
  uint32_t cur_n = (uint32_t)(b - a);
  uint32_t level_n[FNNUE_QUIESCE_MAX + 1] = {};
  uint32_t *roff[FNNUE_QUIESCE_MAX + 1] = {}, *gidx[FNNUE_QUIESCE_MAX + 1] = {};
  uint16_t* moves[FNNUE_QUIESCE_MAX + 1] = {};
  fnnue_quiet* res[FNNUE_QUIESCE_MAX + 1] = {};
  uint64_t recs[FNNUE_QUIESCE_MAX + 1] = {};
  uint8_t* flag[FNNUE_QUIESCE_MAX + 1] = {};
  // the trace's evasion counters, per level [evasion records, nodes in check with one]
  unsigned long long* evas = nullptr;
  if (gen.checks && st && st->timed) {
    HIP_TRY(ws.get(W::kQEvasions, FNNUE_QUIESCE_MAX * 16, (void**)&evas), "device allocation (quiescence scratch)");
    HIP_TRY(hipMemsetAsync(evas, 0, FNNUE_QUIESCE_MAX * 16, s), "hipMemsetAsync");
  }
  res[0] = res0 + a;
  int deepest = 0;
  for (int L = 1; L <= depth && cur_n; ++L) {
    const int x = L - 1;  // the level's scratch slots
    uint32_t *cnt = nullptr, *has = nullptr;
    tm.mark(Marks::kGen);
    HIP_TRY(ws.get(W::kQCnt, ((size_t)cur_n + 1) * 4, (void**)&cnt), "device allocation (quiescence scratch)");
    HIP_TRY(ws.get(W::kQHas, ((size_t)cur_n + 1) * 4, (void**)&has), "device allocation (quiescence scratch)");
    HIP_TRY(ws.get(W::kQRoff + x, ((size_t)cur_n + 1) * 4, (void**)&roff[L]), "device allocation (quiescence scratch)");
    HIP_TRY(ws.get(W::kQGidx + x, ((size_t)cur_n + 1) * 4, (void**)&gidx[L]), "device allocation (quiescence scratch)");
    HIP_TRY(hipMemsetAsync(cnt + cur_n, 0, 4, s), "hipMemsetAsync");
    HIP_TRY(hipMemsetAsync(has + cur_n, 0, 4, s), "hipMemsetAsync");
    if (gen.decided) HIP_TRY(ws.get(W::kQFlag + x, cur_n, (void**)&flag[L]), "device allocation (quiescence scratch)");
    gen.count(cur, cur_active, cur_n, cnt, has, flag[L], res[L - 1], evas ? evas + 2 * x : nullptr, s);
    HIP_TRY(hipGetLastError(), "capture_count launch");
    HIP_TRY(builder_exclusive_scan(cnt, roff[L], cur_n, s, ws), "capture scan");
    HIP_TRY(builder_exclusive_scan(has, gidx[L], cur_n, s, ws), "capture scan");
    uint32_t sizes[2] = {0, 0};
    HIP_TRY(hipMemcpyAsync(&sizes[0], roff[L] + cur_n, 4, hipMemcpyDeviceToHost, s), "D2H(level size)");
    HIP_TRY(hipMemcpyAsync(&sizes[1], gidx[L] + cur_n, 4, hipMemcpyDeviceToHost, s), "D2H(level size)");
    HIP_TRY(hipStreamSynchronize(s), "hipStreamSynchronize");
    if (st) ++st->syncs;
    const uint32_t total = sizes[0], ngroups = sizes[1];
    if (total == 0) break;  // no capture anywhere: the level above is the deepest
    if (total > budget && b - a > 1) {
      *overflow = total;
      tm.mark(Marks::kEnd);
      return FNNUE_OK;
    }
    const uint32_t nkid = total - ngroups;
    void* pos = nullptr;
    uint32_t* goff = nullptr;
    int32_t *ps = nullptr, *po = nullptr;
    void* next = nullptr;
    HIP_TRY(ws.get(W::kQPos, (size_t)total * gen.record_bytes, &pos), "device allocation (quiescence scratch)");
    HIP_TRY(ws.get(W::kQGoff, ((size_t)ngroups + 1) * 4, (void**)&goff), "device allocation (quiescence scratch)");
    HIP_TRY(ws.get(W::kQPsqt, (size_t)total * 4, (void**)&ps), "device allocation (quiescence scratch)");
    HIP_TRY(ws.get(W::kQPositional, (size_t)total * 4, (void**)&po), "device allocation (quiescence scratch)");
    HIP_TRY(ws.get(W::kQMoves + x, (size_t)total * 2, (void**)&moves[L]), "device allocation (quiescence scratch)");
    HIP_TRY(ws.get(W::kQRes + x, (size_t)nkid * sizeof(fnnue_quiet), (void**)&res[L]),
            "device allocation (quiescence scratch)");
    if (L < depth || gen.decided)  // the decided form keeps the last level's boards too: they are probed below
      HIP_TRY(ws.get(W::kQBoards + x, (size_t)nkid * gen.board_bytes, &next), "device allocation (quiescence scratch)");
    gen.write(cur, cur_n, roff[L], gidx[L], total, ngroups, pos, moves[L], goff, next, flag[L], s);
    HIP_TRY(hipGetLastError(), "capture_write launch");
    tm.mark(Marks::kEval);
    if (int rc = gen.variant ? fnnue_eval_vgroups_device(ctx, static_cast<const fnnue_vpos*>(pos), goff, ngroups, total,
                                                         FNNUE_GROUP_STAR, ps, po, s)
                             : fnnue_eval_groups_device(ctx, static_cast<const fnnue_pos*>(pos), goff, ngroups, total,
                                                        FNNUE_GROUP_STAR, ps, po, s))
      return rc;
    tm.mark(Marks::kReduce);
    hipLaunchKernelGGL(quiet_leaves_kernel, grid_for(cur_n, kBlock), dim3(kBlock), 0, s, roff[L], gidx[L], cur_n, ps,
                       po, res[L]);
    HIP_TRY(hipGetLastError(), "quiet_leaves launch");
    if (gen.decided && L == depth) {  // the horizon: a mated or finished child is so at depth 0 as well
      gen.probe(next, nkid, res[L], s);
      HIP_TRY(hipGetLastError(), "mate_probe launch");
    }
    level_n[L] = cur_n;
    recs[L] = total;
    deepest = L;
    cur = next;
    cur_active = nullptr;
    cur_n = nkid;
  }
  tm.mark(Marks::kReduce);
  for (int L = deepest; L >= 1; --L) {
    gen.reduce(roff[L], gidx[L], level_n[L], moves[L], res[L], res[L - 1], flag[L], s);
    HIP_TRY(hipGetLastError(), "quiet_reduce launch");
  }
  tm.mark(Marks::kEnd);
  if (st)
    for (int L = 1; L <= deepest; ++L) st->level_records[L - 1] += recs[L];
  if (evas) {  // the trace only: one more wait
    unsigned long long h[2 * FNNUE_QUIESCE_MAX] = {};
    HIP_TRY(hipMemcpyAsync(h, evas, sizeof(h), hipMemcpyDeviceToHost, s), "D2H(evasion counters)");
    HIP_TRY(hipStreamSynchronize(s), "hipStreamSynchronize");
    for (int l = 0; l < FNNUE_QUIESCE_MAX; ++l) {
      st->level_evasions[l] += h[2 * l];
      st->level_in_check[l] += h[2 * l + 1];
    }
  }
  return FNNUE_OK;
}

// Every root in slices of whole roots: a slice whose tree passes the budget at
// some level is cut down (to what the level's size says fits, at most to half)
// and redone; the next slice starts with the size that fit.
int quiesce_frontier(fnnue_ctx* ctx, W& ws, const Gen& gen, const void* roots, const uint8_t* active, size_t n,
                     fnnue_quiet* res0, int depth, hipStream_t s, QuiesceStats* st, Marks& tm) {
  const size_t budget = quiesce_budget();
  size_t step = std::min(n, budget);
  for (size_t a = 0; a < n;) {
    size_t b = std::min(n, a + step);
    for (;;) {
      size_t overflow = 0;  // the records of the level that passed the bound
      if (int rc = quiesce_slice(ctx, ws, gen, roots, active, a, b, res0, depth, budget, s, st, tm, &overflow)) return rc;
      if (!overflow) break;
      const size_t fits = (size_t)((double)(b - a) * (double)budget / (double)overflow * 0.875);
      step = std::max<size_t>(1, std::min(fits, (b - a) / 2));
      b = a + step;
      if (st) ++st->redone;
    }
    if (st) ++st->slices;
    ++ctx->quiesce_slices;
    a = b;
  }
  return FNNUE_OK;
}

}  // namespace

size_t quiesce_budget() {
  size_t n = (size_t)16 << 20;
  if (const char* e = std::getenv("FNNUE_QUIESCE_RECORDS")) n = (size_t)std::max(0LL, std::atoll(e));
  return std::min<size_t>(std::max(n, kQuiesceMinRecords), (size_t)16 << 20);
}

int quiesce_leaves_device(fnnue_ctx* ctx, BuilderScratch& ws, SearchRules rules, const void* d_parents, uint32_t n,
                          const uint32_t* d_off, uint32_t total, const uint8_t* d_end, int32_t* d_psqt,
                          int32_t* d_positional, int depth, bool checks, int ply, hipStream_t s, QuiesceStats* st) {
  if (depth <= 0 || n == 0 || total <= n) return FNNUE_OK;
  if (depth > FNNUE_QUIESCE_MAX) return fail(FNNUE_E_ARG, "quiescence depth above FNNUE_QUIESCE_MAX");
  Gen gen;
  if (!gen_for(rules, checks, &gen)) return fail(FNNUE_E_ARCH, "no capture quiescence for this variant");
  const uint32_t nleaf = total - n;
  void* roots = nullptr;
  uint2* map = nullptr;
  uint8_t* active = nullptr;
  fnnue_quiet* res0 = nullptr;
  HIP_TRY(ws.get(W::kQRoots, (size_t)nleaf * gen.board_bytes, &roots), "device allocation (quiescence scratch)");
  HIP_TRY(ws.get(W::kQMap, (size_t)nleaf * sizeof(uint2), (void**)&map), "device allocation (quiescence scratch)");
  HIP_TRY(ws.get(W::kQActive, nleaf, (void**)&active), "device allocation (quiescence scratch)");
  HIP_TRY(ws.get(W::kQRes0, (size_t)nleaf * sizeof(fnnue_quiet), (void**)&res0),
          "device allocation (quiescence scratch)");
  Marks tm;
  tm.on = st && st->timed;
  tm.s = s;
  tm.mark(Marks::kRoots);
  HIP_TRY(child_states(rules, d_parents, n, d_off, total, roots, map, s), "child_states launch");
  // a variant's FNNUE_END_WON children have no move either: NO_MOVES covers them
  hipLaunchKernelGGL(leaf_init_kernel, grid_for(nleaf, kBlock), dim3(kBlock), 0, s, map, d_off, d_end, d_psqt,
                     d_positional, nleaf, res0, active);
  HIP_TRY(hipGetLastError(), "leaf_init launch");
  if (int rc = quiesce_frontier(ctx, ws, gen, roots, active, nleaf, res0, depth, s, st, tm)) return rc;
  tm.mark(Marks::kRoots);
  gen.scatter(map, d_off, active, res0, nleaf, d_psqt, d_positional, (int32_t)ply, s);
  HIP_TRY(hipGetLastError(), "leaf_scatter launch");
  tm.mark(Marks::kEnd);
  tm.report(st);
  return FNNUE_OK;
}

int quiesce_nodes_device(fnnue_ctx* ctx, BuilderScratch& ws, SearchRules rules, const void* d_states, uint32_t n,
                         int depth, bool checks, fnnue_quiet* d_out, hipStream_t s, QuiesceStats* st) {
  if (n == 0) return FNNUE_OK;
  if (depth < 0 || depth > FNNUE_QUIESCE_MAX) return fail(FNNUE_E_ARG, "quiescence depth above FNNUE_QUIESCE_MAX");
  Gen gen;
  if (!gen_for(rules, checks, &gen)) return fail(FNNUE_E_ARCH, "no capture quiescence for this variant");
  void* pos = nullptr;
  int32_t *ps = nullptr, *po = nullptr;
  HIP_TRY(ws.get(W::kQRoots, (size_t)n * gen.record_bytes, &pos), "device allocation (quiescence scratch)");
  HIP_TRY(ws.get(W::kQMap, (size_t)n * 4, (void**)&ps), "device allocation (quiescence scratch)");
  HIP_TRY(ws.get(W::kQRes0, (size_t)n * 4, (void**)&po), "device allocation (quiescence scratch)");
  gen.pack(d_states, n, pos, s);
  HIP_TRY(hipGetLastError(), "pack_boards launch");
  if (int rc = gen.variant ? fnnue_eval_vpositions_device(ctx, static_cast<const fnnue_vpos*>(pos), n, ps, po, s)
                           : fnnue_eval_positions_device(ctx, static_cast<const fnnue_pos*>(pos), n, ps, po, s))
    return rc;
  hipLaunchKernelGGL(node_init_kernel, grid_for(n, kBlock), dim3(kBlock), 0, s, ps, po, n, d_out);
  HIP_TRY(hipGetLastError(), "node_init launch");
  if (depth == 0) {
    if (gen.decided) {  // a mated or finished ply is so at depth 0 as well
      gen.probe(d_states, n, d_out, s);
      HIP_TRY(hipGetLastError(), "mate_probe launch");
    }
    return FNNUE_OK;
  }
  Marks tm;  // untimed
  return quiesce_frontier(ctx, ws, gen, d_states, nullptr, n, d_out, depth, s, st, tm);
}

}  // namespace fnnue
