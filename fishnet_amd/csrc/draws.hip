// draws.hip — repetition and fifty-move draws in the device search (ABI 3.12;
// the variants: ABI 3.16; the rules: include/fnnue.h).
//
// The history: the replay leaves every ply's board on the device, so a ply's
// clock and the number of earlier plies with its identity follow from the
// boards alone, without touching the replay.
//   root_clocks_kernel   one thread per game: the FEN's fifth field
//   ply_keys_kernel      one thread per ply: the 63-bit key of its identity, and
//                        in bit 63 whether the move that led to it was
//                        irreversible (piece count or pawn sets changed against
//                        the ply before)
//   ply_walk_kernel      one thread per ply: back to the last irreversible move
//                        (the window: equal identities cannot straddle one) for
//                        the clock, and over the window's plies of its own
//                        parity for `seen`, each key match confirmed on the boards
//   ply_list_kernel      one thread per ply: can a child or grandchild be drawn
//                        at all (clock >= 98, or a ply of the window that has
//                        been seen before)?  Those plies are appended to a list.
// The marking passes run over that list only: a block per listed ply, a thread
// per record, the record's move code applied to its parent's board (no move
// generation), its clock and identity compared with the ply's window, and
// FNNUE_END_DRAW ORed into the record's end byte.  On ordinary games the list
// is empty and every block returns after one load.
//
// The variants: what depends on the board (identity, key, reversibility,
// applying a code) is a rule set R, as quiesce.hip's generators have one.
//   DBoardDraws<V>  chess, and kingofthehill / racingkings / threecheck on the
//                   same boards.  threecheck's identity has the check counters
//                   (bt[0]) and its codes are played with do_move_v, which
//                   spends them.
//   VBoardDraws<V>  atomic and crazyhouse on vboard.h's boards.  Crazyhouse has
//                   no clock and no irreversible move: both pockets and the
//                   promoted marks belong to the identity, every window starts
//                   at the game's root (so the list holds a ply as soon as any
//                   ply up to it has been seen before), and a code with
//                   from == to drops the piece in its promo field.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdlib>

#include "board.h"
#include "builder.h"
#include "chess_rules.h"
#include "search_steps.h"
#include "vboard.h"

namespace fnnue {

namespace {

constexpr uint32_t kBlock = 256, kMarkBlocks = 512;
constexpr uint64_t kIrreversible = 1ull << 63;
static_assert(sizeof(fnnue_ply_history) == 4, "fnnue_ply_history is one dword");

// The en-passant square as the identity counts it: only when a pawn of the
// side to move attacks it.
__device__ __forceinline__ int32_t ident_ep(const DBoard& b) {
  if (b.ep < 0 || b.ep > 63) return -1;
  const int us = (int)b.stm;
  return (pawn_att(us ^ 1, b.ep) & b.bt[PAWN] & colour(b, us)) ? b.ep : -1;
}

__device__ __forceinline__ uint64_t mix64(uint64_t z) {  // splitmix64's finaliser
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

template <int V>
__device__ __forceinline__ uint64_t ident_key(const DBoard& b, int32_t ep, uint64_t mask) {
  uint64_t h = 0x9E3779B97F4A7C15ull;
  h = mix64(h ^ b.bc[0]);
  h = mix64(h ^ b.bc[1]);
#pragma unroll
  for (int t = PAWN; t <= KING; ++t) h = mix64(h ^ b.bt[t]);
  if constexpr (V == kVariantThreeCheck) h = mix64(h ^ b.bt[0]);  // both check counters
  h = mix64(h ^ ((uint64_t)b.cr | (uint64_t)(b.stm & 1u) << 32 | (uint64_t)(uint32_t)(ep + 1) << 40));
  return h & mask;
}

// b's identity against x's (xep: x's counted en-passant square).
template <int V>
__device__ __forceinline__ bool same_identity(const DBoard& x, int32_t xep, const DBoard& b) {
  bool eq = x.bc[0] == b.bc[0] && x.bc[1] == b.bc[1] && x.stm == b.stm && x.cr == b.cr;
#pragma unroll
  for (int t = PAWN; t <= KING; ++t) eq = eq && x.bt[t] == b.bt[t];
  if constexpr (V == kVariantThreeCheck) eq = eq && x.bt[0] == b.bt[0];
  return eq && xep == ident_ep(b);
}

// Was the move between two consecutive boards a pawn move or a capture?
__device__ __forceinline__ bool irreversible_between(const DBoard& before, const DBoard& after) {
  return before.bt[PAWN] != after.bt[PAWN] ||
         __popcll(before.bc[0] | before.bc[1]) != __popcll(after.bc[0] | after.bc[1]);
}

__device__ __forceinline__ uint32_t clock_up(uint32_t c) { return c >= 65535u ? 65535u : c + 1u; }

// The move a code names on b (ChessRules::step's reading: the own king onto a
// castling rook's square, or in a standard game onto its two-square destination,
// castles), played on c under V's rules; irreversible: a pawn move or a capture.
template <int V>
__device__ __forceinline__ void apply_code(const DBoard& b, uint32_t code, DBoard& c, bool& irreversible) {
  const int from = (int)(code & 63u), to = (int)((code >> 6) & 63u), promo = (int)((code >> 12) & 7u);
  const int us = (int)b.stm, back = us == WHITE ? 0 : 56;
  const uint64_t fm = 1ull << from, tm = 1ull << to;
  int rsq = -1;
  if ((b.bt[KING] & fm) && !promo) {
#pragma unroll
    for (int side = 0; side < 2; ++side) {
      const int r = cr_get(b, us, side);
      if (rsq < 0 && r >= 0 && (to == r || (!b.c960 && to == back + (side == 0 ? 6 : 2)))) rsq = r;
    }
  }
  irreversible = rsq < 0 && ((b.bt[PAWN] & fm) || ((b.bc[0] | b.bc[1]) & tm));
  const DMove m{from, rsq >= 0 ? rsq : to, promo, rsq >= 0 ? 1 : 0};
  c = b;
  do_move_v<V>(c, m);
}

// Chess (V = kVariantChess) and the variants whose moves are chess moves.
template <int V>
struct DBoardDraws {
  using Board = DBoard;
  static constexpr bool kClocked = true;
  // threecheck: the clock is the first field from the fifth on without a '+'
  static constexpr bool kSkipPlus = V == kVariantThreeCheck;
  __device__ static int32_t ep(const Board& b) { return ident_ep(b); }
  __device__ static uint64_t key(const Board& b, int32_t e, uint64_t mask) { return ident_key<V>(b, e, mask); }
  __device__ static bool same(const Board& x, int32_t xep, const Board& b) { return same_identity<V>(x, xep, b); }
  __device__ static bool irreversible(const Board& before, const Board& after) {
    return irreversible_between(before, after);
  }
  __device__ static void apply(const Board& b, uint32_t code, Board& c, bool& irr) { apply_code<V>(b, code, c, irr); }
};

// ---- vboard.h's boards: atomic and crazyhouse ----
__device__ __forceinline__ int32_t vident_ep(const vb::VBoard& b) {
  if (b.ep < 0 || b.ep > 63) return -1;
  const int us = (int)b.stm;
  return (vb::pawn_att(us ^ 1, b.ep) & b.bt[vb::PAWN] & vb::colour(b, us)) ? (int32_t)b.ep : -1;
}
__device__ __forceinline__ uint32_t vrights(const vb::VBoard& b) {  // the four castling rooks as one word
  return (uint32_t)(uint8_t)b.cr[0][0] | (uint32_t)(uint8_t)b.cr[0][1] << 8 | (uint32_t)(uint8_t)b.cr[1][0] << 16 |
         (uint32_t)(uint8_t)b.cr[1][1] << 24;
}

template <int V>
struct VBoardDraws {
  using Board = vb::VBoard;
  static constexpr bool kHands = V == kVariantCrazyhouse;
  static constexpr bool kClocked = !kHands;
  static constexpr bool kSkipPlus = false;
  __device__ static int32_t ep(const Board& b) { return vident_ep(b); }
  __device__ static uint64_t key(const Board& b, int32_t e, uint64_t mask) {
    uint64_t h = 0x9E3779B97F4A7C15ull;
    h = mix64(h ^ b.bc[0]);
    h = mix64(h ^ b.bc[1]);
#pragma unroll
    for (int t = vb::PAWN; t <= vb::KING; ++t) h = mix64(h ^ b.bt[t]);
    if constexpr (kHands) {
      h = mix64(h ^ b.pocket[0]);
      h = mix64(h ^ b.pocket[1]);
      h = mix64(h ^ b.promoted);
    }
    h = mix64(h ^ ((uint64_t)vrights(b) | (uint64_t)(b.stm & 1u) << 32 | (uint64_t)(uint32_t)(e + 1) << 40));
    return h & mask;
  }
  __device__ static bool same(const Board& x, int32_t xep, const Board& b) {
    bool eq = x.bc[0] == b.bc[0] && x.bc[1] == b.bc[1] && x.stm == b.stm && vrights(x) == vrights(b);
#pragma unroll
    for (int t = vb::PAWN; t <= vb::KING; ++t) eq = eq && x.bt[t] == b.bt[t];
    if constexpr (kHands) eq = eq && x.pocket[0] == b.pocket[0] && x.pocket[1] == b.pocket[1] && x.promoted == b.promoted;
    return eq && xep == vident_ep(b);
  }
  // a pawn move, a capture or (atomic) an explosion; crazyhouse: never
  __device__ static bool irreversible(const Board& before, const Board& after) {
    if constexpr (kHands) return false;
    return before.bt[vb::PAWN] != after.bt[vb::PAWN] ||
           __popcll(vb::occupied(before)) != __popcll(vb::occupied(after));
  }
  // The move a code names on b, as vb::move_code writes it: from == to drops
  // the piece in the promo field; the own king onto a castling rook's square, or
  // in a standard game onto its two-square destination, castles.
  __device__ static void apply(const Board& b, uint32_t code, Board& c, bool& irr) {
    const int from = (int)(code & 63u), to = (int)((code >> 6) & 63u), promo = (int)((code >> 12) & 7u);
    const int us = (int)b.stm, back = us == 0 ? 0 : 56;
    const uint64_t fm = 1ull << from, tm = 1ull << to;
    c = b;
    if (kHands && from == to) {
      irr = false;
      vb::do_move(c, vb::VMove{(int8_t)-1, (int8_t)to, (int8_t)promo, (int8_t)2});
      return;
    }
    int rsq = -1;
    if ((b.bt[vb::KING] & fm) && !promo) {
#pragma unroll
      for (int side = 0; side < 2; ++side) {
        const int r = vb::cr_get(b, us, side);
        if (rsq < 0 && r >= 0 && (to == r || (!b.c960 && to == back + (side == 0 ? 6 : 2)))) rsq = r;
      }
    }
    irr = !kHands && rsq < 0 && ((b.bt[vb::PAWN] & fm) || (vb::occupied(b) & tm));
    vb::do_move(c, vb::VMove{(int8_t)from, (int8_t)(rsq >= 0 ? rsq : to), (int8_t)(rsq >= 0 ? 0 : promo),
                             (int8_t)(rsq >= 0 ? 1 : 0)});
  }
};

// kSkipPlus (threecheck): fields with a '+' (the check counters, "3+3" or
// "+0+0") are passed over, so the clock is the first field from the fifth on
// without one.
template <bool kSkipPlus>
__global__ void root_clocks_kernel(const char* __restrict__ text, const uint32_t* __restrict__ fen_off,
                                   const uint32_t* __restrict__ mv_off, uint32_t ngames,
                                   uint32_t* __restrict__ clock0) {
  const uint32_t g = blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= ngames) return;
  uint32_t p = fen_off[g], st = 0;
  const uint32_t end = mv_off[g];
  int len = 0;
  for (int field = 0; field < 5; ++field) len = next_token(text, p, end, st);  // 0 once the text has run out
  if constexpr (kSkipPlus) {
    for (;;) {
      bool plus = false;
      for (int i = 0; i < len; ++i) plus = plus || text[st + i] == '+';
      if (!plus) break;
      len = next_token(text, p, end, st);
    }
  }
  uint32_t v = 0;
  bool number = len > 0;
  for (int i = 0; i < len; ++i) {
    const char ch = text[st + i];
    if (ch < '0' || ch > '9') number = false;
    else v = v * 10u + (uint32_t)(ch - '0') > 65535u ? 65535u : v * 10u + (uint32_t)(ch - '0');
  }
  clock0[g] = number ? v : 0u;
}

// The game of ply p: ply_off[g] <= p < ply_off[g + 1] (every game has a ply).
__device__ __forceinline__ uint32_t game_of(const uint32_t* __restrict__ ply_off, uint32_t ngames, uint32_t p) {
  uint32_t lo = 0, hi = ngames;
  while (hi - lo > 1) {
    const uint32_t mid = (lo + hi) >> 1;
    if (ply_off[mid] <= p) lo = mid;
    else hi = mid;
  }
  return lo;
}

template <class R>
__global__ __launch_bounds__(kBlock) void ply_keys_kernel(const typename R::Board* __restrict__ states, uint32_t n,
                                                          const uint32_t* __restrict__ ply_off, uint32_t ngames,
                                                          uint64_t mask, uint64_t* __restrict__ keys) {
  const uint32_t p = blockIdx.x * kBlock + threadIdx.x;
  if (p >= n) return;
  const typename R::Board b = states[p];
  uint64_t key = R::key(b, R::ep(b), mask);
  if constexpr (R::kClocked) {
    if (p > ply_off[game_of(ply_off, ngames, p)] && R::irreversible(states[p - 1], b)) key |= kIrreversible;
  }
  keys[p] = key;
}

template <class R>
__global__ __launch_bounds__(kBlock) void ply_walk_kernel(const typename R::Board* __restrict__ states, uint32_t n,
                                                          const uint32_t* __restrict__ ply_off, uint32_t ngames,
                                                          const uint32_t* __restrict__ clock0,
                                                          const uint64_t* __restrict__ keys, uint32_t* __restrict__ lo,
                                                          fnnue_ply_history* __restrict__ hist) {
  const uint32_t p = blockIdx.x * kBlock + threadIdx.x;
  if (p >= n) return;
  const uint32_t g = game_of(ply_off, ngames, p), first = ply_off[g];
  uint32_t r = p;  // the window's first ply: the last irreversible move's, or the root
  uint64_t clock = 0;
  if constexpr (R::kClocked) {
    while (r > first && !(keys[r] & kIrreversible)) --r;
    clock = keys[r] & kIrreversible ? (uint64_t)(p - r) : (uint64_t)clock0[g] + (p - first);
  } else {
    r = first;  // no move makes a position unreachable: the whole game
  }
  const uint64_t mine = keys[p] & ~kIrreversible;
  uint32_t seen = 0;
  if (p - r >= 2) {  // the plies of p's own side to move
    const typename R::Board b = states[p];
    const int32_t ep = R::ep(b);
    for (uint32_t q = p - 2;; q -= 2) {
      if ((keys[q] & ~kIrreversible) == mine && R::same(b, ep, states[q])) ++seen;
      if (q < r + 2) break;
    }
  }
  lo[p] = r;
  fnnue_ply_history h;
  h.clock = (uint16_t)(clock > 65535 ? 65535 : clock);
  h.seen = (uint8_t)(seen > 255u ? 255u : seen);
  h.reserved = 0;
  hist[p] = h;
}

// A child X of P repeats for the third time only when an identity stands twice
// among the plies [lo, P] already, i.e. one of them has been seen before; a
// grandchild the same.  Its clock reaches 100 only from 98 (two moves) up.
__global__ __launch_bounds__(kBlock) void ply_list_kernel(uint32_t n, const uint32_t* __restrict__ lo,
                                                          const fnnue_ply_history* __restrict__ hist,
                                                          uint32_t* __restrict__ list) {
  const uint32_t p = blockIdx.x * kBlock + threadIdx.x;
  if (p >= n) return;
  bool any = hist[p].clock >= 98;
  const uint32_t r = lo[p];
  for (uint32_t q = p; !any && q > r; --q) any = hist[q].seen != 0;  // ply r itself follows an irreversible move
  if (any) list[1 + atomicAdd(&list[0], 1u)] = p;
}

// Is the searched position x drawn?  clock: x's; reversible: every move of the
// path from ply P was (else nothing before it can equal x); f: x's end byte.
template <class R>
__device__ __forceinline__ bool drawn(const typename R::Board& x, uint32_t clock, bool reversible, uint32_t f,
                                      const typename R::Board* __restrict__ states,
                                      const uint64_t* __restrict__ keys, uint64_t mask, uint32_t r, uint32_t P) {
  if ((f & kFinalWon) || ((f & kFinalNoMoves) && (f & (kFinalCheck | kFinalExtinct | kFinalVariant)))) return false;
  if (clock >= 100) return true;
  if (!reversible) return false;
  const int32_t ep = R::ep(x);
  const uint64_t key = R::key(x, ep, mask);
  uint32_t seen = 0;
  for (uint32_t q = P;; --q) {  // the other side's plies never match: the side to move is part of the key's input
    if ((keys[q] & ~kIrreversible) == key && R::same(x, ep, states[q]) && ++seen >= 2) return true;
    if (q == r) break;
  }
  return false;
}

template <class R>
__global__ __launch_bounds__(kBlock) void mark_level1_kernel(
    const uint32_t* __restrict__ list, const fnnue_ply_history* __restrict__ hist, const uint64_t* __restrict__ keys,
    const uint32_t* __restrict__ lo, uint64_t mask, const typename R::Board* __restrict__ states, uint32_t n,
    const uint32_t* __restrict__ off, const uint16_t* __restrict__ moves, uint8_t* __restrict__ end) {
  const uint32_t count = list[0] < n ? list[0] : n;
  for (uint32_t i = blockIdx.x; i < count; i += gridDim.x) {
    const uint32_t P = list[1 + i];
    if (P >= n) continue;
    const uint32_t o = off[P], e = off[P + 1];
    if (e - o < 2 || e < o) continue;
    const typename R::Board b = states[P];
    const uint32_t clock = hist[P].clock, r = lo[P];
    for (uint32_t c = 1 + threadIdx.x; c < e - o; c += kBlock) {
      typename R::Board x;
      bool irr;
      R::apply(b, moves[o + c], x, irr);
      const uint32_t f = end[o + c];
      if (drawn<R>(x, irr ? 0u : clock_up(clock), !irr, f, states, keys, mask, r, P))
        end[o + c] = (uint8_t)(f | kFinalDraw);
    }
  }
}

template <class R>
__global__ __launch_bounds__(kBlock) void mark_level2_kernel(
    const uint32_t* __restrict__ list, const fnnue_ply_history* __restrict__ hist, const uint64_t* __restrict__ keys,
    const uint32_t* __restrict__ lo, uint64_t mask, const typename R::Board* __restrict__ states, uint32_t p0,
    uint32_t p1, const uint32_t* __restrict__ off, const typename R::Board* __restrict__ kid_states,
    const uint32_t* __restrict__ kid_off, uint32_t rec0, const uint16_t* __restrict__ gmoves,
    uint8_t* __restrict__ gend) {
  const uint32_t count = list[0];
  for (uint32_t i = blockIdx.x; i < count; i += gridDim.x) {
    const uint32_t P = list[1 + i];
    if (P < p0 || P >= p1) continue;
    const uint32_t d0 = off[P] - P, d1 = off[P + 1] - (P + 1);  // the ply's children in the dense array
    if (d1 <= d0) continue;
    const typename R::Board b = states[P];
    const uint32_t clock = hist[P].clock, r = lo[P];
    const uint32_t r0 = kid_off[d0], r1 = kid_off[d1];
    for (uint32_t rr = r0 + threadIdx.x; rr < r1; rr += kBlock) {
      uint32_t dl = d0, dh = d1;  // kid_off[dl] <= rr < kid_off[dh]
      while (dh - dl > 1) {
        const uint32_t mid = (dl + dh) >> 1;
        if (kid_off[mid] <= rr) dl = mid;
        else dh = mid;
      }
      if (rr == kid_off[dl]) continue;  // the child's own record: level 1's
      const typename R::Board c = kid_states[dl];
      const bool irr1 = R::irreversible(b, c);
      const uint32_t cclock = irr1 ? 0u : clock_up(clock);
      typename R::Board x;
      bool irr2;
      R::apply(c, gmoves[rr - rec0], x, irr2);
      const uint32_t f = gend[rr - rec0];
      if (drawn<R>(x, irr2 ? 0u : clock_up(cclock), !irr1 && !irr2, f, states, keys, mask, r, P))
        gend[rr - rec0] = (uint8_t)(f | kFinalDraw);
    }
  }
}

__global__ __launch_bounds__(kBlock) void own_terms_kernel(const uint32_t* __restrict__ list, uint32_t p0, uint32_t p1,
                                                           const uint32_t* __restrict__ off,
                                                           const uint8_t* __restrict__ end,
                                                           const uint32_t* __restrict__ kid_off, uint32_t rec0,
                                                           const int32_t* __restrict__ gps,
                                                           const int32_t* __restrict__ gpo,
                                                           uint32_t* __restrict__ kid_best) {
  const uint32_t count = list[0];
  for (uint32_t i = blockIdx.x; i < count; i += gridDim.x) {
    const uint32_t P = list[1 + i];
    if (P < p0 || P >= p1) continue;
    const uint32_t o = off[P], e = off[P + 1];
    for (uint32_t c = 1 + threadIdx.x; c < e - o; c += kBlock) {
      if (!(end[o + c] & kFinalDraw)) continue;
      const uint32_t d = o - P + c - 1, rr = kid_off[d] - rec0;
      kid_best[(size_t)d * 6 + 0] = (uint32_t)gps[rr];
      kid_best[(size_t)d * 6 + 1] = (uint32_t)gpo[rr];
    }
  }
}

uint64_t key_mask(uint32_t bits) { return bits >= 63 ? ~kIrreversible : (1ull << (bits ? bits : 1)) - 1; }

// f(R{}) with the rule set of `variant` (a known one: the callers' searches checked it).
template <class F>
void with_rules(int variant, F&& f) {
  switch (variant) {
    case kVariantCrazyhouse: f(VBoardDraws<kVariantCrazyhouse>{}); break;
    case kVariantAtomic: f(VBoardDraws<kVariantAtomic>{}); break;
    case kVariantKingOfTheHill: f(DBoardDraws<kVariantKingOfTheHill>{}); break;
    case kVariantRacingKings: f(DBoardDraws<kVariantRacingKings>{}); break;
    case kVariantThreeCheck: f(DBoardDraws<kVariantThreeCheck>{}); break;
    default: f(DBoardDraws<kVariantChess>{}); break;
  }
}

}  // namespace

uint32_t draw_key_bits() {
  const char* e = std::getenv("FNNUE_DRAW_KEY_BITS");
  if (!e || !*e) return 63;
  const long v = std::atol(e);
  return v < 1 ? 1u : v > 63 ? 63u : (uint32_t)v;
}

hipError_t game_history_device(SearchRules rules, const char* d_text, const uint32_t* d_fen_off,
                               const uint32_t* d_mv_off, const uint32_t* d_ply_off, uint32_t ngames,
                               const void* d_states, uint32_t n, uint32_t key_bits, hipStream_t s, BuilderScratch& ws,
                               DrawHistory* out) {
  using W = BuilderScratch;
  hipError_t e;
  uint32_t *clock0 = nullptr, *lo = nullptr, *list = nullptr;
  uint64_t* keys = nullptr;
  fnnue_ply_history* hist = nullptr;
  if ((e = ws.get(W::kDrawClock0, (size_t)(ngames + 1) * 4, (void**)&clock0)) != hipSuccess) return e;
  if ((e = ws.get(W::kDrawKeys, (size_t)(n + 1) * 8, (void**)&keys)) != hipSuccess) return e;
  if ((e = ws.get(W::kDrawLo, (size_t)(n + 1) * 4, (void**)&lo)) != hipSuccess) return e;
  if ((e = ws.get(W::kDrawHist, (size_t)(n + 1) * sizeof(fnnue_ply_history), (void**)&hist)) != hipSuccess) return e;
  if ((e = ws.get(W::kDrawList, (size_t)(n + 1) * 4, (void**)&list)) != hipSuccess) return e;
  if ((e = hipMemsetAsync(list, 0, 4, s)) != hipSuccess) return e;
  out->hist = hist;
  out->keys = keys;
  out->lo = lo;
  out->list = list;
  out->key_bits = key_bits;
  if (n == 0 || ngames == 0) return hipSuccess;
  const uint64_t mask = key_mask(key_bits);
  const dim3 per_ply((n + kBlock - 1) / kBlock);
  with_rules(rules.variant, [&](auto r) {
    using R = decltype(r);
    using B = typename R::Board;
    if constexpr (R::kClocked)  // crazyhouse reads no clock
      hipLaunchKernelGGL(root_clocks_kernel<R::kSkipPlus>, dim3((ngames + 63) / 64), dim3(64), 0, s, d_text, d_fen_off,
                         d_mv_off, ngames, clock0);
    hipLaunchKernelGGL(ply_keys_kernel<R>, per_ply, dim3(kBlock), 0, s, static_cast<const B*>(d_states), n, d_ply_off,
                       ngames, mask, keys);
    hipLaunchKernelGGL(ply_walk_kernel<R>, per_ply, dim3(kBlock), 0, s, static_cast<const B*>(d_states), n, d_ply_off,
                       ngames, clock0, keys, lo, hist);
  });
  hipLaunchKernelGGL(ply_list_kernel, per_ply, dim3(kBlock), 0, s, n, lo, hist, list);
  return hipGetLastError();
}

hipError_t mark_draws_level1(SearchRules rules, const DrawHistory& h, const void* d_states, uint32_t n,
                             const uint32_t* d_off, const uint16_t* d_moves, uint8_t* d_end, hipStream_t s) {
  if (n == 0) return hipSuccess;
  with_rules(rules.variant, [&](auto r) {
    using R = decltype(r);
    hipLaunchKernelGGL(mark_level1_kernel<R>, dim3(std::min(n, kMarkBlocks)), dim3(kBlock), 0, s, h.list, h.hist, h.keys,
                       h.lo, key_mask(h.key_bits), static_cast<const typename R::Board*>(d_states), n, d_off, d_moves,
                       d_end);
  });
  return hipGetLastError();
}

hipError_t mark_draws_level2(SearchRules rules, const DrawHistory& h, const void* d_states, uint32_t p0, uint32_t p1,
                             const uint32_t* d_off, const void* d_kid_states, const uint32_t* d_kid_off, uint32_t rec0,
                             const uint16_t* d_gmoves, uint8_t* d_gend, hipStream_t s) {
  if (p1 <= p0) return hipSuccess;
  with_rules(rules.variant, [&](auto r) {
    using R = decltype(r);
    using B = typename R::Board;
    hipLaunchKernelGGL(mark_level2_kernel<R>, dim3(std::min(p1 - p0, kMarkBlocks)), dim3(kBlock), 0, s, h.list, h.hist,
                       h.keys, h.lo, key_mask(h.key_bits), static_cast<const B*>(d_states), p0, p1, d_off,
                       static_cast<const B*>(d_kid_states), d_kid_off, rec0, d_gmoves, d_gend);
  });
  return hipGetLastError();
}

hipError_t draw_own_terms(const DrawHistory& h, uint32_t p0, uint32_t p1, const uint32_t* d_off, const uint8_t* d_end,
                          const uint32_t* d_kid_off, uint32_t rec0, const int32_t* d_gps, const int32_t* d_gpo,
                          fnnue_best* d_kid_best, hipStream_t s) {
  if (p1 <= p0) return hipSuccess;
  hipLaunchKernelGGL(own_terms_kernel, dim3(std::min(p1 - p0, kMarkBlocks)), dim3(kBlock), 0, s, h.list, p0, p1, d_off,
                     d_end, d_kid_off, rec0, d_gps, d_gpo, reinterpret_cast<uint32_t*>(d_kid_best));
  return hipGetLastError();
}

}  // namespace fnnue
