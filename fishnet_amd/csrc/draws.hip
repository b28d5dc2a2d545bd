// draws.hip — repetition and fifty-move draws in the device search (ABI 3.12;
// the rule: include/fnnue.h).
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
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdlib>

#include "board.h"
#include "builder.h"
#include "chess_rules.h"

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

__device__ __forceinline__ uint64_t ident_key(const DBoard& b, int32_t ep, uint64_t mask) {
  uint64_t h = 0x9E3779B97F4A7C15ull;
  h = mix64(h ^ b.bc[0]);
  h = mix64(h ^ b.bc[1]);
#pragma unroll
  for (int t = PAWN; t <= KING; ++t) h = mix64(h ^ b.bt[t]);
  h = mix64(h ^ ((uint64_t)b.cr | (uint64_t)(b.stm & 1u) << 32 | (uint64_t)(uint32_t)(ep + 1) << 40));
  return h & mask;
}

// b's identity against x's (xep: x's counted en-passant square).
__device__ __forceinline__ bool same_identity(const DBoard& x, int32_t xep, const DBoard& b) {
  bool eq = x.bc[0] == b.bc[0] && x.bc[1] == b.bc[1] && x.stm == b.stm && x.cr == b.cr;
#pragma unroll
  for (int t = PAWN; t <= KING; ++t) eq = eq && x.bt[t] == b.bt[t];
  return eq && xep == ident_ep(b);
}

// Was the move between two consecutive boards a pawn move or a capture?
__device__ __forceinline__ bool irreversible_between(const DBoard& before, const DBoard& after) {
  return before.bt[PAWN] != after.bt[PAWN] ||
         __popcll(before.bc[0] | before.bc[1]) != __popcll(after.bc[0] | after.bc[1]);
}

__device__ __forceinline__ uint32_t clock_up(uint32_t c) { return c >= 65535u ? 65535u : c + 1u; }

__global__ void root_clocks_kernel(const char* __restrict__ text, const uint32_t* __restrict__ fen_off,
                                   const uint32_t* __restrict__ mv_off, uint32_t ngames,
                                   uint32_t* __restrict__ clock0) {
  const uint32_t g = blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= ngames) return;
  uint32_t p = fen_off[g], st = 0;
  const uint32_t end = mv_off[g];
  int len = 0;
  for (int field = 0; field < 5; ++field) len = next_token(text, p, end, st);  // 0 once the text has run out
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

__global__ __launch_bounds__(kBlock) void ply_keys_kernel(const DBoard* __restrict__ states, uint32_t n,
                                                          const uint32_t* __restrict__ ply_off, uint32_t ngames,
                                                          uint64_t mask, uint64_t* __restrict__ keys) {
  const uint32_t p = blockIdx.x * kBlock + threadIdx.x;
  if (p >= n) return;
  const DBoard b = states[p];
  uint64_t key = ident_key(b, ident_ep(b), mask);
  if (p > ply_off[game_of(ply_off, ngames, p)] && irreversible_between(states[p - 1], b)) key |= kIrreversible;
  keys[p] = key;
}

__global__ __launch_bounds__(kBlock) void ply_walk_kernel(const DBoard* __restrict__ states, uint32_t n,
                                                          const uint32_t* __restrict__ ply_off, uint32_t ngames,
                                                          const uint32_t* __restrict__ clock0,
                                                          const uint64_t* __restrict__ keys, uint32_t* __restrict__ lo,
                                                          fnnue_ply_history* __restrict__ hist) {
  const uint32_t p = blockIdx.x * kBlock + threadIdx.x;
  if (p >= n) return;
  const uint32_t g = game_of(ply_off, ngames, p), first = ply_off[g];
  uint32_t r = p;  // the window's first ply: the last irreversible move's, or the root
  while (r > first && !(keys[r] & kIrreversible)) --r;
  const uint64_t clock = keys[r] & kIrreversible ? (uint64_t)(p - r) : (uint64_t)clock0[g] + (p - first);
  const uint64_t mine = keys[p] & ~kIrreversible;
  uint32_t seen = 0;
  if (p - r >= 2) {  // the plies of p's own side to move
    const DBoard b = states[p];
    const int32_t ep = ident_ep(b);
    for (uint32_t q = p - 2;; q -= 2) {
      if ((keys[q] & ~kIrreversible) == mine && same_identity(b, ep, states[q])) ++seen;
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

// The move a code names on b (ChessRules::step's reading: the own king onto a
// castling rook's square, or in a standard game onto its two-square destination,
// castles), played on c; irreversible: a pawn move or a capture.
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
  do_move(c, m);
}

// Is the searched position x drawn?  clock: x's; reversible: every move of the
// path from ply P was (else nothing before it can equal x); f: x's end byte.
__device__ __forceinline__ bool drawn(const DBoard& x, uint32_t clock, bool reversible, uint32_t f,
                                      const DBoard* __restrict__ states, const uint64_t* __restrict__ keys,
                                      uint64_t mask, uint32_t r, uint32_t P) {
  if ((f & kFinalWon) || ((f & kFinalNoMoves) && (f & (kFinalCheck | kFinalExtinct | kFinalVariant)))) return false;
  if (clock >= 100) return true;
  if (!reversible) return false;
  const int32_t ep = ident_ep(x);
  const uint64_t key = ident_key(x, ep, mask);
  uint32_t seen = 0;
  for (uint32_t q = P;; --q) {  // the other side's plies never match: the side to move is part of the key's input
    if ((keys[q] & ~kIrreversible) == key && same_identity(x, ep, states[q]) && ++seen >= 2) return true;
    if (q == r) break;
  }
  return false;
}

__global__ __launch_bounds__(kBlock) void mark_level1_kernel(
    const uint32_t* __restrict__ list, const fnnue_ply_history* __restrict__ hist, const uint64_t* __restrict__ keys,
    const uint32_t* __restrict__ lo, uint64_t mask, const DBoard* __restrict__ states, uint32_t n,
    const uint32_t* __restrict__ off, const uint16_t* __restrict__ moves, uint8_t* __restrict__ end) {
  const uint32_t count = list[0] < n ? list[0] : n;
  for (uint32_t i = blockIdx.x; i < count; i += gridDim.x) {
    const uint32_t P = list[1 + i];
    if (P >= n) continue;
    const uint32_t o = off[P], e = off[P + 1];
    if (e - o < 2 || e < o) continue;
    const DBoard b = states[P];
    const uint32_t clock = hist[P].clock, r = lo[P];
    for (uint32_t c = 1 + threadIdx.x; c < e - o; c += kBlock) {
      DBoard x;
      bool irr;
      apply_code(b, moves[o + c], x, irr);
      const uint32_t f = end[o + c];
      if (drawn(x, irr ? 0u : clock_up(clock), !irr, f, states, keys, mask, r, P)) end[o + c] = (uint8_t)(f | kFinalDraw);
    }
  }
}

__global__ __launch_bounds__(kBlock) void mark_level2_kernel(
    const uint32_t* __restrict__ list, const fnnue_ply_history* __restrict__ hist, const uint64_t* __restrict__ keys,
    const uint32_t* __restrict__ lo, uint64_t mask, const DBoard* __restrict__ states, uint32_t p0, uint32_t p1,
    const uint32_t* __restrict__ off, const DBoard* __restrict__ kid_states, const uint32_t* __restrict__ kid_off,
    uint32_t rec0, const uint16_t* __restrict__ gmoves, uint8_t* __restrict__ gend) {
  const uint32_t count = list[0];
  for (uint32_t i = blockIdx.x; i < count; i += gridDim.x) {
    const uint32_t P = list[1 + i];
    if (P < p0 || P >= p1) continue;
    const uint32_t d0 = off[P] - P, d1 = off[P + 1] - (P + 1);  // the ply's children in the dense array
    if (d1 <= d0) continue;
    const DBoard b = states[P];
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
      const DBoard c = kid_states[dl];
      const bool irr1 = irreversible_between(b, c);
      const uint32_t cclock = irr1 ? 0u : clock_up(clock);
      DBoard x;
      bool irr2;
      apply_code(c, gmoves[rr - rec0], x, irr2);
      const uint32_t f = gend[rr - rec0];
      if (drawn(x, irr2 ? 0u : clock_up(cclock), !irr1 && !irr2, f, states, keys, mask, r, P))
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

}  // namespace

uint32_t draw_key_bits() {
  const char* e = std::getenv("FNNUE_DRAW_KEY_BITS");
  if (!e || !*e) return 63;
  const long v = std::atol(e);
  return v < 1 ? 1u : v > 63 ? 63u : (uint32_t)v;
}

hipError_t game_history_device(const char* d_text, const uint32_t* d_fen_off, const uint32_t* d_mv_off,
                               const uint32_t* d_ply_off, uint32_t ngames, const DBoard* d_states, uint32_t n,
                               uint32_t key_bits, hipStream_t s, BuilderScratch& ws, DrawHistory* out) {
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
  hipLaunchKernelGGL(root_clocks_kernel, dim3((ngames + 63) / 64), dim3(64), 0, s, d_text, d_fen_off, d_mv_off, ngames,
                     clock0);
  hipLaunchKernelGGL(ply_keys_kernel, per_ply, dim3(kBlock), 0, s, d_states, n, d_ply_off, ngames, mask, keys);
  hipLaunchKernelGGL(ply_walk_kernel, per_ply, dim3(kBlock), 0, s, d_states, n, d_ply_off, ngames, clock0, keys, lo,
                     hist);
  hipLaunchKernelGGL(ply_list_kernel, per_ply, dim3(kBlock), 0, s, n, lo, hist, list);
  return hipGetLastError();
}

hipError_t mark_draws_level1(const DrawHistory& h, const DBoard* d_states, uint32_t n, const uint32_t* d_off,
                             const uint16_t* d_moves, uint8_t* d_end, hipStream_t s) {
  if (n == 0) return hipSuccess;
  hipLaunchKernelGGL(mark_level1_kernel, dim3(std::min(n, kMarkBlocks)), dim3(kBlock), 0, s, h.list, h.hist, h.keys, h.lo,
                     key_mask(h.key_bits), d_states, n, d_off, d_moves, d_end);
  return hipGetLastError();
}

hipError_t mark_draws_level2(const DrawHistory& h, const DBoard* d_states, uint32_t p0, uint32_t p1,
                             const uint32_t* d_off, const DBoard* d_kid_states, const uint32_t* d_kid_off,
                             uint32_t rec0, const uint16_t* d_gmoves, uint8_t* d_gend, hipStream_t s) {
  if (p1 <= p0) return hipSuccess;
  hipLaunchKernelGGL(mark_level2_kernel, dim3(std::min(p1 - p0, kMarkBlocks)), dim3(kBlock), 0, s, h.list, h.hist, h.keys,
                     h.lo, key_mask(h.key_bits), d_states, p0, p1, d_off, d_kid_states, d_kid_off, rec0, d_gmoves,
                     d_gend);
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
