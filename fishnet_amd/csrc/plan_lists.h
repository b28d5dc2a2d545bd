// plan_lists.h — both feature lists of a position from one walk over its board
// (plan_scatter_kernel, ft_sliced.hip; DESIGN §4.2 "Plan lists").  Plain
// integer code shared by the kernel and the host test
// (tests/plan_lists_host.cpp): no HIP types, only compiler builtins that gcc
// and clang both have.  On the device the staging row is the lane's LDS row,
// on the host a plain array.
#pragma once
#include <stdint.h>

#ifdef __HIPCC__
#define FNNUE_HD __host__ __device__
#define FNNUE_HD_INLINE __host__ __device__ __forceinline__
#define FNNUE_UNROLL _Pragma("unroll")
#else
#define FNNUE_HD
#define FNNUE_HD_INLINE inline
#define FNNUE_UNROLL
#endif

namespace fnnue {

constexpr uint32_t kListRows = 704;                 // rows per king block (sliced_common.h: kRowsPerBlock)
constexpr uint32_t kListNoEntry = 16 * kListRows;   // the zero row's entry (sliced_common.h: kNoEntry)
constexpr int kListWalked = 30;                     // pieces other than the two kings, at most

// Plane of piece code pc (0..15) seen by white, one nibble per pc:
// 2 * (type - 1) + (colour is black); the kings never reach the table (upstream
// half_ka_v2_hm.h PieceSquareIndex / 64).  Black sees a non-king's plane ^ 1.
FNNUE_HD constexpr uint64_t white_plane_table() {
  uint64_t t = 0;
  for (int pc = 1; pc < 16; ++pc) {
    const int type = pc & 7;
    if (type < 1 || type > 5) continue;
    t |= (uint64_t)(2 * (type - 1) + (pc >> 3)) << (4 * pc);
  }
  return t;
}

struct alignas(16) ListQuad {  // 16 bytes of a list, stored at once
  uint32_t x, y, z, w;
} __attribute__((__may_alias__));

// Writes the 32-entry feature lists of one position's two items: item `itw`
// (white's perspective, own king on wk) and item `itb` (black's, own king on
// bk).  Contract of a list, as ft_slices reads it: 32 u16 entries 16 * row,
// row = the feature's row in the item's king block (oriented square + 64 *
// plane), laid out as
//   first   the entries whose row parity equals pp,
//   then    the entries of the other parity,
//   then    kListNoEntry up to entry 31,
// where pp = (item - first item of its king block) & 1 (ppw, ppb).  The own
// king is left out (its row joins the bias), the other king is listed (plane
// 10).  The order inside a parity run is free.  ft_slices pairs the items 2k
// and 2k + 1 of a pass on one ds_read_b128 lane group and a 128-B tile row r
// lies in bank half r & 1, so the pair mostly reads opposite bank halves.
//
// w = the packed board (word i = squares 8i .. 8i + 7, one nibble each), occ
// its occupancy.  `mine` = 16 words of staging (the lane's row), flist 16-byte
// aligned.
//
// The lanes of a wave move in lockstep, so a divergent loop runs as often as
// its busiest lane.  Walking rank by rank, once per perspective, cost 2 x 55
// steps on the benchmark's positions (22 pieces on average); here the board is
// walked once, per 32-square half (34 steps), without the kings: what a piece
// contributes to either list then differs only by constants of the lane.  With
//   val = square | white's plane << 6
// white lists t = val ^ fx0, black t = val ^ fx1, entry t << 4, row parity
// t & 1:  fx0 = (wk on files a-d ? 7 : 0),  fx1 = 56 ^ (bk on a-d ? 7 : 0) ^ 64
// (rank flip, file mirror, plane ^ 1).  The walk stores val at its walk index;
// the row is read back as words with static indices, and each perspective
// partitions it into its two runs in straight-line code, one u16 store per
// piece (the loop over k is unrolled; `k >= n` ends it for the whole wave at
// the wave's longest list).
struct ListWalk {
  uint32_t v[kListWalked / 2];  // val of the walked pieces, two per word, in walk order
  uint64_t pcs;                 // their squares
  uint32_t n;                   // their count
};

// The walk: needs the board alone, not the items' places in the plan, so
// plan_scatter runs it while its range reservations are in flight.
FNNUE_HD_INLINE ListWalk walk_board(const uint32_t (&w)[8], uint64_t occ, int wk, int bk, uint32_t* __restrict__ mine) {
  // the row is written as u16 and as words: may_alias types keep the compiler
  // from reordering (or dropping) one kind against the other
  typedef uint16_t u16_alias __attribute__((__may_alias__));
  typedef uint32_t u32_alias __attribute__((__may_alias__));
  u32_alias* M = reinterpret_cast<u32_alias*>(mine);
  u16_alias* L = reinterpret_cast<u16_alias*>(mine);
  constexpr uint64_t ptab = white_plane_table();
  ListWalk r;
  const uint64_t pcs = occ & ~(1ull << wk) & ~(1ull << bk);
  r.pcs = pcs;
  r.n = (uint32_t)__builtin_popcount((uint32_t)pcs) + (uint32_t)__builtin_popcount((uint32_t)(pcs >> 32));
  uint32_t at = 0;
FNNUE_UNROLL
  for (int h = 0; h < 2; ++h) {
    uint32_t m = (uint32_t)(pcs >> (32 * h));
    const uint32_t wa = w[4 * h], wb = w[4 * h + 1], wc = w[4 * h + 2], wd = w[4 * h + 3];
    while (m) {
      const uint32_t j = (uint32_t)__builtin_ctz(m);
      m &= m - 1;
      const uint32_t lo = (j & 8u) ? wb : wa, hi = (j & 8u) ? wd : wc;
      const uint32_t nib = (((j & 16u) ? hi : lo) >> ((j & 7u) << 2)) & 15u;
      const uint32_t plane = (uint32_t)(ptab >> (nib << 2)) & 15u;
      L[at++] = (uint16_t)((32u * h + j) | plane << 6);
    }
  }
FNNUE_UNROLL
  for (int j = 0; j < kListWalked / 2; ++j) r.v[j] = M[j];
  return r;
}

// The two partitions: the lists of items itw / itb from the walked row.
FNNUE_HD_INLINE void emit_list_pair(const ListWalk& r, int wk, int bk, uint32_t itw, uint32_t ppw, uint32_t itb,
                                    uint32_t ppb, uint32_t* __restrict__ mine, uint16_t* __restrict__ flist) {
  typedef uint16_t u16_alias __attribute__((__may_alias__));
  typedef uint32_t u32_alias __attribute__((__may_alias__));
  u32_alias* M = reinterpret_cast<u32_alias*>(mine);
  u16_alias* L = reinterpret_cast<u16_alias*>(mine);
  constexpr uint64_t kEvenFiles = 0x5555555555555555ull;
  const uint64_t pcs = r.pcs;
  const uint32_t n = r.n;
  const uint32_t m0 = (wk & 7) < 4 ? 7u : 0u, m1 = (bk & 7) < 4 ? 7u : 0u;
  auto emit = [&](uint32_t fx, uint32_t king_t, int king_sq, uint32_t mirror, uint32_t pp, uint32_t it) {
FNNUE_UNROLL
    for (int j = 0; j < 16; ++j) M[j] = kListNoEntry | kListNoEntry << 16;
    // length of the first run: the listed pieces on files of the parity that
    // orients to pp
    const uint64_t first_files = (pp ^ (mirror & 1u)) ? ~kEvenFiles : kEvenFiles;
    const uint64_t firsts = (pcs | 1ull << king_sq) & first_files;
    // running ends of the two runs; s = 1: the piece goes to the second run
    u16_alias* pf = L;
    u16_alias* ps = L + (uint32_t)__builtin_popcount((uint32_t)firsts) + (uint32_t)__builtin_popcount((uint32_t)(firsts >> 32));
    auto put = [&](uint32_t e, uint32_t s) {  // the low 16 bits of e are the entry
      *(s ? ps : pf) = (uint16_t)e;
      ps += s;
      pf += 1u - s;
    };
    put(king_t << 4, (king_t ^ pp) & 1u);
    const uint32_t fx2 = fx | fx << 16, pp2 = pp | pp << 16;
FNNUE_UNROLL
    for (int k = 0; k < kListWalked; ++k) {
      if ((uint32_t)k >= n) break;
      const uint32_t t2 = r.v[k >> 1] ^ fx2;  // two pieces per word: val < 2^10, so t2 << 4 is both entries
      const uint32_t e2 = t2 << 4, s2 = (t2 ^ pp2) & 0x00010001u;
      put((k & 1) ? e2 >> 16 : e2, (k & 1) ? s2 >> 16 : s2 & 1u);
    }
    ListQuad* dst = static_cast<ListQuad*>(__builtin_assume_aligned(flist + (size_t)it * 32, 16));
FNNUE_UNROLL
    for (int q = 0; q < 4; ++q) dst[q] = ListQuad{M[4 * q], M[4 * q + 1], M[4 * q + 2], M[4 * q + 3]};
  };
  const uint32_t fx0 = m0, fx1 = 56u ^ m1 ^ 64u;
  emit(fx0, ((uint32_t)bk | 10u << 6) ^ fx0, bk, m0, ppw, itw);          // white's list: the black king
  emit(fx1, ((uint32_t)wk | 10u << 6) ^ fx1 ^ 64u, wk, m1, ppb, itb);   // black's list: the white king, plane 10
}

FNNUE_HD_INLINE void build_list_pair(const uint32_t (&w)[8], uint64_t occ, int wk, int bk, uint32_t itw, uint32_t ppw,
                                     uint32_t itb, uint32_t ppb, uint32_t* __restrict__ mine,
                                     uint16_t* __restrict__ flist) {
  emit_list_pair(walk_board(w, occ, wk, bk, mine), wk, bk, itw, ppw, itb, ppb, mine, flist);
}

}  // namespace fnnue
