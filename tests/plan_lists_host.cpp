// Host check of build_list_pair (fishnet_amd/csrc/plan_lists.h): both feature
// lists of a position, built from one walk over its board, against a naive
// per-square reference written here.  Built with ASan + UBSan and run by
// tests/test_plan_lists.py.
//
// For each board, each perspective and each item parity pp it checks the list
// contract: the multiset of entries is the reference's; the first run holds
// the entries whose row parity is pp and has the reference's length; the second
// run holds the others; kListNoEntry pads through entry 31; nothing is written
// outside the 16 staging words and the two 64-byte lists.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "plan_lists.h"

namespace {

constexpr int kWhiteKing = 6, kBlackKing = 14;
constexpr uint32_t kStageGuard = 0xDEADBEEFu;
constexpr uint16_t kListGuard = 0xA5A5u;

struct Board {
  int pc[64];  // piece code per square: type 1..6 (6 = king) | 8 for black, 0 = empty
};

uint64_t rng_state = 0x9E3779B97F4A7C15ull;
uint32_t rnd() {
  rng_state ^= rng_state << 13;
  rng_state ^= rng_state >> 7;
  rng_state ^= rng_state << 17;
  return (uint32_t)(rng_state >> 32);
}

// The contract, square by square: the entries 16 * row of perspective p (own
// king left out), row = oriented square + 64 * plane, plane = 2 * (type - 1) +
// (the piece is the other side's), kings plane 10; the square is flipped
// vertically for black and mirrored when the own king stands on files a-d.
std::vector<uint16_t> reference(const Board& b, int p) {
  int own = -1;
  for (int s = 0; s < 64; ++s)
    if (b.pc[s] == (p ? kBlackKing : kWhiteKing)) own = s;
  const int flip = (p ? 56 : 0) ^ ((own & 7) < 4 ? 7 : 0);
  std::vector<uint16_t> out;
  for (int s = 0; s < 64; ++s) {
    const int pc = b.pc[s];
    if (!pc || s == own) continue;
    const int type = pc & 7, colour = pc >> 3;
    const int plane = type == 6 ? 10 : 2 * (type - 1) + (colour != p ? 1 : 0);
    out.push_back((uint16_t)(16 * ((s ^ flip) + 64 * plane)));
  }
  return out;
}

long boards_checked = 0;

bool fail(const Board& b, const char* what, int p, uint32_t pp) {
  std::printf("error: %s (perspective %d, pp %u), board:", what, p, pp);
  for (int s = 0; s < 64; ++s) std::printf(" %d", b.pc[s]);
  std::printf("\n");
  return false;
}

bool check_board(const Board& b) {
  uint32_t w[8] = {0};
  uint64_t occ = 0;
  int wk = -1, bk = -1;
  for (int s = 0; s < 64; ++s) {
    w[s >> 3] |= (uint32_t)b.pc[s] << (4 * (s & 7));
    if (b.pc[s]) occ |= 1ull << s;
    if (b.pc[s] == kWhiteKing) wk = s;
    if (b.pc[s] == kBlackKing) bk = s;
  }
  const std::vector<uint16_t> ref[2] = {reference(b, 0), reference(b, 1)};
  for (uint32_t pps = 0; pps < 4; ++pps) {
    const uint32_t pp[2] = {pps & 1u, pps >> 1};
    // staging: one guard word, the 17-word row of a lane, one guard word
    uint32_t stage[19];
    for (uint32_t& x : stage) x = kStageGuard;
    for (int j = 1; j <= 16; ++j) stage[j] = rnd();  // what an earlier position left behind
    // five lists of 32 entries; items 1 and 3 are written (in either order)
    alignas(64) uint16_t flist[5 * 32];
    for (uint16_t& x : flist) x = kListGuard;
    const uint32_t it[2] = {pps == 1 ? 3u : 1u, pps == 1 ? 1u : 3u};
    fnnue::build_list_pair(w, occ, wk, bk, it[0], pp[0], it[1], pp[1], stage + 1, flist);
    if (stage[0] != kStageGuard || stage[17] != kStageGuard || stage[18] != kStageGuard)
      return fail(b, "write outside the staging row", 0, pps);
    for (int i = 0; i < 5 * 32; ++i)
      if ((uint32_t)(i / 32) != it[0] && (uint32_t)(i / 32) != it[1] && flist[i] != kListGuard)
        return fail(b, "write outside the two lists", 0, pps);
    for (int p = 0; p < 2; ++p) {
      const uint16_t* l = flist + 32 * it[p];
      const std::vector<uint16_t>& r = ref[p];
      const size_t n = r.size();
      if (n < 1 || n > 31) return fail(b, "reference length", p, pp[p]);
      size_t nf = 0;
      for (uint16_t e : r) nf += ((e >> 4) & 1u) == pp[p];
      for (size_t k = n; k < 32; ++k)
        if (l[k] != fnnue::kListNoEntry) return fail(b, "padding", p, pp[p]);
      std::vector<uint16_t> got(l, l + n), want(r);
      std::sort(got.begin(), got.end());
      std::sort(want.begin(), want.end());
      if (got != want) return fail(b, "entries differ from the reference", p, pp[p]);
      for (size_t k = 0; k < n; ++k)
        if ((((l[k] >> 4) & 1u) == pp[p]) != (k < nf)) return fail(b, "parity runs", p, pp[p]);
    }
  }
  ++boards_checked;
  return true;
}

Board empty_board() {
  Board b;
  std::memset(&b, 0, sizeof b);
  return b;
}

// A non-king piece code: type 1..5, either colour.
int some_piece() { return 1 + (int)(rnd() % 5) + 8 * (int)(rnd() & 1); }

// Kings on wk / bk and `extra` other pieces on squares drawn from `allowed`.
bool placed(int wk, int bk, int extra, uint64_t allowed) {
  Board b = empty_board();
  b.pc[wk] = kWhiteKing;
  b.pc[bk] = kBlackKing;
  allowed &= ~(1ull << wk) & ~(1ull << bk);
  std::vector<int> sq;
  for (int s = 0; s < 64; ++s)
    if (allowed >> s & 1) sq.push_back(s);
  for (size_t i = sq.size(); i > 1; --i) std::swap(sq[i - 1], sq[rnd() % i]);
  for (int i = 0; i < extra && i < (int)sq.size(); ++i) b.pc[sq[i]] = some_piece();
  return check_board(b);
}

}  // namespace

int main() {
  constexpr uint64_t kAll = ~0ull, kEvenFiles = 0x5555555555555555ull, kLower = 0xFFFFFFFFull;
  // king squares: files a-d and e-h, in the lower and the upper half board
  const int kings[] = {0, 2, 3, 4, 7, 9, 27, 28, 31, 32, 35, 36, 58, 60, 61, 63};
  bool ok = true;
  for (int wk : kings)
    for (int bk : kings) {
      if (wk == bk) continue;
      ok = ok && placed(wk, bk, 0, kAll);             // two bare kings: one entry
      ok = ok && placed(wk, bk, 30, kAll);            // 32 pieces: 31 entries, no padding
      ok = ok && placed(wk, bk, 1, kAll);
      ok = ok && placed(wk, bk, 13, kEvenFiles);      // one parity run empty (the other king aside)
      ok = ok && placed(wk, bk, 13, ~kEvenFiles);
      ok = ok && placed(wk, bk, 30, kEvenFiles);
      ok = ok && placed(wk, bk, 30, ~kEvenFiles);
      ok = ok && placed(wk, bk, 12, kLower);          // the walk's first loop only
      ok = ok && placed(wk, bk, 12, ~kLower);         // the second only
      ok = ok && placed(wk, bk, 30, kLower);
      ok = ok && placed(wk, bk, 30, ~kLower);
    }
  // every pair of king squares once, a few pieces
  for (int wk = 0; wk < 64 && ok; ++wk)
    for (int bk = 0; bk < 64 && ok; ++bk)
      if (wk != bk) ok = placed(wk, bk, (int)(rnd() % 31), kAll);
  // random placements of 2 to 32 pieces
  for (int i = 0; i < 6000 && ok; ++i) {
    const int wk = (int)(rnd() % 64);
    int bk = (int)(rnd() % 63);
    bk += bk >= wk;
    ok = placed(wk, bk, (int)(rnd() % 31), kAll);
  }
  if (!ok) return 1;
  std::printf("plan lists ok: %ld boards\n", boards_checked);
  return 0;
}
