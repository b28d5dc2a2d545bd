// draws_host.cpp — fnnue_game_history on the host (include/fnnue.h, ABI 3.12):
// the clock and the identity count of every ply by the host replay (board.h),
// the record the device history (draws.hip) is held to.
#include <algorithm>
#include <string>
#include <vector>

#include "board.h"
#include "internal.h"

using namespace fnnue;
using fnnue::detail::fail;

namespace {

bool space(char c) { return c == ' ' || c == '\t' || c == '\n' || c == '\r'; }

std::vector<std::string> tokens(const char* p, const char* end) {
  std::vector<std::string> out;
  while (p < end) {
    while (p < end && space(*p)) ++p;
    const char* q = p;
    while (q < end && !space(*q)) ++q;
    if (q > p) out.emplace_back(p, q);
    p = q;
  }
  return out;
}

// The FEN's fifth field when it is an unsigned decimal number (saturating), else 0.
uint32_t root_clock(const std::vector<std::string>& fen) {
  if (fen.size() < 5 || fen[4].empty()) return 0;
  uint32_t v = 0;
  for (char ch : fen[4]) {
    if (ch < '0' || ch > '9') return 0;
    v = std::min<uint32_t>(v * 10u + (uint32_t)(ch - '0'), 65535u);
  }
  return v;
}

}  // namespace

extern "C" int fnnue_game_history(const char* text, size_t text_len, const uint32_t* fen_off,
                                  const uint32_t* moves_off, size_t ngames, fnnue_ply_history* out, size_t cap,
                                  uint32_t* off, size_t off_cap, size_t* n_out, size_t* n_groups) {
  if (!n_out || !n_groups || (ngames && (!text || !fen_off || !moves_off))) return fail(FNNUE_E_ARG, "null argument");
  *n_out = *n_groups = 0;
  if (ngames == 0) return FNNUE_OK;
  if (fen_off[ngames] > text_len) return fail(FNNUE_E_ARG, "offsets exceed the text");
  for (size_t g = 0; g < ngames; ++g)
    if (fen_off[g] > moves_off[g] || moves_off[g] > fen_off[g + 1]) return fail(FNNUE_E_ARG, "offsets out of order");
  std::vector<std::vector<std::string>> moves(ngames);
  size_t plies = 0;
  for (size_t g = 0; g < ngames; ++g) {
    moves[g] = tokens(text + moves_off[g], text + fen_off[g + 1]);
    plies += moves[g].size() + 1;
  }
  *n_out = plies;
  *n_groups = ngames;
  if (!out || !off || cap < plies || off_cap < ngames + 1) return fail(FNNUE_E_CAPACITY, "output buffer too small");
  size_t p = 0;
  std::vector<BoardIdentity> ids;
  std::vector<uint32_t> clocks;
  for (size_t g = 0; g < ngames; ++g) {
    const std::string fen(text + fen_off[g], text + moves_off[g]);
    Board b;
    std::string err;
    if (!board_from_fen(fen.c_str(), b, &err))
      return fail(FNNUE_E_FEN, "unparsable FEN in game " + std::to_string(g) + ": " + err);
    b.halfmove = (int)root_clock(tokens(fen.data(), fen.data() + fen.size()));
    ids.clear();
    off[g] = (uint32_t)p;
    for (size_t i = 0; i <= moves[g].size(); ++i) {
      if (i) {
        Move m;
        if (!parse_uci(b, moves[g][i - 1].c_str(), m))
          return fail(FNNUE_E_MOVE, "illegal move at ply " + std::to_string(i) + " of game " + std::to_string(g));
        b.do_move(m);  // halfmove: 0 after a pawn move or a capture, else one more
      }
      ids.push_back(b.identity());
      size_t seen = 0;
      for (size_t q = 0; q < i; ++q) seen += ids[q] == ids[i] ? 1 : 0;
      out[p].clock = (uint16_t)std::min(b.halfmove, 65535);
      out[p].seen = (uint8_t)std::min<size_t>(seen, 255);
      out[p].reserved = 0;
      ++p;
    }
  }
  off[ngames] = (uint32_t)p;
  return FNNUE_OK;
}
