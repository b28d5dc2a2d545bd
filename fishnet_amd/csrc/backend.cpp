// backend.cpp — fnnue_backend (include/fnnue_backend.h): fishnet's engine
// actor shape over the evaluator.  The reference's pair
//   stockfish::channel -> (StockfishStub, StockfishActor)   [ref] src/stockfish.rs:23-61
// is a bounded mpsc channel (capacity 1) into an actor owning one engine
// process; StockfishStub::go sends a Position with a oneshot callback and
// maps any failure to PositionFailed{batch_id}.  Here the actor owns one
// fnnue_ctx per net (chess, and optionally the crazyhouse and atomic variant
// nets) and answers one message at a time on the caller's thread (a second
// caller waits: the capacity-1 channel); a message carries whole acquired batches
// (AcquireResponseBody, [ref] src/api.rs:293-309), expanded the way
// IncomingBatch::from_acquired does ([ref] src/queue.rs:518-627) — but on the
// device: the FEN/UCI text goes to HBM once, the builder replays every game
// there and the plies are evaluated incrementally along each game.
//
// One go(), per net: the host counts each batch's plies (it must: the
// response offsets are part of the answer) and cuts the games into pieces;
// per piece it stages the text, offsets (and, in the last piece, the
// move-work children) in a pinned image and sends it with one copy; the
// context's stream runs the replay (one wave per game), the CHAIN evaluation
// and the children's evaluation, and one copy brings back the builder's error
// word, the game-end flags and every (psqt, positional).  The nets' streams
// run side by side, and the host stages the next pieces and writes a piece's
// responses while the device works on the later ones.  Buffers are grow-only
// (device and pinned host), so a steady stream of calls allocates nothing.  A
// failed batch costs a second pass for its piece only.  Large calls spread the
// host work (text staging, response fill) over a few threads.
//
// Analysis at depth 1 (fnnue_backend_set_analysis_depth; chess nets): a piece's
// replay also keeps the plies' boards, and instead of the CHAIN evaluation the
// stream runs the children expansion with moves and end flags, their STAR
// evaluation and the per-group reduction (stage_search); the piece brings back
// one fnnue_best per ply, from which fill() writes best move, score, depth 1.
//
// The variant nets at depth 1 (fnnue_backend_set_variant_analysis_depth):
// the same staging over the variant's boards (vbuilder.hip: VBoard, or DBoard
// for kingofthehill / racingkings), children with variant move codes (drops)
// and the variant's end flags, fnnue_eval_vgroups_device's STAR evaluation and
// the same reduction, whose ranks know the variant flags.
//
// Analysis at two plies (fnnue_backend_set_analysis_plies(b, 2) for the chess
// nets, fnnue_backend_set_variant_analysis_plies(b, 2) for the variant nets,
// over their boards, rules and ranks: vchild_states_device, launch_vbest_replies):
// stage_search goes on behind the children's evaluation: the children's boards
// as a dense array (child_states_device), their own children counted (a second
// sizing read-back), expanded, evaluated as STAR groups and reduced to one
// fnnue_best per child, then the second reduction (fnnue_best_replies_device's)
// into one fnnue_best2 per ply; fill() writes score, depth = the pv's length,
// best move, and the reply beside the responses (fnnue_backend_go_pv).
//
// MultiPV (fnnue_backend_go_lines, a depth-1 channel): a piece with a batch
// that asked for k lines carries every ply's slot offsets up (after ply_off)
// and one more kernel, fnnue_topk_children_device's, ranks the children that
// are on the device anyway into a `lines` section behind the fnnue_best
// records; fill() converts each ply's first min(k, nodes) lines.  go() and
// go_compact() stage no slots and launch exactly what they did before.
//
// MultiPV at two plies (fnnue_backend_go_lines_pv): the call searches at the
// channel's own plies; a two-plies piece with slots launches
// fnnue_topk_replies_device's kernel beside the second reduction instead, over
// the same end bytes, moves and children's records, and its `lines` section
// holds fnnue_line2 records (move, reply); a one-ply piece ranks as go_lines.
#include "../../include/fnnue_backend.h"

#include <algorithm>
#include <atomic>
#include <chrono>
#include <climits>
#include <condition_variable>
#include <cstdio>
#include <cstdlib>
#include <cstddef>
#include <cstring>
#include <functional>
#include <mutex>
#include <string>
#include <thread>
#include <emmintrin.h>
#include <sched.h>
#include <vector>

#include "board.h"
#include "builder.h"
#include "internal.h"
#include "search_steps.h"
#include "text_scan.h"
#include "vboard.h"
#include "workers.h"

using namespace fnnue;
using namespace fnnue::detail;

namespace {

constexpr int32_t kNormalizeToPawnSf151 = 361;  // upstream uci.h NormalizeToPawnValue (SF 15.1, recalled)
constexpr int kKinds = kVariants;               // net slots: one per variant id (net.h kVariant*)
constexpr uint32_t kDefaultTimeoutMs = 60000;
// Per-batch text bounds: far beyond any lichess batch (a FEN is < 100 bytes;
// the longest possible game, ~5,900 moves, < 64 KB of UCI), so that a piece's
// text fits its 32-bit offsets whatever the caller sends.
constexpr size_t kMaxFenBytes = 4096, kMaxMovesBytes = (size_t)1 << 22;
constexpr size_t kMaxPieceText = (size_t)1 << 30;  // a new piece before a piece's text passes this   // the worker's budget cap, min(60 s, budget) ([ref] src/main.rs:316)
using Clock = std::chrono::steady_clock;

double ms_since(Clock::time_point t) { return std::chrono::duration<double, std::milli>(Clock::now() - t).count(); }

// One message on the channel: StockfishMessage::Go with its answer.
struct Job {
  const fnnue_acquired* batches = nullptr;
  size_t nb = 0;
  fnnue_position_response* out = nullptr;    // the full records, or
  fnnue_position_compact* cout = nullptr;    // the compact form (fnnue_backend_go_compact) with
  fnnue_batch_compact* bout = nullptr;       // its per-batch part
  size_t cap = 0;
  uint32_t* off = nullptr;
  int32_t* rc = nullptr;
  uint32_t timeout_ms = 0;  // the call's budget (0: the channel's)
  // fnnue_backend_go_lines: the MultiPV lines beside `out`, line_off per response
  fnnue_pv_line* lines = nullptr;
  uint32_t* line_off = nullptr;
  fnnue_move* reply = nullptr;  // fnnue_backend_go_pv: the pv's second move beside `out`
  fnnue_pv_line2* lines2 = nullptr;  // fnnue_backend_go_lines_pv: the lines with their whole pv, instead of `lines`
  bool with_lines() const { return lines || lines2; }
  int ret = 0;
  std::string err;  // fnnue_last_error of a failed call
};

// Grow-only device buffer.
struct DevBuf {
  void* p = nullptr;
  size_t bytes = 0;
  int reserve(size_t want) {
    if (want <= bytes) return FNNUE_OK;
    if (p) (void)hipFree(p);
    p = nullptr;
    bytes = 0;
    want = want + want / 4 + 256;
    if (hipMalloc(&p, want) != hipSuccess) return fail(FNNUE_E_OOM, "backend device buffer");
    bytes = want;
    return FNNUE_OK;
  }
  void release() {
    if (p) (void)hipFree(p);
    p = nullptr;
    bytes = 0;
  }
  template <class T>
  T* at(size_t off) const {
    return reinterpret_cast<T*>(static_cast<char*>(p) + off);
  }
};
// b with at least `bytes`, *out its start.
template <class T>
int reserve(DevBuf& b, size_t bytes, T** out) {
  const int rc = b.reserve(bytes);
  *out = static_cast<T*>(b.p);
  return rc;
}

// Grow-only pinned host buffer (the DMA engines read / write it directly, so
// the copies are asynchronous and need no staging through pageable memory).
struct PinnedBuf {
  void* p = nullptr;
  size_t bytes = 0;
  int reserve(size_t want) {
    if (want <= bytes) return FNNUE_OK;
    if (p) (void)hipHostFree(p);
    p = nullptr;
    bytes = 0;
    want = want + want / 4 + 4096;
    if (hipHostMalloc(&p, want, hipHostMallocDefault) != hipSuccess) return fail(FNNUE_E_OOM, "backend pinned buffer");
    bytes = want;
    return FNNUE_OK;
  }
  void release() {
    if (p) (void)hipHostFree(p);
    p = nullptr;
    bytes = 0;
  }
  template <class T>
  T* at(size_t off) const {
    return reinterpret_cast<T*>(static_cast<char*>(p) + off);
  }
};

size_t count_moves(const char* s) {
  size_t len = 0;
  return s ? scan_tokens(s, &len) : 0;
}

// A position without a legal move with one of these is lost (`mate 0`), else drawn (`cp 0`).
constexpr uint8_t kFinalDecided = kFinalCheck | kFinalExtinct | kFinalVariant;

// A root with no legal move: the engine prints `info depth 0 score mate 0`
// (checkmated; atomic: its king exploded; kingofthehill / racingkings: lost
// by the variant's rule) or `score cp 0` (stalemate, a racingkings draw) and
// `bestmove (none)` ([ref] src/stockfish.rs:359-376, 418-425: Score::Mate(0)
// / Score::Cp(0), best_move None, nodes 0).
void terminal_response(fnnue_position_response& r, uint8_t fin) {
  r.score_kind = (fin & kFinalDecided) ? FNNUE_SCORE_MATE : FNNUE_SCORE_CP;
  r.score = 0;
  r.depth = 0;
  r.nodes = 0;
  r.best_move[0] = 0;
}

size_t align16(size_t x) { return (x + 15) & ~(size_t)15; }

// A search record's (kind, value) as an answer's (FNNUE_SCORE_*, score), for a
// piece answered in units of `norm`: a mate in one and its mirror images
// (mated: every move allows a mate in one; lost: every move loses at once) are
// Score::Mate(1) / Mate(-1).  coded: with quiescence checks a FNNUE_BEST_CP
// value beyond the static domain is a coded mate, answered as Score::Mate of
// its moves.  Everything else is centipawns.  One rule for every record: only
// the replies' kernels emit FNNUE_BEST_MATED, so no one-ply answer changes by it;
// fill() answers a depth-0 ply as a FNNUE_BEST_CP record of its own value, no move.
struct Answer { uint8_t kind; int64_t score; };
struct ScoreRule {
  int32_t norm;
  bool coded;
  Answer operator()(uint8_t kind, int64_t value) const {
    if (kind == FNNUE_BEST_MATE) return {FNNUE_SCORE_MATE, 1};
    if (kind == FNNUE_BEST_MATED || kind == FNNUE_BEST_LOST) return {FNNUE_SCORE_MATE, -1};
    const int64_t a = value < 0 ? -value : value;
    if (coded && kind == FNNUE_BEST_CP && a > FNNUE_VALUE_MATE - 64) {
      const int64_t plies = FNNUE_VALUE_MATE - a;
      if (const int64_t moves = value > 0 ? (plies + 1) / 2 : -(plies / 2)) return {FNNUE_SCORE_MATE, moves};
    }
    return {FNNUE_SCORE_CP, value * 100 / norm};
  }
};

// A move code of net k's rules as UCI text (a variant's may be a drop).
void move_uci(int k, fnnue_move m, char* out) {
  (void)(k == kVariantChess ? fnnue_move_uci(m, out) : fnnue_vmove_uci(m, out));
}

// A fnnue_line2, or a fnnue_line with reply "", as the answer's line with its whole pv.
template <class Line>
fnnue_pv_line2 pv_line2(int k, const ScoreRule& rule, const Line& L, const char* reply) {
  char mv[8] = {0};
  move_uci(k, L.move, mv);
  const Answer a = rule(L.kind, L.value);
  fnnue_pv_line2 out{};
  out.score = a.score;
  out.psqt = L.psqt;
  out.positional = L.positional;
  std::snprintf(out.pv, sizeof(out.pv), "%s%s%s", mv, reply[0] ? " " : "", reply);
  out.score_kind = a.kind;
  out.pv_len = reply[0] ? 2 : 1;
  return out;
}

// MultiPV slots per ply of an analysis batch: Some(k) asks for k lines, and a
// ply has at most FNNUE_MAX_CHILDREN legal moves.
uint32_t line_slots(const fnnue_acquired& a) {
  return a.work == FNNUE_WORK_ANALYSIS && a.multipv >= 1 ? (uint32_t)std::min(a.multipv, FNNUE_MAX_CHILDREN) : 0u;
}
static_assert(sizeof(fnnue_pv_line) == 24 && offsetof(fnnue_pv_line, move) == 16 &&
                  offsetof(fnnue_pv_line, score_kind) == 23,
              "fnnue_pv_line layout");
static_assert(sizeof(fnnue_pv_line2) == 32 && offsetof(fnnue_pv_line2, pv) == 16 &&
                  offsetof(fnnue_pv_line2, score_kind) == 30 && offsetof(fnnue_pv_line2, pv_len) == 31,
              "fnnue_pv_line2 layout");

// A full response written in place as four stores — bytes 0-15 (position id,
// the four flag bytes, score), 16-31 (psqt, positional, nodes), 32-47 and
// 48-55 (time, nps, best move: the same for a whole piece of analysis plies)
// — instead of a memset and a store per field: the fill is bound by the
// stores into the caller's buffer.
static_assert(offsetof(fnnue_position_response, skipped) == 4 && offsetof(fnnue_position_response, score) == 8 &&
                  offsetof(fnnue_position_response, psqt) == 16 && offsetof(fnnue_position_response, nodes) == 24 &&
                  offsetof(fnnue_position_response, time_ms) == 32 && offsetof(fnnue_position_response, nps) == 40 &&
                  offsetof(fnnue_position_response, best_move) == 44 && sizeof(fnnue_position_response) == 56,
              "fnnue_position_response layout");
static_assert(sizeof(fnnue_position_compact) == 16 && sizeof(fnnue_batch_compact) == 24, "compact layouts");
struct ResponseTail {  // bytes 32-55 of an analysis response of one piece
  __m128i t32;
  uint64_t t48;
  ResponseTail(uint64_t ms, uint32_t nps) : t32(_mm_set_epi64x((long long)nps, (long long)ms)), t48(0) {}
};
inline uint64_t response_head(uint32_t id, uint8_t skipped, uint8_t kind, uint8_t depth, uint8_t matrix) {
  return id | (uint64_t)skipped << 32 | (uint64_t)kind << 40 | (uint64_t)depth << 48 | (uint64_t)matrix << 56;
}
inline void put_response(fnnue_position_response* r, uint64_t head, int64_t score, int32_t psqt, int32_t positional,
                         uint64_t nodes, const ResponseTail& tail) {
  char* d = reinterpret_cast<char*>(r);
  _mm_storeu_si128(reinterpret_cast<__m128i*>(d), _mm_set_epi64x((long long)score, (long long)head));
  _mm_storeu_si128(reinterpret_cast<__m128i*>(d + 16),
                   _mm_set_epi64x((long long)nodes, (long long)((uint64_t)(uint32_t)psqt | (uint64_t)(uint32_t)positional << 32)));
  _mm_storeu_si128(reinterpret_cast<__m128i*>(d + 32), tail.t32);
  std::memcpy(d + 48, &tail.t48, 8);
}
inline void put_compact(fnnue_position_compact* r, int32_t psqt, int32_t positional, int32_t score, uint8_t kind,
                        uint8_t depth, uint8_t flags) {
  _mm_storeu_si128(reinterpret_cast<__m128i*>(r),
                   _mm_set_epi32((int)((uint32_t)kind | (uint32_t)depth << 8 | (uint32_t)flags << 16), score,
                                 positional, psqt));
}

// The net slot of a batch's variant (shakmaty Variant names, [ref]
// src/api.rs:304; logger.rs:194-201): standard chess (EngineFlavor::Official
// for analysis, queue.rs:530-539) and the five variants with a Fairy-Stockfish
// NNUE feature set here.  -1: a variant this backend does not evaluate
// (antichess, horde: kingless sides, which the king-block feature sets cannot
// express).
int kind_of(const char* v) {
  if (!v || !*v || !std::strcmp(v, "standard") || !std::strcmp(v, "chess960") || !std::strcmp(v, "fromPosition") ||
      !std::strcmp(v, "chess"))
    return kVariantChess;
  if (!std::strcmp(v, "crazyhouse")) return kVariantCrazyhouse;
  if (!std::strcmp(v, "atomic")) return kVariantAtomic;
  if (!std::strcmp(v, "kingOfTheHill")) return kVariantKingOfTheHill;
  if (!std::strcmp(v, "racingKings")) return kVariantRacingKings;
  if (!std::strcmp(v, "threeCheck")) return kVariantThreeCheck;
  return -1;
}

// Host replay of a move batch's root (Work::Move: the position after all
// moves), with its legal children and their game-end flags.
struct MoveRoot {
  uint8_t fin = 0;                 // kFinal* of the root
  std::vector<std::string> uci;    // legal moves
  std::vector<uint8_t> kid_fin;    // kFinal* of each child
};

int chess_move_root(const fnnue_acquired& a, MoveRoot& R, std::vector<fnnue_pos>& kids) {
  Board b;
  std::string e;
  if (!board_from_fen(a.position ? a.position : "", b, &e)) return FNNUE_E_FEN;
  std::string tok;
  for (const char* p = a.moves ? a.moves : "";; ++p) {
    if (*p && *p != ' ' && *p != '\t' && *p != '\n' && *p != '\r') {
      tok += *p;
      continue;
    }
    if (!tok.empty()) {
      Move m;
      if (!parse_uci(b, tok.c_str(), m)) return FNNUE_E_MOVE;
      b.do_move(m);
      tok.clear();
    }
    if (!*p) break;
  }
  auto fin_of = [](const Board& x, bool any) {
    return (uint8_t)((any ? 0 : kFinalNoMoves) | (x.in_check() ? kFinalCheck : 0));
  };
  std::vector<Move> ms;
  b.legal_moves(ms);
  R.fin = fin_of(b, !ms.empty());
  kids.reserve(ms.size());
  for (const Move& m : ms) {
    Board k = b;
    k.do_move(m);
    kids.push_back(k.pack());
    R.uci.push_back(b.uci(m, b.chess960));
    R.kid_fin.push_back(fin_of(k, k.has_legal_move()));
  }
  return FNNUE_OK;
}

int variant_move_root(int variant, const fnnue_acquired& a, MoveRoot& R, std::vector<fnnue_vpos>& kids) {
  vb::VBoard b;
  const char* fen = a.position ? a.position : "";
  if (!vb::parse_fen(fen, 0, (uint32_t)std::strlen(fen), variant, b)) return FNNUE_E_FEN;
  const char* mv = a.moves ? a.moves : "";
  const uint32_t end = (uint32_t)std::strlen(mv);
  uint32_t p = 0, st;
  int len;
  while ((len = vb::next_token(mv, p, end, st)) > 0) {
    vb::VMove m;
    if (!vb::match_uci(b, mv + st, len, m)) return FNNUE_E_MOVE;
    vb::do_move(b, m);
  }
  R.fin = vb::final_state(b);
  vb::for_each_legal(b, [&](const vb::VMove& m) -> bool {
    vb::VBoard k = b;
    vb::do_move(k, m);
    kids.push_back(vb::pack(k));
    R.uci.push_back(vb::vuci(b, m));
    // a child the mover has lost by the variant's rule (racingkings: black
    // did not catch up) is marked, so that it is never chosen as a mate
    R.kid_fin.push_back((uint8_t)(vb::final_state(k) | (vb::variant_over(k) && vb::variant_won(k) ? kFinalWon : 0)));
    return true;
  });
  return FNNUE_OK;
}

// One piece of a net's work: a run of its analysis games (the net's last piece
// also carries the move-work children), staged as one image
//   [text | fen_off | mv_off | ply_off | children | err (16 B) | fin | psqt | positional]
// at its own place in the net's buffers: the first five parts and the zeroed
// error words go up with one copy, the last four come back with one.  err
// words 0-2 are the builder's (code, game, ply), word 3 the evaluator's: the
// context's error word points there while the piece's evaluation is enqueued.
struct Piece {
  std::vector<size_t> games;  // analysis batches (job indices)
  bool kids = false;          // the net's move-work children ride in this piece
  uint32_t ng = 0, n = 0;     // games, plies
  size_t nk = 0;              // children
  size_t o_fen = 0, o_mv = 0, o_ply = 0, o_kids = 0, o_res = 0, o_fin = 0, o_ps = 0, o_po = 0, o_best = 0, end = 0;
  size_t up0 = 0, down0 = 0, dev0 = 0, pos0 = 0;  // where the piece lives in the net's buffers
  // Analysis at depth 1 (chess): the results image ends with one fnnue_best per
  // ply (o_best; psqt / positional then hold each ply's own terms), the plies'
  // boards sit at st0 of the net's board buffer, and `searched` counts the
  // children the piece's search evaluated.
  bool depth1 = false;
  // Two plies: depth1's image with one fnnue_best2 per ply at o_best instead;
  // `searched` counts the children and the grandchildren.
  bool depth2 = false;
  size_t st0 = 0;
  size_t searched = 0;
  // MultiPV (fnnue_backend_go_lines at depth 1): the plies' slot offsets go up
  // at o_loff (n + 1 words: min(multipv, 218) slots for every ply of a batch
  // that asked), and the results image ends with the nslots fnnue_line slots
  // (a two-plies piece of a go_lines_pv(): fnnue_line2 slots).
  size_t nslots = 0, o_loff = 0, o_lines = 0;
  bool pending = false;                           // evaluation enqueued, results not yet read
};

// One net's share of a go(): its analysis games cut into pieces of about
// piece_plies plies, and its move-work roots.  A piece's upload, replay,
// evaluation and download run on the context's stream, one piece after the
// other; the host stages the next pieces and writes a piece's responses while
// the device works on the later ones.  (The replay of the next piece on a
// stream of its own, beside this piece's evaluation, measured slower: its
// waves hold CU slots the evaluation's 1024-thread workgroups need.)
struct NetWork {
  std::vector<size_t> games;      // analysis batches (job indices)
  std::vector<size_t> roots;      // move batches whose roots have legal children
  std::vector<MoveRoot> mroots;   // their replayed roots
  std::vector<size_t> kid_first;  // first child of each root
  std::vector<uint8_t> kids;      // children records
  std::vector<size_t> terminal;   // move batches whose root has no legal move
  std::vector<MoveRoot> troots;
  std::vector<Piece> pieces;
  size_t nk = 0, rec = 0;
  size_t next = 0;                // first piece whose responses are not written yet
  std::vector<hipEvent_t> ev_done;  // per piece: results and error word on the host
  DevBuf dev, pos;
  PinnedBuf up, down, scratch;      // scratch: a failing piece's positions, read back by recover()
  // Analysis at depth 1: every piece's boards, and one piece's children at a
  // time (records, counts and offsets, moves, end flags, psqt, positional; the
  // pieces follow one another on the stream), with the builder's scan scratch.
  DevBuf states, kid_pos, kid_cnt, kid_off, kid_moves, kid_end, kid_ps, kid_po;
  // Two plies: one piece's children as boards, their counts, STAR offsets and
  // depth-1 records, and the grandchildren (records, moves, end flags, terms).
  DevBuf kid_states, kid2_cnt, kid2_off, kid_best, g_pos, g_moves, g_end, g_ps, g_po;
  PinnedBuf sizing;                 // the builder's error word and a piece's record count, read back
  BuilderScratch bscratch;
  void clear() {
    games.clear();
    roots.clear();
    mroots.clear();
    kid_first.clear();
    kids.clear();
    terminal.clear();
    troots.clear();
    pieces.clear();
    nk = 0;
    next = 0;
  }
  int events(size_t n) {
    while (ev_done.size() < n) {
      hipEvent_t e = nullptr;
      if (hipEventCreateWithFlags(&e, hipEventDisableTiming) != hipSuccess) return fail(FNNUE_E_DEVICE, "hipEventCreate");
      ev_done.push_back(e);
    }
    return FNNUE_OK;
  }
  void release() {
    dev.release();
    pos.release();
    up.release();
    down.release();
    scratch.release();
    for (DevBuf* b : {&states, &kid_pos, &kid_cnt, &kid_off, &kid_moves, &kid_end, &kid_ps, &kid_po, &kid_states,
                      &kid2_cnt, &kid2_off, &kid_best, &g_pos, &g_moves, &g_end, &g_ps, &g_po})
      b->release();
    sizing.release();
    bscratch.release();
    for (hipEvent_t e : ev_done) (void)hipEventDestroy(e);
    ev_done.clear();
  }
};

size_t align256(size_t x) { return (x + 255) & ~(size_t)255; }

// CPUs this process may use: its affinity mask, capped by a cgroup v2 CPU
// quota (a container's share of a large host)
int usable_cpus() {
  int n = (int)std::max(1u, std::thread::hardware_concurrency());
  cpu_set_t set;
  if (sched_getaffinity(0, sizeof(set), &set) == 0) n = std::max(1, CPU_COUNT(&set));
  if (FILE* f = std::fopen("/sys/fs/cgroup/cpu.max", "r")) {
    char quota[32] = {0};
    long period = 0;
    if (std::fscanf(f, "%31s %ld", quota, &period) == 2 && std::strcmp(quota, "max") != 0 && period > 0)
      n = std::max(1, std::min(n, (int)((std::atol(quota) + period - 1) / period)));
    std::fclose(f);
  }
  return n;
}

}  // namespace

struct fnnue_backend;
namespace {
// Backends freed while a timed-out call's work was still on their streams
// (fnnue_backend_free): released here once the streams have drained.
std::mutex g_abandoned_mu;
std::vector<fnnue_backend*> g_abandoned;
void reap_abandoned();
}  // namespace

struct fnnue_backend {
  fnnue_ctx* ctx[kKinds] = {};  // one evaluator per net, all on one device
  int device = 0;
  int32_t norm = kNormalizeToPawnSf151;
  // fnnue_backend_set_analysis_depth / _plies: 1 = a one-ply search per chess analysis ply, 2 = two plies
  int analysis_depth = 0;
  int variant_analysis_depth = 0;  // fnnue_backend_set_variant_analysis_depth: the same for the variant nets' plies
  bool draw_rules = false;  // fnnue_backend_set_draw_rules: repetition and fifty-move draws in the chess searches
  int quiesce = 0;  // fnnue_backend_set_quiesce: capture quiescence depth below the chess searches' leaves
  bool quiesce_checks = false;  // fnnue_backend_set_quiesce_checks: evasions and mates inside it, coded mates answered
  // fnnue_backend_set_variant_quiesce: the same below the variant searches' leaves, with the variants' rule
  // (decided values exist with checks off too: coded mates are answered whenever the depth is set)
  int vquiesce = 0;
  bool vquiesce_checks = false;
  // fnnue_backend_set_variant_draw_rules: repetition and n-move draws in the variant searches, each variant's rule
  bool variant_draw_rules = false;
  int job_plies = 0;  // the chess depth of the go() in flight: analysis_depth, 1 for a go_lines() on a 2-plies channel
  int vjob_plies = 0;  // the same for the variant nets: variant_analysis_depth (0, 1 or 2 plies)
  // a search per ply (one ply or two), and the two-ply search
  bool depth1(int k) const { return (k == kVariantChess ? job_plies : vjob_plies) >= 1; }
  bool depth2(int k) const { return (k == kVariantChess ? job_plies : vjob_plies) == 2; }
  size_t piece_plies = 524288;  // FNNUE_BACKEND_PIECE_PLIES
  bool any_order = true;         // FNNUE_BACKEND_ANY_ORDER=0: wait for the nets' pieces in net order
  size_t tail_plies = 0;         // FNNUE_BACKEND_TAIL_PLIES: a net's last piece cut to about this many
  size_t fill_grain = 64;        // FNNUE_BACKEND_FILL_GRAIN: games per fill task
  size_t size_grain = 256;       // FNNUE_BACKEND_SIZE_GRAIN: batches per sizing task
  size_t stage_grain = 512;      // FNNUE_BACKEND_STAGE_GRAIN: games per text-staging task
  // The worker's time budget ([ref] src/main.rs:316, 343-351: a go() that
  // overruns it fails, and the engine is dropped — its child killed,
  // stockfish.rs:138).  Every wait of a go() is bounded by the call's
  // deadline; a call that overruns it returns FNNUE_E_TIMEOUT and breaks the
  // channel: the device may still be working on the call's pieces (in the
  // channel's buffers), so later calls fail fast and the caller opens a new
  // channel, as the worker restarts its engine.
  uint32_t timeout_ms = kDefaultTimeoutMs;
  bool broken = false;
  Clock::time_point deadline;
  // The capacity-1 channel: a go() runs on its caller's thread holding run_mu,
  // so a second caller waits until the first call is answered
  // (mpsc::channel(1) with one message in flight, without a thread hand-off
  // each way: ~10 µs of a one-batch call).
  std::mutex run_mu;
  bool closed = false;
  Workers pool;
  int pool_threads = 1;
  NetWork net[kKinds];
  std::vector<uint32_t> flen, mlen;  // per batch of the job in flight: FEN / moves text lengths
  std::vector<int8_t> kind;          // per batch: its net slot
  std::vector<uint8_t> bskip;        // per batch: has skipPositions
  std::vector<uint8_t> skip;         // per response of such a batch: skipped
  std::vector<size_t> lbase;         // go_lines: per batch, where fill() puts its lines before close_lines() packs them
  std::mutex stats_mu;
  fnnue_backend_stats stats{};
  // per go(): its clock, positions written so far, host time spent writing / waiting
  Clock::time_point t0;
  uint64_t filled = 0;
  double fill_ms = 0, wait_ms = 0;
  uint32_t syncs = 0, rebuilds = 0;
  // FNNUE_BACKEND_TRACE=1: each go() prints its host timeline (µs since the
  // call started) to stderr — diagnostics only
  bool trace = false;
  std::string tl;
  void mark(const char* what, int k = -1, long pi = -1) {
    if (!trace) return;
    char b[96];
    std::snprintf(b, sizeof(b), "%s[\"%s\",%d,%ld,%.1f]", tl.empty() ? "" : ",", what, k, pi, ms_since(t0) * 1e3);
    tl += b;
  }

  void run(Job& j);
  void release_device() {
    for (NetWork& W : net) W.release();
    for (fnnue_ctx*& c : ctx) {
      fnnue_ctx_free(c);
      c = nullptr;
    }
  }
  bool expired() const { return Clock::now() >= deadline; }
  int timed_out(const char* where);
  int wait_event(hipEvent_t e, const char* what);
  bool streams_idle();
  void abandon_unanswered(Job& j);
  void drain_streams();
  int prepare_moves(Job& j, int k);
  void layout(const Job& j, int k, Piece& P);
  int plan(Job& j, int k);
  int stage_up(Job& j, int k, size_t pi);
  int stage_eval(int k, size_t pi);
  int stage_search(int k, size_t pi);
  int finish(Job& j, int k, bool wait, bool* ready);
  int recover(Job& j, int k, size_t pi);
  void fill(Job& j, int k, const Piece& P);
  void fill_roots(Job& j, int k, const Piece& P, uint64_t ms, uint32_t nps);
  void fill_hostonly(Job& j, const std::vector<size_t>& all_skipped);
  void close_lines(Job& j);
};

int fnnue_backend::timed_out(const char* where) {
  return fail(FNNUE_E_TIMEOUT, std::string("go() overran its budget of ") + std::to_string(timeout_ms) +
                                   " ms (" + where + ", " + std::to_string(ms_since(t0)) + " ms in)");
}

// Waits for an event until the call's deadline: a few microseconds of
// spinning (a small call's piece is back within them), then the CPU is
// yielded between polls, so that a long wait does not hold a core the worker
// threads or the rest of fishnet could use.
int fnnue_backend::wait_event(hipEvent_t e, const char* what) {
  for (uint32_t i = 0;; ++i) {
    const hipError_t q = hipEventQuery(e);
    if (q == hipSuccess) return FNNUE_OK;
    if (q != hipErrorNotReady) return hip_fail(q, what);
    if (expired()) return timed_out(what);
    if (i < 512) {
      for (int p = 0; p < 16; ++p) _mm_pause();
    } else {
      sched_yield();
    }
  }
}

// Nothing of the channel's is left on the device (its streams are drained).
bool fnnue_backend::streams_idle() {
  for (fnnue_ctx* c : ctx)
    if (c && hipStreamQuery(c->stream) == hipErrorNotReady) return false;
  return true;
}

// After a timeout: the batches whose responses were not written fail with
// FNNUE_E_TIMEOUT (those already written stand); the channel is broken.
void fnnue_backend::abandon_unanswered(Job& j) {
  for (NetWork& W : net) {
    for (size_t pi = W.next; pi < W.pieces.size(); ++pi)
      for (size_t i : W.pieces[pi].games) j.rc[i] = FNNUE_E_TIMEOUT;
    if (W.next < W.pieces.size())  // the move work rides in the net's last piece
      for (size_t i : W.roots) j.rc[i] = FNNUE_E_TIMEOUT;
  }
  broken = true;
}

// After an error other than the budget: the pinned images stay in use until
// the device's copies are done, so the streams are drained before the call
// returns — polled, and only until the call's deadline (a stuck device then
// breaks the channel instead of hanging the caller).
void fnnue_backend::drain_streams() {
  for (uint32_t i = 0; !streams_idle(); ++i) {
    if (expired()) {
      broken = true;
      return;
    }
    if (i < 512) {
      for (int p = 0; p < 16; ++p) _mm_pause();
    } else {
      sched_yield();
    }
  }
}

// Move batches of one net, host side: the position after all moves (one per
// batch) and its legal children with their game-end flags.  A batch whose
// root cannot be replayed fails alone; so does one with a child the
// evaluator would reject (e.g. a root with more than 32 pieces, a pocket
// beyond the variant's limits) — checked here, so that the device never
// latches an error for move work (one bad batch no longer fails
// the call).
// The roots are replayed on the pool's threads (each root ~40-70 us of host
// board work: its moves matched against the legal moves, then every child's
// legal moves for its game-end flags), then merged in batch order.
int fnnue_backend::prepare_moves(Job& j, int k) {
  NetWork& W = net[k];
  const bool chess = k == kVariantChess;
  const size_t nr = W.roots.size();
  std::vector<MoveRoot> R(nr);
  std::vector<std::vector<fnnue_pos>> kids(chess ? nr : 0);
  std::vector<std::vector<fnnue_vpos>> vkids(chess ? 0 : nr);
  std::vector<int> rcs(nr, FNNUE_OK);
  pool.run(nr, 1, [&](size_t lo, size_t hi) {
    for (size_t t = lo; t < hi; ++t) {
      const fnnue_acquired& a = j.batches[W.roots[t]];
      int rc = chess ? chess_move_root(a, R[t], kids[t]) : variant_move_root(k, a, R[t], vkids[t]);
      if (rc == FNNUE_OK && chess)
        for (const fnnue_pos& p : kids[t]) rc = rc ? rc : (valid_host_pos(p) ? 0 : (int)FNNUE_E_POSITION);
      if (rc == FNNUE_OK && !chess)
        for (const fnnue_vpos& p : vkids[t]) rc = rc ? rc : (host_vpos_state(p, k) ? 0 : (int)FNNUE_E_POSITION);
      rcs[t] = rc;
    }
  });
  std::vector<size_t> dev_roots;
  for (size_t t = 0; t < nr; ++t) {
    const size_t i = W.roots[t];
    if (rcs[t]) {
      j.rc[i] = rcs[t];
      continue;
    }
    if (R[t].uci.empty()) {
      W.terminal.push_back(i);
      W.troots.push_back(std::move(R[t]));
      continue;
    }
    const uint8_t* src = chess ? reinterpret_cast<const uint8_t*>(kids[t].data())
                               : reinterpret_cast<const uint8_t*>(vkids[t].data());
    const size_t cnt = chess ? kids[t].size() : vkids[t].size();
    W.kid_first.push_back(W.nk);
    W.kids.insert(W.kids.end(), src, src + cnt * W.rec);
    W.nk += cnt;
    W.mroots.push_back(std::move(R[t]));
    dev_roots.push_back(i);
  }
  W.roots.swap(dev_roots);
  return FNNUE_OK;
}

// A piece's image layout from its games (offsets relative to the piece).
void fnnue_backend::layout(const Job& j, int k, Piece& P) {
  const NetWork& W = net[k];
  size_t text = 0, plies = 0;
  for (size_t i : P.games) {
    text += flen[i] + 1 + mlen[i];
    plies += j.off[i + 1] - j.off[i];
  }
  P.ng = (uint32_t)P.games.size();
  P.n = (uint32_t)plies;
  P.nk = P.kids ? W.nk : 0;
  const size_t ng = P.ng, n = P.n, nk = P.nk;
  P.depth1 = depth1(k) && ng;
  P.depth2 = depth2(k) && ng;
  P.nslots = 0;
  if (j.with_lines() && P.depth1)
    for (size_t i : P.games) P.nslots += (size_t)(j.off[i + 1] - j.off[i]) * line_slots(j.batches[i]);
  P.o_fen = align16(text);
  P.o_mv = P.o_fen + 4 * (ng + 1);
  P.o_ply = P.o_mv + 4 * ng;
  P.o_loff = P.o_ply + 4 * (ng + 1);
  P.o_kids = align16(P.o_loff + (P.nslots ? 4 * (n + 1) : 0));
  P.o_res = align16(P.o_kids + nk * W.rec);
  P.o_fin = P.o_res + 16;
  P.o_ps = align16(P.o_fin + ng);
  P.o_po = P.o_ps + 4 * (n + nk);
  P.o_best = align16(P.o_po + 4 * (n + nk));
  P.o_lines = P.o_best + n * (P.depth2 ? sizeof(fnnue_best2) : sizeof(fnnue_best));
  P.end = P.depth1 ? P.o_lines + P.nslots * (P.depth2 ? sizeof(fnnue_line2) : sizeof(fnnue_line)) : P.o_po + 4 * (n + nk);
}

// Cuts the net's games into pieces and places them in its (grow-only) buffers.
int fnnue_backend::plan(Job& j, int k) {
  NetWork& W = net[k];
  W.pieces.clear();
  size_t acc = 0, plies = 0, text = 0;
  // At depth 1 a ply brings about 35 children (at most 218) into the net's
  // grow-only children buffers and the evaluator's workspace: pieces of a 32nd
  // of the plies keep a piece's records where a depth-0 piece's plies are.
  // The variant nets' pieces are cut at an 8th: their children buffers are
  // sized from the count each piece reads back, whatever a ply brings (a
  // crazyhouse ply with full pockets several hundred), and every piece costs
  // that read-back, so fewer and larger pieces measured faster (DESIGN.md
  // §4.16: 1024 crazyhouse batches in 33.1 / 17.4 / 13.4 ms at a 128th / 32nd
  // / 8th).
  // At two plies a ply brings about a thousand grandchildren: a 1024th.  The
  // variant nets' two-plies pieces are cut at a 256th: 64 crazyhouse batches in
  // 59.7 / 46.3 / 38.1 / 33.8 ms at a 2048th / 1024th / 512th / 256th (DESIGN.md
  // §4.18; a piece of 2048 crazyhouse plies holds about 4M grandchild records).
  const size_t cut_plies = !depth1(k)           ? piece_plies
                           : depth2(k)          ? std::max<size_t>(16, piece_plies / (k == kVariantChess ? 1024 : 256))
                           : k == kVariantChess ? std::max<size_t>(1024, piece_plies / 32)
                                                : std::max<size_t>(256, piece_plies / 8);
  for (size_t i : W.games) {
    const size_t t = (size_t)flen[i] + 1 + mlen[i];
    if (W.pieces.empty() || acc >= cut_plies || text + t > kMaxPieceText) {
      W.pieces.emplace_back();
      acc = 0;
      text = 0;
    }
    W.pieces.back().games.push_back(i);
    acc += j.off[i + 1] - j.off[i];
    text += t;
    plies += j.off[i + 1] - j.off[i];
  }
  if (plies >= (1ull << 31)) return fail(FNNUE_E_ARG, "batch too large");
  // A short last piece: its fill is the one the device cannot hide
  if (tail_plies && W.pieces.size() > 1) {
    Piece& L = W.pieces.back();
    size_t t = 0, cut = L.games.size();
    while (cut > 1 && t < tail_plies) {
      --cut;
      t += j.off[L.games[cut] + 1] - j.off[L.games[cut]];
    }
    if (cut > 1 && cut < L.games.size()) {
      Piece T;
      T.games.assign(L.games.begin() + (long)cut, L.games.end());
      L.games.resize(cut);
      W.pieces.push_back(std::move(T));
    }
  }
  if (W.nk) {
    if (W.pieces.empty()) W.pieces.emplace_back();
    W.pieces.back().kids = true;
  }
  size_t up = 0, down = 0, dev = 0, pos = 0, st = 0;
  for (Piece& P : W.pieces) {
    layout(j, k, P);
    if (P.o_fen >= (1ull << 31)) return fail(FNNUE_E_ARG, "batch text too large");
    if (P.nslots > UINT32_MAX) return fail(FNNUE_E_ARG, "too many MultiPV lines in one piece");
    P.up0 = up;
    P.down0 = down;
    P.dev0 = dev;
    P.pos0 = pos;
    P.st0 = st;
    if (P.depth1) st = align256(st + (size_t)P.n * (k == kVariantChess ? sizeof(DBoard) : vstate_bytes(k)));
    up = align256(up + P.o_res + 16);
    down = align256(down + P.end - P.o_res);
    dev = align256(dev + P.end);
    pos = align256(pos + (size_t)P.n * W.rec);
  }
  if (int rc = W.dev.reserve(dev)) return rc;
  if (int rc = W.up.reserve(up)) return rc;
  if (int rc = W.down.reserve(down)) return rc;
  if (pos)
    if (int rc = W.pos.reserve(pos)) return rc;
  if (st)
    if (int rc = W.states.reserve(st)) return rc;
  return W.events(W.pieces.size());
}

// Host image of a piece, then on the context's stream: its upload and the
// replay of its games.  Nothing waits.
int fnnue_backend::stage_up(Job& j, int k, size_t pi) {
  NetWork& W = net[k];
  Piece& P = W.pieces[pi];
  char* img = W.up.at<char>(P.up0);
  uint32_t* fo = reinterpret_cast<uint32_t*>(img + P.o_fen);
  uint32_t* mo = reinterpret_cast<uint32_t*>(img + P.o_mv);
  uint32_t* po = reinterpret_cast<uint32_t*>(img + P.o_ply);
  uint32_t text = 0, acc = 0;
  for (uint32_t g = 0; g < P.ng; ++g) {
    const size_t i = P.games[g];
    fo[g] = text;
    mo[g] = text + flen[i];
    po[g] = acc;
    text += flen[i] + 1 + mlen[i];
    acc += j.off[i + 1] - j.off[i];
  }
  fo[P.ng] = text;
  po[P.ng] = acc;
  if (P.nslots) {  // MultiPV: every ply's slots, in ply order
    uint32_t* lo = reinterpret_cast<uint32_t*>(img + P.o_loff);
    uint32_t slot = 0, p = 0;
    for (uint32_t g = 0; g < P.ng; ++g) {
      const size_t i = P.games[g];
      const uint32_t kk = line_slots(j.batches[i]);
      for (uint32_t q = j.off[i + 1] - j.off[i]; q; --q, slot += kk) lo[p++] = slot;
    }
    lo[p] = slot;
  }
  pool.run(P.ng, stage_grain, [&](size_t lo, size_t hi) {
    for (size_t g = lo; g < hi; ++g) {
      const size_t i = P.games[g];
      const fnnue_acquired& a = j.batches[i];
      char* d = img + fo[g];
      const uint32_t fl = flen[i], ml = mlen[i];
      if (fl) std::memcpy(d, a.position, fl);
      d[fl] = ' ';
      if (ml) std::memcpy(d + fl + 1, a.moves, ml);
    }
  });
  if (P.nk) std::memcpy(img + P.o_kids, W.kids.data(), P.nk * W.rec);
  std::memset(img + P.o_res, 0, 16);
  char* dimg = W.dev.at<char>(P.dev0);
  hipStream_t us = ctx[k]->stream;
  HIP_TRY(hipMemcpyAsync(dimg, img, P.o_res + 16, hipMemcpyHostToDevice, us), "H2D(batch image)");
  if (P.depth1 && k != kVariantChess)
    HIP_TRY(replay_vgames_device(k, dimg, reinterpret_cast<uint32_t*>(dimg + P.o_fen),
                                 reinterpret_cast<uint32_t*>(dimg + P.o_mv), reinterpret_cast<uint32_t*>(dimg + P.o_ply),
                                 P.ng, W.pos.at<fnnue_vpos>(P.pos0), W.states.at<char>(P.st0),
                                 reinterpret_cast<uint8_t*>(dimg + P.o_fin), reinterpret_cast<uint32_t*>(dimg + P.o_res),
                                 us),
            "batch replay launch");
  else if (P.depth1)
    HIP_TRY(replay_chess_states_device(dimg, reinterpret_cast<uint32_t*>(dimg + P.o_fen),
                                       reinterpret_cast<uint32_t*>(dimg + P.o_mv),
                                       reinterpret_cast<uint32_t*>(dimg + P.o_ply), P.ng, W.pos.at<fnnue_pos>(P.pos0),
                                       W.states.at<DBoard>(P.st0), reinterpret_cast<uint8_t*>(dimg + P.o_fin),
                                       reinterpret_cast<uint32_t*>(dimg + P.o_res), us),
            "batch replay launch");
  else if (P.ng)
    HIP_TRY(replay_games_device(k, dimg, reinterpret_cast<uint32_t*>(dimg + P.o_fen),
                                reinterpret_cast<uint32_t*>(dimg + P.o_mv), reinterpret_cast<uint32_t*>(dimg + P.o_ply),
                                P.ng, W.pos.at<char>(P.pos0), reinterpret_cast<uint8_t*>(dimg + P.o_fin),
                                reinterpret_cast<uint32_t*>(dimg + P.o_res), us),
            "batch replay launch");
  mark("up", k, (long)pi);
  return FNNUE_OK;
}

// On the context's stream, behind the piece's replay: the CHAIN evaluation of
// its plies and the children's evaluation (latching into the piece's own
// error word), then the results to the host.  Nothing waits.
int fnnue_backend::stage_eval(int k, size_t pi) {
  NetWork& W = net[k];
  Piece& P = W.pieces[pi];
  fnnue_ctx* c = ctx[k];
  hipStream_t s = c->stream;
  const bool chess = k == kVariantChess;
  char* dimg = W.dev.at<char>(P.dev0);
  int32_t* d_ps = reinterpret_cast<int32_t*>(dimg + P.o_ps);
  int32_t* d_po = reinterpret_cast<int32_t*>(dimg + P.o_po);
  struct ErrWord {  // the context's error word, redirected for this piece's launches
    fnnue_ctx* c;
    uint32_t* saved;
    ~ErrWord() { c->err = saved; }
  } ew{c, c->err};
  c->err = reinterpret_cast<uint32_t*>(dimg + P.o_res) + 3;
  P.searched = 0;
  if (P.depth1) {
    if (int rc = stage_search(k, pi)) return rc;
  } else if (P.ng) {
    const uint32_t* d_off = reinterpret_cast<const uint32_t*>(dimg + P.o_ply);
    const void* d_pos = W.pos.at<char>(P.pos0);
    if (int rc = eval_groups(SearchRules{k}, c, d_pos, d_off, P.ng, P.n, FNNUE_GROUP_CHAIN, d_ps, d_po, s)) return rc;
  }
  if (P.nk) {
    const void* d_kids = dimg + P.o_kids;
    const int rc = chess ? fnnue_eval_positions_device(c, static_cast<const fnnue_pos*>(d_kids), P.nk, d_ps + P.n,
                                                       d_po + P.n, s)
                         : fnnue_eval_vpositions_device(c, static_cast<const fnnue_vpos*>(d_kids), P.nk, d_ps + P.n,
                                                        d_po + P.n, s);
    if (rc) return rc;
  }
  HIP_TRY(hipMemcpyAsync(W.down.at<char>(P.down0), dimg + P.o_res, P.end - P.o_res, hipMemcpyDeviceToHost, s),
          "D2H(results)");
  HIP_TRY(hipEventRecord(W.ev_done[pi], s), "hipEventRecord(results)");
  P.pending = true;
  mark("eval", k, (long)pi);
  return FNNUE_OK;
}

// Analysis at depth 1, a piece of a net at depth 1 (chess, or a variant net
// over its own boards and rules): behind its replay the children of every
// ply are counted and the count read back (the builder's sizing read-back,
// with the replay's error word: a piece with a rejected game skips the search
// and goes to recover() as it is); then the children with their moves and end
// flags, their STAR evaluation, the reduction into the results image and each
// ply's own terms (a ply without a legal move reports them, as at depth 0).
// The wait is bounded by the call's deadline.
int fnnue_backend::stage_search(int k, size_t pi) {
  NetWork& W = net[k];
  Piece& P = W.pieces[pi];
  fnnue_ctx* c = ctx[k];
  hipStream_t s = c->stream;
  char* dimg = W.dev.at<char>(P.dev0);
  const uint32_t n = P.n;
  const SearchRules rules{k};
  // this backend's bounded wait for a size the device wrote to hs[1]
  if (int rc = W.sizing.reserve(8)) return rc;
  uint32_t* hs = W.sizing.at<uint32_t>(0);
  auto read_size = [&](const uint32_t* d_size, const char* what) {
    HIP_TRY(hipMemcpyAsync(hs + 1, d_size, 4, hipMemcpyDeviceToHost, s), "D2H(size)");
    HIP_TRY(hipEventRecord(W.ev_done[pi], s), "hipEventRecord(size)");
    const auto tw = Clock::now();
    const int rc = wait_event(W.ev_done[pi], what);
    wait_ms += ms_since(tw);
    ++syncs;
    return rc;
  };
  StarGroups g;  // the plies' groups: their children
  g.states = W.states.at<char>(P.st0);
  g.n = n;
  uint32_t *cnt = nullptr, *coff = nullptr;
  if (int rc = reserve(W.kid_cnt, (size_t)(n + 1) * 4, &cnt)) return rc;
  if (int rc = reserve(W.kid_off, (size_t)(n + 1) * 4, &coff)) return rc;
  g.off = coff;
  HIP_TRY(count_children(rules, g.states, n, cnt, coff, s, W.bscratch), "children count launch");
  HIP_TRY(hipMemcpyAsync(hs, dimg + P.o_res, 4, hipMemcpyDeviceToHost, s), "D2H(builder error)");
  if (int rc = read_size(coff + n, "sizing a piece's children")) return rc;
  if (hs[0]) return FNNUE_OK;  // a rejected game: its boards are not those of a game
  const size_t total = hs[1];
  g.total = (uint32_t)total;
  void* kp = nullptr;
  uint16_t* km = nullptr;
  if (int rc = reserve(W.kid_pos, total * W.rec, &kp)) return rc;
  if (int rc = reserve(W.kid_moves, total * 2, &km)) return rc;
  if (int rc = reserve(W.kid_end, total, &g.end)) return rc;
  if (int rc = reserve(W.kid_ps, total * 4, &g.psqt)) return rc;
  if (int rc = reserve(W.kid_po, total * 4, &g.positional)) return rc;
  g.moves = km;
  HIP_TRY(write_children(rules, g.states, n, coff, g.total, kp, km, g.end, s), "children launch");
  // The draw rules (fnnue_backend_set_draw_rules for chess batches,
  // fnnue_backend_set_variant_draw_rules for a variant's): a piece holds
  // whole games (plan() never cuts one), so the history of its plies is
  // complete; the marks go on the listed plies' children here and on their
  // grandchildren behind the second expansion, before the reductions.
  SearchSettings set{nullptr, rules.chess() ? quiesce : vquiesce, rules.chess() ? quiesce_checks : vquiesce_checks};
  DrawHistory hist;
  if (rules.chess() ? draw_rules : variant_draw_rules) {
    if (int rc = draw_history_level1(rules, dimg, reinterpret_cast<const uint32_t*>(dimg + P.o_fen),
                                     reinterpret_cast<const uint32_t*>(dimg + P.o_mv),
                                     reinterpret_cast<const uint32_t*>(dimg + P.o_ply), P.ng, g.states, n, coff, km,
                                     g.end, s, W.bscratch, &hist, nullptr))
      return rc;
    set.draws = &hist;
  }
  if (int rc = eval_groups(rules, c, kp, coff, n, total, FNNUE_GROUP_STAR, g.psqt, g.positional, s)) return rc;
  P.searched = total - n;
  QuiesceStats qs;
  if (P.depth2) {
    // Two plies: the children's boards, their own children counted and the
    // count read back (the second sizing wait), then the piece as one chunk:
    // one fnnue_best per child; the second reduction into the results image,
    // and for a go_lines_pv() call the lines with their replies.
    const size_t nkid = total - n;
    fnnue_best* kb = nullptr;
    if (int rc = reserve(W.kid_best, (nkid + 1) * sizeof(fnnue_best), &kb)) return rc;
    if (nkid) {
      void* ks = nullptr;
      uint32_t *gcnt = nullptr, *goff = nullptr;
      if (int rc = reserve(W.kid_states, nkid * rules.state_bytes(), &ks)) return rc;
      if (int rc = reserve(W.kid2_cnt, (nkid + 1) * 4, &gcnt)) return rc;
      if (int rc = reserve(W.kid2_off, (nkid + 1) * 4, &goff)) return rc;
      HIP_TRY(child_states(rules, g.states, n, coff, g.total, ks, nullptr, s), "child_states launch");
      HIP_TRY(count_children(rules, ks, (uint32_t)nkid, gcnt, goff, s, W.bscratch), "grandchildren count launch");
      if (int rc = read_size(goff + nkid, "sizing a piece's grandchildren")) return rc;
      const size_t gtotal = hs[1];
      Level2Chunk ch;
      ch.p1 = n, ch.nk = (uint32_t)nkid, ch.nr = (uint32_t)gtotal;
      ch.ch_off = goff;
      if (int rc = reserve(W.g_pos, gtotal * W.rec, &ch.pos)) return rc;
      if (int rc = reserve(W.g_moves, gtotal * 2, &ch.moves)) return rc;
      if (int rc = reserve(W.g_end, gtotal, &ch.end)) return rc;
      if (int rc = reserve(W.g_ps, gtotal * 4, &ch.psqt)) return rc;
      if (int rc = reserve(W.g_po, gtotal * 4, &ch.positional)) return rc;
      if (int rc = search_level2_chunk(c, W.bscratch, rules, set, g, ks, goff, ch, kb, s, &qs, nullptr)) return rc;
      P.searched += gtotal - nkid;
    }
    HIP_TRY(best_replies(rules.vranks(), g.end, km, coff, n, g.total, kb, nullptr,
                         reinterpret_cast<fnnue_best2*>(dimg + P.o_best), s),
            "best_replies launch");
    if (P.nslots)
      HIP_TRY(topk_replies(rules.vranks(), g.end, km, coff, n, g.total, kb, nullptr,
                           reinterpret_cast<const uint32_t*>(dimg + P.o_loff), 0,
                           reinterpret_cast<fnnue_line2*>(dimg + P.o_lines), P.nslots, s),
              "topk_replies launch");
  } else {
    // One ply: the reduction into the results image, and the lines of a go_lines() call that asked for MultiPV
    if (int rc = reduce_level1(c, W.bscratch, rules, set, g, reinterpret_cast<fnnue_best*>(dimg + P.o_best),
                               reinterpret_cast<const uint32_t*>(dimg + P.o_loff), 0,
                               P.nslots ? reinterpret_cast<fnnue_line*>(dimg + P.o_lines) : nullptr, P.nslots, s, &qs))
      return rc;
  }
  syncs += (uint32_t)qs.syncs;
  HIP_TRY(launch_gather_parents(g.psqt, g.positional, coff, n, g.total, reinterpret_cast<int32_t*>(dimg + P.o_ps),
                                reinterpret_cast<int32_t*>(dimg + P.o_po), s),
          "gather_parents launch");
  return FNNUE_OK;
}

// The net's next piece: when its results are on the host (waiting for them if
// `wait`), writes its responses — after recovering, if the builder or the
// evaluator reported an error.  *ready = false: not there yet.
int fnnue_backend::finish(Job& j, int k, bool wait, bool* ready) {
  NetWork& W = net[k];
  const size_t pi = W.next;
  *ready = false;
  if (wait) {
    const auto tw = Clock::now();
    mark("wait", k, (long)pi);
    const int rc = wait_event(W.ev_done[pi], "waiting for a piece's results");
    wait_ms += ms_since(tw);
    ++syncs;
    if (rc) return rc;
  } else {
    const hipError_t q = hipEventQuery(W.ev_done[pi]);
    if (q == hipErrorNotReady) return FNNUE_OK;
    HIP_TRY(q, "hipEventQuery");
  }
  *ready = true;
  Piece& P = W.pieces[pi];
  P.pending = false;
  const uint32_t* err = W.down.at<uint32_t>(P.down0);
  if (err[0] || err[3])
    if (int rc = recover(j, k, pi)) return rc;
  fill(j, k, P);
  ++W.next;
  return FNNUE_OK;
}

// A game the builder rejected (FEN / move), or whose positions the evaluator
// rejects, fails its own batch: it is dropped from its piece and the piece is
// staged again (its own error words: the other pieces are not affected).
int fnnue_backend::recover(Job& j, int k, size_t pi) {
  NetWork& W = net[k];
  Piece& P = W.pieces[pi];
  for (;;) {
    const uint32_t* berr = W.down.at<uint32_t>(P.down0);
    const uint32_t cerr = berr[3];
    if (!berr[0] && !cerr) break;
    if (berr[0]) {
      // The replay flags every game it rejected (kFinalFailed | code in the
      // game's flag byte); those batches fail (PositionFailed) and the rest
      // are staged again, in one pass however many failed.  A count mismatch
      // or a game index outside the piece cannot be blamed on any batch: the
      // call fails.
      auto bad_word = [&](uint32_t code, uint32_t g) {
        return fail(FNNUE_E_DEVICE, "batch builder reported game " + std::to_string(g) + " of " +
                                        std::to_string(P.ng) + " (code " + std::to_string(code) + ")");
      };
      if (berr[0] == kBuildErrCount || berr[1] >= P.ng) return bad_word(berr[0], berr[1]);
      const uint8_t* fin = W.down.at<uint8_t>(P.down0) + (P.o_fin - P.o_res);
      std::vector<size_t> keep;
      keep.reserve(P.games.size());
      for (uint32_t g = 0; g < P.ng; ++g) {
        const uint32_t code = fin[g] & kFinalFailed ? fin[g] & ~kFinalFailed & 0xFFu : 0u;
        if (code == kBuildErrCount || code > kBuildErrCount) return bad_word(code, g);
        if (code)
          j.rc[P.games[g]] = code == kBuildErrFen ? FNNUE_E_FEN : FNNUE_E_MOVE;
        else
          keep.push_back(P.games[g]);
      }
      if (keep.size() == P.games.size()) return bad_word(berr[0], berr[1]);  // the named game carries no flag
      P.games.swap(keep);
    } else {
      // A FEN the builder parses but the evaluator cannot (kings, > 32
      // pieces): find the games holding such positions, fail those batches.
      // (Move-work children were checked on the host.)
      const size_t nbytes = (size_t)P.n * W.rec;
      if (int rc = W.scratch.reserve(nbytes + 1)) return rc;
      const uint8_t* hpos = W.scratch.at<uint8_t>(0);
      if (nbytes) {
        hipStream_t s = ctx[k]->stream;
        HIP_TRY(hipMemcpyAsync(W.scratch.p, W.pos.at<char>(P.pos0), nbytes, hipMemcpyDeviceToHost, s),
                "D2H(positions)");
        HIP_TRY(hipEventRecord(W.ev_done[pi], s), "hipEventRecord(positions)");
        if (int rc = wait_event(W.ev_done[pi], "reading a failing piece's positions")) return rc;
      }
      ++syncs;
      const uint32_t* ply = W.up.at<uint32_t>(P.up0 + P.o_ply);
      std::vector<size_t> keep;
      for (uint32_t g = 0; g < P.ng; ++g) {
        bool ok = true;
        for (uint32_t x = ply[g]; x < ply[g + 1] && ok; ++x) {
          const uint8_t* p = hpos + (size_t)x * W.rec;
          ok = k == kVariantChess ? valid_host_pos(*reinterpret_cast<const fnnue_pos*>(p))
                                  : host_vpos_state(*reinterpret_cast<const fnnue_vpos*>(p), k) != 0;
        }
        if (ok)
          keep.push_back(P.games[g]);
        else
          j.rc[P.games[g]] = FNNUE_E_POSITION;
      }
      if (keep.size() == P.games.size())
        return fail(cerr & 2u ? FNNUE_E_DEVICE : FNNUE_E_POSITION,
                    "the evaluator latched error " + std::to_string(cerr) + " on piece " + std::to_string(pi) + " of " +
                        std::to_string(W.pieces.size()) + " (net " + std::to_string(k) + ", " + std::to_string(P.ng) +
                        " games, " + std::to_string(P.n) + " plies, pass " + std::to_string(rebuilds) +
                        ") and no batch of the piece holds an invalid position");
      P.games.swap(keep);
    }
    ++rebuilds;
    layout(j, k, P);  // fewer games: the piece still fits its place
    if (int rc = stage_up(j, k, pi)) return rc;
    if (int rc = stage_eval(k, pi)) return rc;
    const int rc = wait_event(W.ev_done[pi], "waiting for a restaged piece");
    ++syncs;
    if (rc) return rc;
    P.pending = false;
  }
  return FNNUE_OK;
}

// Responses of one piece's games from its results image (several threads for
// large pieces): analysis plies as Score::Cp, a game's last ply with no legal
// move as mate 0 / cp 0; then the move work it carries.  time / nps: the wall
// time of the go() call until these results were on the host, and the
// positions evaluated by then per second.  Full records or the compact form.
void fnnue_backend::fill(Job& j, int k, const Piece& P) {
  const auto tf = Clock::now();
  NetWork& W = net[k];
  mark("fill", k, (long)(&P - W.pieces.data()));
  const char* res = W.down.at<char>(P.down0);  // the results image from o_res on
  const uint8_t* fin = reinterpret_cast<const uint8_t*>(res + (P.o_fin - P.o_res));
  const int32_t* ps = reinterpret_cast<const int32_t*>(res + (P.o_ps - P.o_res));
  const int32_t* po = reinterpret_cast<const int32_t*>(res + (P.o_po - P.o_res));
  const uint32_t* ply = W.up.at<uint32_t>(P.up0 + P.o_ply);
  filled += P.n + P.nk + P.searched;
  const fnnue_best* best = P.depth1 && !P.depth2 ? reinterpret_cast<const fnnue_best*>(res + (P.o_best - P.o_res)) : nullptr;
  const fnnue_best2* best2 = P.depth2 ? reinterpret_cast<const fnnue_best2*>(res + (P.o_best - P.o_res)) : nullptr;
  const bool with_lines = P.depth1 && P.nslots && j.with_lines();
  const fnnue_line* dlines =
      with_lines && !P.depth2 ? reinterpret_cast<const fnnue_line*>(res + (P.o_lines - P.o_res)) : nullptr;
  const fnnue_line2* dlines2 =
      with_lines && P.depth2 ? reinterpret_cast<const fnnue_line2*>(res + (P.o_lines - P.o_res)) : nullptr;
  const uint32_t* loff = with_lines ? W.up.at<uint32_t>(P.up0 + P.o_loff) : nullptr;
  const double el = ms_since(t0);
  const uint64_t ms = (uint64_t)el;
  const uint32_t nps = el > 0 ? (uint32_t)std::min(4.0e9, (double)filled / (el * 1e-3)) : 0;
  const int32_t nrm = norm;
  const ResponseTail tail(ms, nps);
  // coded mates: chess searches with quiescence checks, variant searches with a quiescence depth (the variants'
  // rule decides finished positions with checks off too); otherwise no value is ever remapped
  const ScoreRule rule{nrm, k == kVariantChess ? quiesce_checks && quiesce > 0 : vquiesce > 0};
  pool.run(P.ng, fill_grain, [&](size_t lo, size_t hi) {
    for (size_t g = lo; g < hi; ++g) {
      const size_t i = P.games[g];
      const uint32_t b = j.off[i], len = j.off[i + 1] - b;
      const uint8_t matrix = j.batches[i].multipv > 0 ? 1 : 0;  // Work::matrix_wanted: multipv is Some
      const bool sk = bskip[i];
      const int32_t* gps = ps + ply[g];
      const int32_t* gpo = po + ply[g];
      // The last ply is the only one that can have no legal move (nothing can
      // be played from it): mate 0 / cp 0 instead of an evaluation.
      const bool ends = fin[g] & kFinalNoMoves;
      const uint8_t end_kind = (fin[g] & kFinalDecided) ? FNNUE_SCORE_MATE : FNNUE_SCORE_CP;
      if (j.cout) {  // the compact form's batch record, whatever the plies' answers come from
        fnnue_batch_compact& B = j.bout[i];
        B.time_ms = ms;
        B.nps = nps;
        B.nodes = 0;
        std::memset(B.best_move, 0, sizeof(B.best_move));
      }
      // Ply q's answer from its record B, full or compact: a fnnue_best2 (two plies), a fnnue_best, or at
      // depth 0 the ply's own value as one.  A ply without a child is the game's last one without a legal move:
      // mate 0 / cp 0 with its own terms.  true: a full record was written for a ply with a move.
      const uint8_t fl = matrix ? FNNUE_COMPACT_MATRIX : 0;
      auto answer = [&](uint32_t q, const auto& B, uint8_t pv_len, const ScoreRule& rule) {
        const bool none = B.kind == FNNUE_BEST_NONE;
        const Answer a = none ? Answer{end_kind, 0} : rule(B.kind, B.value);
        const int32_t rps = none ? gps[q] : B.psqt, rpo = none ? gpo[q] : B.positional;
        const uint8_t depth = none ? 0 : pv_len;
        const bool skipped = sk && skip[b + q];
        if (j.cout) {
          if (skipped)
            put_compact(j.cout + b + q, 0, 0, 0, 0, 0, FNNUE_COMPACT_SKIPPED);
          else
            put_compact(j.cout + b + q, rps, rpo, (int32_t)a.score, a.kind, depth, none ? fl | FNNUE_COMPACT_NO_MOVES : fl);
          return false;
        }
        fnnue_position_response* r = j.out + b + q;
        if (skipped) {
          put_response(r, response_head(q, 1, 0, 0, 0), 0, 0, 0, 0, tail);
          return false;
        }
        put_response(r, response_head(q, 0, a.kind, depth, matrix), a.score, rps, rpo, none ? 0 : B.nodes, tail);
        if (!none && B.move) move_uci(k, B.move, r->best_move);
        return !none;
      };
      if (best2 || best) {
        const uint32_t kk = dlines2 || dlines ? line_slots(j.batches[i]) : 0;
        // the lines go to the batch's provisional place, lbase[i] + q * kk (close_lines() packs them afterwards)
        for (uint32_t q = 0; q < len; ++q) {
          uint32_t nl = 0;
          if (best2) {
            const fnnue_best2& B = best2[ply[g] + q];
            if (!answer(q, B, B.pv_len, rule)) continue;
            if (j.reply) j.reply[b + q] = B.reply;
            if (!kk) continue;
            // MultiPV at two plies: the ply's lines until the first unused slot
            // (the slots beyond its legal moves are all-zero)
            const fnnue_line2* src = dlines2 + loff[ply[g] + q];
            const size_t at = lbase[i] + (size_t)q * kk;
            for (; nl < kk && src[nl].kind != FNNUE_BEST_NONE; ++nl) {
              const fnnue_line2& L = src[nl];
              char rp[8] = {0};
              if (L.pv_len == 2) move_uci(k, L.reply, rp);
              j.lines2[at + nl] = pv_line2(k, rule, L, rp);
            }
          } else {
            const fnnue_best& B = best[ply[g] + q];
            if (!answer(q, B, 1, rule) || !kk) continue;
            // MultiPV: the first min(slots, nodes) lines of the ply
            const fnnue_line* src = dlines + loff[ply[g] + q];
            const size_t at = lbase[i] + (size_t)q * kk;
            nl = std::min(kk, B.nodes);
            for (uint32_t l = 0; l < nl; ++l) {
              const fnnue_line& L = src[l];
              if (!j.lines) {  // go_lines_pv at one ply: the same line in the two-ply record
                j.lines2[at + l] = pv_line2(k, rule, L, "");
                continue;
              }
              const Answer a = rule(L.kind, L.value);
              char mv[8] = {0};
              move_uci(k, L.move, mv);
              fnnue_pv_line out{};
              out.score = a.score;
              out.psqt = L.psqt;
              out.positional = L.positional;
              std::memcpy(out.move, mv, 6);  // at most "e7e8q" and its NUL
              out.score_kind = a.kind;
              j.lines[at + l] = out;
            }
          }
          j.line_off[b + q + 1] = nl;  // a count for now
        }
        continue;
      }
      // Depth 0: every ply's own value in centipawns (never a coded mate), but the last without a legal move
      for (uint32_t q = 0; q < len; ++q) {
        fnnue_best B{};
        B.kind = q + 1 == len && ends ? FNNUE_BEST_NONE : FNNUE_BEST_CP;
        B.value = (int32_t)(((int64_t)gps[q] + gpo[q]) / 16);  // OutputScale, C truncation
        B.psqt = gps[q];
        B.positional = gpo[q];
        B.nodes = 1;
        answer(q, B, 0, ScoreRule{nrm, false});
      }
    }
  });
  if (P.kids) fill_roots(j, k, P, ms, nps);
  fill_ms += ms_since(tf);
  mark("filled", k, (long)(&P - W.pieces.data()));
}

// Move work: a one-ply search over each root's children.
void fnnue_backend::fill_roots(Job& j, int k, const Piece& P, uint64_t ms, uint32_t nps) {
  NetWork& W = net[k];
  const char* res = W.down.at<char>(P.down0);
  const int32_t* kps = reinterpret_cast<const int32_t*>(res + (P.o_ps - P.o_res)) + P.n;
  const int32_t* kpo = reinterpret_cast<const int32_t*>(res + (P.o_po - P.o_res)) + P.n;
  for (size_t t = 0; t < W.roots.size(); ++t) {
    const MoveRoot& R = W.mroots[t];
    const size_t i = W.roots[t];
    // rank: 2 = mates, 1 = evaluated, 0 = loses at once (value orders within a rank)
    size_t best = 0;
    int best_rank = -1;
    int64_t bv = INT64_MIN;
    for (size_t q = 0; q < R.uci.size(); ++q) {
      const size_t x = W.kid_first[t] + q;
      const uint8_t f = R.kid_fin[q];
      int rank = 1;
      int64_t v;
      if (f & kFinalWon) {
        rank = 0;
        v = 0;
      } else if (f & kFinalDecided && (f & kFinalNoMoves)) {
        rank = 2;
        v = 0;
      } else if (f & kFinalNoMoves) {
        v = 0;  // stalemate
      } else {
        v = -(((int64_t)kps[x] + kpo[x]) / 16);  // Stockfish value of the child, negated
      }
      if (rank > best_rank || (rank == best_rank && v > bv)) {
        best_rank = rank;
        bv = v;
        best = q;
      }
    }
    const size_t x = W.kid_first[t] + best;
    // the ranks as the searches' records name them: no coded mates at this depth
    const Answer a = ScoreRule{norm, false}(
        best_rank == 2 ? FNNUE_BEST_MATE : best_rank == 0 ? FNNUE_BEST_LOST : FNNUE_BEST_CP, bv);
    if (j.cout) {
      put_compact(j.cout + j.off[i], -kps[x], -kpo[x], (int32_t)a.score, a.kind, 1, 0);
      fnnue_batch_compact& B = j.bout[i];
      B.time_ms = ms;
      B.nps = nps;
      B.nodes = (uint32_t)R.uci.size();
      std::memset(B.best_move, 0, sizeof(B.best_move));
      std::strncpy(B.best_move, R.uci[best].c_str(), sizeof(B.best_move) - 1);
      continue;
    }
    fnnue_position_response& r = j.out[j.off[i]];
    std::memset(&r, 0, sizeof(r));
    r.time_ms = ms;
    r.nps = nps;
    r.psqt = -kps[x];
    r.positional = -kpo[x];
    r.depth = 1;
    r.nodes = R.uci.size();
    r.score_kind = a.kind;
    r.score = a.score;
    std::strncpy(r.best_move, R.uci[best].c_str(), sizeof(r.best_move) - 1);
  }
}

// The batches answered without the device: move-work roots without a legal
// move, analysis batches whose every position is skipped.
void fnnue_backend::fill_hostonly(Job& j, const std::vector<size_t>& all_skipped) {
  const double el = ms_since(t0);
  const uint64_t ms = (uint64_t)el;
  const uint32_t nps = el > 0 ? (uint32_t)std::min(4.0e9, (double)filled / (el * 1e-3)) : 0;
  auto batch = [&](size_t i) {
    fnnue_batch_compact& B = j.bout[i];
    std::memset(&B, 0, sizeof(B));
    B.time_ms = ms;
    B.nps = nps;
  };
  for (int k = 0; k < kKinds; ++k) {
    NetWork& W = net[k];
    for (size_t t = 0; t < W.terminal.size(); ++t) {
      const size_t i = W.terminal[t];
      const uint8_t fin = W.troots[t].fin;
      if (j.cout) {
        put_compact(j.cout + j.off[i], 0, 0, 0,
                    (fin & kFinalDecided) ? FNNUE_SCORE_MATE : FNNUE_SCORE_CP, 0,
                    FNNUE_COMPACT_NO_MOVES);
        batch(i);
        continue;
      }
      fnnue_position_response& r = j.out[j.off[i]];
      std::memset(&r, 0, sizeof(r));
      r.time_ms = ms;
      r.nps = nps;
      terminal_response(r, fin);
    }
  }
  for (size_t i : all_skipped) {
    if (j.cout) batch(i);
    for (uint32_t q = j.off[i]; q < j.off[i + 1]; ++q) {
      if (j.cout) {
        put_compact(j.cout + q, 0, 0, 0, 0, 0, FNNUE_COMPACT_SKIPPED);
        continue;
      }
      fnnue_position_response& r = j.out[q];
      std::memset(&r, 0, sizeof(r));
      r.position_id = q - j.off[i];
      r.skipped = 1;
      r.time_ms = ms;
      r.nps = nps;
    }
  }
}

// go_lines: fill() left every response's lines at its batch's provisional
// place (lbase: the bound's own prefix sums, so they never overlap) and its
// count in line_off; here the lines are packed in response order and the
// counts become offsets.  A batch that failed keeps an empty range.
void fnnue_backend::close_lines(Job& j) {
  if (!j.with_lines()) return;
  char* const base = j.lines ? reinterpret_cast<char*>(j.lines) : reinterpret_cast<char*>(j.lines2);
  const size_t sz = j.lines ? sizeof(fnnue_pv_line) : sizeof(fnnue_pv_line2);
  size_t w = 0;
  j.line_off[0] = 0;
  for (size_t i = 0; i < j.nb; ++i) {
    const uint32_t kk = line_slots(j.batches[i]);
    for (uint32_t r = j.off[i]; r < j.off[i + 1]; ++r) {
      const uint32_t nl = j.rc[i] ? 0 : j.line_off[r + 1];
      const size_t from = lbase[i] + (size_t)(r - j.off[i]) * kk;
      if (nl && from != w) std::memmove(base + w * sz, base + from * sz, nl * sz);
      w += nl;
      j.line_off[r + 1] = (uint32_t)w;
    }
  }
}

void fnnue_backend::run(Job& j) {
  t0 = Clock::now();
  deadline = t0 + std::chrono::milliseconds(j.timeout_ms ? j.timeout_ms : timeout_ms);
  tl.clear();
  filled = 0;
  fill_ms = wait_ms = 0;
  syncs = rebuilds = 0;
  job_plies = analysis_depth == 2 && j.lines ? 1 : analysis_depth;  // MultiPV is a one-ply search
  vjob_plies = variant_analysis_depth == 2 && j.lines ? 1 : variant_analysis_depth;
  const size_t nb = j.nb;
  flen.resize(nb);
  mlen.resize(nb);
  // sizes (IncomingBatch::from_acquired: moves + 1 positions, or 1 for move
  // work) and each batch's net; the strings are scattered in the caller's
  // memory, so the next batches' are prefetched
  kind.resize(nb);
  bskip.resize(nb);
  pool.run(nb, size_grain, [&](size_t lo, size_t hi) {
    for (size_t i = lo; i < hi; ++i) {
      if (i + 8 < hi) {
        __builtin_prefetch(j.batches[i + 8].moves);
        __builtin_prefetch(j.batches[i + 8].position);
      }
      const fnnue_acquired& a = j.batches[i];
      size_t fl = a.position ? std::strlen(a.position) : 0, ml = 0;
      int rc = FNNUE_OK;
      uint32_t n = 0;
      if (a.work == FNNUE_WORK_MOVE) {
        n = 1;
        ml = a.moves ? std::strlen(a.moves) : 0;
      } else if (a.work != FNNUE_WORK_ANALYSIS || (a.nskip && !a.skip_positions)) {
        rc = FNNUE_E_ARG;
      } else {
        n = (uint32_t)(a.moves ? scan_tokens(a.moves, &ml) : 0) + 1;
      }
      // text beyond any real batch fails that batch alone (it
      // used to be clamped, failing the whole call later)
      if (rc == FNNUE_OK && (fl > kMaxFenBytes || ml > kMaxMovesBytes)) {
        rc = FNNUE_E_ARG;
        fl = ml = 0;
      }
      flen[i] = (uint32_t)fl;
      mlen[i] = (uint32_t)ml;
      const int kd = kind_of(a.variant);
      if (rc == FNNUE_OK && (kd < 0 || !ctx[kd])) rc = FNNUE_E_ARCH;  // no net for this variant on this backend
      if (rc == FNNUE_OK && a.multipv < 0) rc = FNNUE_E_ARG;
      kind[i] = (int8_t)kd;
      bskip[i] = a.nskip != 0;
      j.rc[i] = rc;
      j.off[i + 1] = n;  // counts for now, offsets below (a failed batch keeps its responses' place)
    }
  });
  mark("sizes");
  j.off[0] = 0;
  uint64_t total = 0;
  for (size_t i = 0; i < nb; ++i) {
    total += j.off[i + 1];
    j.off[i + 1] = (uint32_t)total;
  }
  if (total > UINT32_MAX) {  // the offsets are 32-bit
    j.ret = fail(FNNUE_E_ARG, "the batches expand to " + std::to_string(total) + " responses, more than 2^32 - 1");
    j.err = g_err;
    return;
  }
  if (j.off[nb] > j.cap) {
    j.ret = fail(FNNUE_E_CAPACITY, "response buffer holds " + std::to_string(j.cap) + ", batches need " +
                                       std::to_string(j.off[nb]));
    j.err = g_err;
    return;
  }
  for (NetWork& W : net) W.clear();
  if (j.reply) std::memset(j.reply, 0, (size_t)j.off[nb] * sizeof(fnnue_move));  // none until fill() says otherwise
  if (j.with_lines()) {  // every response without lines until fill() says otherwise
    std::memset(j.line_off, 0, ((size_t)j.off[nb] + 1) * sizeof(uint32_t));
    lbase.resize(nb);
    size_t at = 0;
    for (size_t i = 0; i < nb; ++i) {
      lbase[i] = at;
      at += (size_t)(j.off[i + 1] - j.off[i]) * line_slots(j.batches[i]);
    }
  }
  if (skip.size() < j.off[nb]) skip.resize(j.off[nb]);  // read only for batches with bskip set
  std::vector<size_t> all_skipped;
  for (size_t i = 0; i < nb; ++i) {
    if (j.rc[i]) continue;
    const fnnue_acquired& a = j.batches[i];
    const int kd = kind[i];
    if (a.work == FNNUE_WORK_MOVE) {
      net[kd].roots.push_back(i);
      continue;
    }
    if (bskip[i]) {
      const uint32_t n = j.off[i + 1] - j.off[i];
      uint32_t live = n;
      std::memset(skip.data() + j.off[i], 0, n);
      for (size_t q = 0; q < a.nskip; ++q)  // positions.get_mut(skip): out-of-range ids are ignored
        if (a.skip_positions[q] < n && !skip[j.off[i] + a.skip_positions[q]]) {
          skip[j.off[i] + a.skip_positions[q]] = 1;
          --live;
        }
      if (!live) {
        all_skipped.push_back(i);  // completed without the engine (IncomingError::AllSkipped)
        continue;
      }
    }
    net[kd].games.push_back(i);
  }
  mark("classified");
  int rc = FNNUE_OK;
  size_t rounds = 0;
  for (int k = 0; k < kKinds && rc == FNNUE_OK; ++k) {
    NetWork& W = net[k];
    W.rec = k == kVariantChess ? sizeof(fnnue_pos) : sizeof(fnnue_vpos);
    if (!W.roots.empty()) rc = prepare_moves(j, k);
    if (rc == FNNUE_OK && (!W.games.empty() || W.nk)) rc = plan(j, k);
    rounds = std::max(rounds, W.pieces.size());
  }
  if (rc == FNNUE_OK && expired()) rc = timed_out("sizing and planning");
  mark("planned");
  // Enqueue order: every net's first upload + replay (the nets' streams run
  // side by side), then each round's evaluations behind the next round's
  // uploads; pieces whose results are back are written between the steps.
  auto poll = [&](bool wait) -> int {
    for (int k = 0; k < kKinds; ++k) {
      NetWork& W = net[k];
      while (W.next < W.pieces.size() && W.pieces[W.next].pending) {
        bool ready = false;
        if (int e = finish(j, k, wait, &ready)) return e;
        if (!ready) break;
      }
    }
    return FNNUE_OK;
  };
  for (size_t r = 0; r <= rounds && rc == FNNUE_OK; ++r) {
    if (r && expired()) {
      rc = timed_out("staging pieces");
      break;
    }
    for (int k = 0; k < kKinds && rc == FNNUE_OK; ++k)
      if (r < net[k].pieces.size()) rc = stage_up(j, k, r);
    for (int k = 0; k < kKinds && rc == FNNUE_OK; ++k)
      if (r >= 1 && r - 1 < net[k].pieces.size()) rc = stage_eval(k, r - 1);
    if (rc == FNNUE_OK && r >= 1 && r < rounds) rc = poll(false);
  }
  // The rest, in the order the results come back: a net's pieces that are
  // back are written while another net's are still on the device (the small
  // variant nets' usually are back first); the host blocks only when a
  // single net is left.
  uint32_t idle_polls = 0;
  while (rc == FNNUE_OK) {
    bool progress = false;
    int first = -1, left = 0;
    for (int k = 0; k < kKinds && rc == FNNUE_OK; ++k) {
      NetWork& W = net[k];
      while (rc == FNNUE_OK && W.next < W.pieces.size()) {
        bool ready = false;
        rc = finish(j, k, false, &ready);
        if (!ready) break;
        progress = true;
      }
      if (W.next < W.pieces.size()) {
        ++left;
        if (first < 0) first = k;
      }
    }
    if (rc || !left) break;
    if (progress) continue;
    if (left == 1 || !any_order) {
      bool ready = false;
      rc = finish(j, first, true, &ready);
    } else {  // polling counts as waiting for the device; a long wait yields the CPU
      const auto tw = Clock::now();
      if (++idle_polls < 256) {
        for (int i = 0; i < 64; ++i) _mm_pause();
      } else {
        sched_yield();
      }
      wait_ms += ms_since(tw);
      if (expired()) rc = timed_out("waiting for the nets' pieces");
    }
    if (progress) idle_polls = 0;
  }
  if (rc == FNNUE_E_TIMEOUT) {
    // The device may still be running this call's pieces, which read and
    // write the channel's pinned buffers: nothing waits for them; the channel
    // is broken (later calls fail fast, fnnue_backend_free reclaims the
    // buffers once the streams have drained).
    abandon_unanswered(j);
    // the answers that need no device (roots without a legal move, batches
    // whose every position is skipped) are written: they are valid
    fill_hostonly(j, all_skipped);
    close_lines(j);
    j.ret = rc;
    j.err = g_err;
    return;
  }
  if (rc) {
    const std::string err = g_err;
    drain_streams();
    j.ret = rc;
    j.err = err;
    return;
  }
  fill_hostonly(j, all_skipped);
  close_lines(j);
  uint32_t npieces = 0;
  for (const NetWork& W : net) npieces += (uint32_t)W.pieces.size();
  j.ret = FNNUE_OK;
  mark("done");
  if (trace) std::fprintf(stderr, "FNNUE_BACKEND_TRACE {\"batches\":%zu,\"marks\":[%s]}\n", nb, tl.c_str());
  std::lock_guard<std::mutex> lk(stats_mu);
  stats.total_ms = ms_since(t0);
  stats.fill_ms = fill_ms;
  stats.device_ms = wait_ms;
  stats.prep_ms = stats.total_ms - fill_ms - wait_ms;
  stats.positions = filled;
  stats.stream_syncs = syncs;
  stats.rebuilds = rebuilds;
  stats.host_threads = pool_threads;
  stats.pieces = npieces;
}

namespace {
void reap_abandoned() {
  std::vector<fnnue_backend*> done;
  {
    std::lock_guard<std::mutex> lk(g_abandoned_mu);
    for (size_t i = 0; i < g_abandoned.size();) {
      fnnue_backend* b = g_abandoned[i];
      DeviceGuard g(b->device);
      if (b->streams_idle()) {
        done.push_back(b);
        g_abandoned[i] = g_abandoned.back();
        g_abandoned.pop_back();
      } else {
        ++i;
      }
    }
  }
  for (fnnue_backend* b : done) {
    DeviceGuard g(b->device);
    b->release_device();
    delete b;
  }
}
}  // namespace

extern "C" {

int fnnue_backend_batch_size(const fnnue_acquired* a, size_t* n) {
  if (!a || !n) return fail(FNNUE_E_ARG, "null argument");
  *n = 0;
  if (a->work == FNNUE_WORK_MOVE) {
    *n = 1;
    return FNNUE_OK;
  }
  if (a->work != FNNUE_WORK_ANALYSIS) return fail(FNNUE_E_ARG, "unknown work type");
  if (a->nskip && !a->skip_positions) return fail(FNNUE_E_ARG, "null skip_positions");
  *n = count_moves(a->moves) + 1;
  return FNNUE_OK;
}

}  // extern "C"

namespace {

// The actor over one net per slot (slot k: a net of variant k, or null).
int channel_slots(const fnnue_net* const (&slot)[kKinds], int device, const fnnue_backend_init* init,
                  fnnue_backend** out) {
  if (init && init->normalize_to_pawn < 0) return fail(FNNUE_E_ARG, "normalize_to_pawn must be positive");
  reap_abandoned();
  fnnue_backend* b = nullptr;
  try {
    b = new fnnue_backend();
  } catch (const std::bad_alloc&) {
    return fail(FNNUE_E_OOM, "host allocation failed");
  }
  b->device = device;
  if (init && init->normalize_to_pawn > 0) b->norm = init->normalize_to_pawn;
  if (init && init->timeout_ms > 0) b->timeout_ms = init->timeout_ms;
  {
    // host threads for the text staging and response fill of large calls: up
    // to 8, at most the CPUs this process may run on (12 or 16: within the
    // box-to-box noise at 16384 batches per call, slower at 1024,
    // profiles/r05/backend_threads/)
    int nt = std::min(8, usable_cpus());
    if (const char* e = std::getenv("FNNUE_BACKEND_THREADS")) nt = std::max(1, std::min(64, std::atoi(e)));
    b->pool_threads = nt;
    b->trace = std::getenv("FNNUE_BACKEND_TRACE") != nullptr;
    if (const char* e = std::getenv("FNNUE_BACKEND_PIECE_PLIES")) b->piece_plies = (size_t)std::max(1024L, std::atol(e));
    if (const char* e = std::getenv("FNNUE_BACKEND_ANY_ORDER")) b->any_order = std::atoi(e) != 0;
    if (const char* e = std::getenv("FNNUE_BACKEND_TAIL_PLIES")) b->tail_plies = (size_t)std::max(0L, std::atol(e));
    if (const char* e = std::getenv("FNNUE_BACKEND_FILL_GRAIN")) b->fill_grain = (size_t)std::max(1L, std::atol(e));
    if (const char* e = std::getenv("FNNUE_BACKEND_SIZE_GRAIN")) b->size_grain = (size_t)std::max(1L, std::atol(e));
    if (const char* e = std::getenv("FNNUE_BACKEND_STAGE_GRAIN")) b->stage_grain = (size_t)std::max(1L, std::atol(e));
  }
  for (int k = 0; k < kKinds; ++k) {
    if (!slot[k]) continue;
    if (int rc = fnnue_ctx_create(slot[k], device, &b->ctx[k])) {
      for (fnnue_ctx* c : b->ctx) fnnue_ctx_free(c);
      delete b;
      return rc;
    }
  }
  try {
    b->pool.start(b->pool_threads);
  } catch (const std::system_error&) {
    b->pool.stop();
    for (fnnue_ctx* c : b->ctx) fnnue_ctx_free(c);
    delete b;
    return fail(FNNUE_E_OOM, "could not start the host worker threads");
  }
  *out = b;
  return FNNUE_OK;
}

}  // namespace

extern "C" {

int fnnue_backend_channel_nets(const fnnue_backend_nets* nets, int device, const fnnue_backend_init* init,
                               fnnue_backend** out) {
  if (!nets || !out) return fail(FNNUE_E_ARG, "null argument");
  *out = nullptr;
  const fnnue_net* slot[kKinds] = {nets->chess, nets->crazyhouse, nets->atomic};
  if (!slot[0] && !slot[1] && !slot[2]) return fail(FNNUE_E_ARG, "no net");
  static const char* const kName[3] = {"chess (HalfKAv2_hm)", "crazyhouse", "atomic"};
  for (int k = 0; k < 3; ++k) {
    if (!slot[k]) continue;
    int variant = -1;
    if (int rc = fnnue_net_variant(slot[k], &variant)) return rc;
    if (variant != k) return fail(FNNUE_E_ARCH, std::string("the ") + kName[k] + " slot needs a " + kName[k] + " net");
  }
  return channel_slots(slot, device, init, out);
}

int fnnue_backend_channel_netv(const fnnue_net* const* nets, size_t n, int device, const fnnue_backend_init* init,
                               fnnue_backend** out) {
  if (!nets || !out) return fail(FNNUE_E_ARG, "null argument");
  *out = nullptr;
  if (n == 0) return fail(FNNUE_E_ARG, "no net");
  const fnnue_net* slot[kKinds] = {};
  for (size_t i = 0; i < n; ++i) {
    int variant = -1;
    if (!nets[i]) return fail(FNNUE_E_ARG, "null net");
    if (int rc = fnnue_net_variant(nets[i], &variant)) return rc;
    if (!variant_known(variant)) return fail(FNNUE_E_ARCH, "a net of unknown variant " + std::to_string(variant));
    if (slot[variant]) return fail(FNNUE_E_ARG, std::string("two ") + variant_name(variant) + " nets");
    slot[variant] = nets[i];
  }
  return channel_slots(slot, device, init, out);
}

int fnnue_backend_channel(const fnnue_net* net, int device, const fnnue_backend_init* init, fnnue_backend** out) {
  if (!net || !out) return fail(FNNUE_E_ARG, "null argument");
  return fnnue_backend_channel_netv(&net, 1, device, init, out);
}

void fnnue_backend_free(fnnue_backend* b) {
  if (!b) return;
  {
    std::lock_guard<std::mutex> lk(b->run_mu);  // after the call in flight
    b->closed = true;
  }
  b->pool.stop();
  {
    DeviceGuard g(b->device);
    if (b->broken && !b->streams_idle()) {
      // A timed-out call's pieces are still on the device: freeing their
      // buffers (or the contexts) would wait for them.  The backend is parked
      // and released by a later channel() / free() once its streams drain.
      std::lock_guard<std::mutex> lk(g_abandoned_mu);
      g_abandoned.push_back(b);
      return;
    }
    b->release_device();
  }
  delete b;
  reap_abandoned();
}

namespace {
int go_job(fnnue_backend* b, Job& j, const fnnue_acquired* batches, size_t nbatches, size_t cap, uint32_t* off,
           int32_t* batch_rc, uint32_t timeout_ms) {
  j.batches = batches;
  j.nb = nbatches;
  j.cap = cap;
  j.off = off;
  j.rc = batch_rc;
  j.timeout_ms = timeout_ms;
  std::lock_guard<std::mutex> lk(b->run_mu);  // mpsc::Sender::send on a full channel waits
  if (b->closed) return fail(FNNUE_E_DEVICE, "backend actor stopped");
  if (b->broken) {
    for (size_t i = 0; i < nbatches; ++i) batch_rc[i] = FNNUE_E_TIMEOUT;
    return fail(FNNUE_E_TIMEOUT, "the channel is broken: an earlier go() overran its budget (open a new channel)");
  }
  DeviceGuard g(b->device);
  g_err.clear();
  b->run(j);
  if (j.ret) return fail(j.ret, j.err);
  return FNNUE_OK;
}
}  // namespace

int fnnue_backend_go_timeout(fnnue_backend* b, const fnnue_acquired* batches, size_t nbatches,
                             fnnue_position_response* out, size_t cap, uint32_t* off, int32_t* batch_rc,
                             uint32_t timeout_ms) {
  if (!b || !off || !batch_rc || (nbatches && !batches) || (cap && !out)) return fail(FNNUE_E_ARG, "null argument");
  if (nbatches > (1u << 24)) return fail(FNNUE_E_ARG, "too many batches");
  Job j;
  j.out = out;
  return go_job(b, j, batches, nbatches, cap, off, batch_rc, timeout_ms);
}

int fnnue_backend_go_compact(fnnue_backend* b, const fnnue_acquired* batches, size_t nbatches,
                             fnnue_position_compact* out, size_t cap, fnnue_batch_compact* bout, uint32_t* off,
                             int32_t* batch_rc, uint32_t timeout_ms) {
  if (!b || !off || !batch_rc || (nbatches && (!batches || !bout)) || (cap && !out))
    return fail(FNNUE_E_ARG, "null argument");
  if (nbatches > (1u << 24)) return fail(FNNUE_E_ARG, "too many batches");
  if (b->norm < 13) return fail(FNNUE_E_ARG, "compact results need normalize_to_pawn >= 13 (32-bit scores)");
  Job j;
  j.cout = out;
  j.bout = bout;
  return go_job(b, j, batches, nbatches, cap, off, batch_rc, timeout_ms);
}

int fnnue_backend_lines_bound(const fnnue_acquired* batches, size_t nbatches, size_t* n) {
  if (!n || (nbatches && !batches)) return fail(FNNUE_E_ARG, "null argument");
  size_t total = 0;
  for (size_t i = 0; i < nbatches; ++i)
    if (const uint32_t kk = line_slots(batches[i])) total += (count_moves(batches[i].moves) + 1) * kk;
  *n = total;
  return FNNUE_OK;
}

int fnnue_backend_go_lines(fnnue_backend* b, const fnnue_acquired* batches, size_t nbatches,
                           fnnue_position_response* out, size_t cap, uint32_t* off, int32_t* batch_rc,
                           fnnue_pv_line* lines, size_t lines_cap, uint32_t* line_off, uint32_t timeout_ms) {
  if (!b || !off || !batch_rc || !line_off || (nbatches && !batches) || (cap && !out) || (lines_cap && !lines))
    return fail(FNNUE_E_ARG, "null argument");
  if (nbatches > (1u << 24)) return fail(FNNUE_E_ARG, "too many batches");
  size_t bound = 0;
  if (int rc = fnnue_backend_lines_bound(batches, nbatches, &bound)) return rc;
  if (bound > UINT32_MAX) return fail(FNNUE_E_ARG, "the batches ask for more than 2^32 - 1 lines");
  if (lines_cap < bound)
    return fail(FNNUE_E_CAPACITY, "line buffer holds " + std::to_string(lines_cap) + ", batches may need " +
                                      std::to_string(bound));
  fnnue_pv_line none;  // a call that can have no line still runs as a go_lines() call
  Job j;
  j.out = out;
  j.lines = lines ? lines : &none;
  j.line_off = line_off;
  return go_job(b, j, batches, nbatches, cap, off, batch_rc, timeout_ms);
}

int fnnue_backend_go_lines_pv(fnnue_backend* b, const fnnue_acquired* batches, size_t nbatches,
                              fnnue_position_response* out, size_t cap, uint32_t* off, int32_t* batch_rc,
                              fnnue_pv_line2* lines, size_t lines_cap, uint32_t* line_off, fnnue_move* reply,
                              uint32_t timeout_ms) {
  if (!b || !off || !batch_rc || !line_off || (nbatches && !batches) || (cap && !out) || (lines_cap && !lines))
    return fail(FNNUE_E_ARG, "null argument");
  if (nbatches > (1u << 24)) return fail(FNNUE_E_ARG, "too many batches");
  size_t bound = 0;
  if (int rc = fnnue_backend_lines_bound(batches, nbatches, &bound)) return rc;
  if (bound > UINT32_MAX) return fail(FNNUE_E_ARG, "the batches ask for more than 2^32 - 1 lines");
  if (lines_cap < bound)
    return fail(FNNUE_E_CAPACITY, "line buffer holds " + std::to_string(lines_cap) + ", batches may need " +
                                      std::to_string(bound));
  fnnue_pv_line2 none;  // a call that can have no line still runs as a go_lines_pv() call
  Job j;
  j.out = out;
  j.lines2 = lines ? lines : &none;
  j.line_off = line_off;
  j.reply = reply;
  return go_job(b, j, batches, nbatches, cap, off, batch_rc, timeout_ms);
}

int fnnue_backend_go_pv(fnnue_backend* b, const fnnue_acquired* batches, size_t nbatches, fnnue_position_response* out,
                        size_t cap, uint32_t* off, int32_t* batch_rc, fnnue_move* reply, uint32_t timeout_ms) {
  if (!b || !off || !batch_rc || (nbatches && !batches) || (cap && (!out || !reply)))
    return fail(FNNUE_E_ARG, "null argument");
  if (nbatches > (1u << 24)) return fail(FNNUE_E_ARG, "too many batches");
  Job j;
  j.out = out;
  j.reply = reply;
  return go_job(b, j, batches, nbatches, cap, off, batch_rc, timeout_ms);
}

int fnnue_backend_go(fnnue_backend* b, const fnnue_acquired* batches, size_t nbatches, fnnue_position_response* out,
                     size_t cap, uint32_t* off, int32_t* batch_rc) {
  return fnnue_backend_go_timeout(b, batches, nbatches, out, cap, off, batch_rc, 0);
}

int fnnue_backend_set_analysis_depth(fnnue_backend* b, int depth) {
  if (!b) return fail(FNNUE_E_ARG, "null argument");
  if (depth != 0 && depth != 1) return fail(FNNUE_E_ARG, "analysis depth 0 or 1, not " + std::to_string(depth));
  std::lock_guard<std::mutex> lk(b->run_mu);  // after the call in flight
  b->analysis_depth = depth;
  return FNNUE_OK;
}

int fnnue_backend_set_analysis_plies(fnnue_backend* b, int plies) {
  if (!b) return fail(FNNUE_E_ARG, "null argument");
  if (plies < 0 || plies > 2) return fail(FNNUE_E_ARG, "analysis plies 0, 1 or 2, not " + std::to_string(plies));
  std::lock_guard<std::mutex> lk(b->run_mu);  // after the call in flight
  b->analysis_depth = plies;
  return FNNUE_OK;
}

int fnnue_backend_set_draw_rules(fnnue_backend* b, int on) {
  if (!b) return fail(FNNUE_E_ARG, "null argument");
  std::lock_guard<std::mutex> lk(b->run_mu);  // after the call in flight
  b->draw_rules = on != 0;
  return FNNUE_OK;
}

int fnnue_backend_set_quiesce(fnnue_backend* b, int depth) {
  if (!b) return fail(FNNUE_E_ARG, "null argument");
  if (depth < 0 || depth > FNNUE_QUIESCE_MAX)
    return fail(FNNUE_E_ARG, "quiescence depth must be 0.." + std::to_string(FNNUE_QUIESCE_MAX));
  std::lock_guard<std::mutex> lk(b->run_mu);  // after the call in flight
  b->quiesce = depth;
  return FNNUE_OK;
}

int fnnue_backend_quiesce(fnnue_backend* b, int* depth) {
  if (!b || !depth) return fail(FNNUE_E_ARG, "null argument");
  std::lock_guard<std::mutex> lk(b->run_mu);
  *depth = b->quiesce;
  return FNNUE_OK;
}

int fnnue_backend_set_quiesce_checks(fnnue_backend* b, int on) {
  if (!b) return fail(FNNUE_E_ARG, "null argument");
  std::lock_guard<std::mutex> lk(b->run_mu);  // after the call in flight
  b->quiesce_checks = on != 0;
  return FNNUE_OK;
}

int fnnue_backend_quiesce_checks(fnnue_backend* b, int* on) {
  if (!b || !on) return fail(FNNUE_E_ARG, "null argument");
  std::lock_guard<std::mutex> lk(b->run_mu);
  *on = b->quiesce_checks ? 1 : 0;
  return FNNUE_OK;
}

int fnnue_backend_set_variant_quiesce(fnnue_backend* b, int depth, int checks) {
  if (!b) return fail(FNNUE_E_ARG, "null argument");
  if (depth < 0 || depth > FNNUE_QUIESCE_MAX)
    return fail(FNNUE_E_ARG, "quiescence depth must be 0.." + std::to_string(FNNUE_QUIESCE_MAX));
  std::lock_guard<std::mutex> lk(b->run_mu);  // after the call in flight
  b->vquiesce = depth;
  b->vquiesce_checks = checks != 0;
  return FNNUE_OK;
}

int fnnue_backend_variant_quiesce(fnnue_backend* b, int* depth, int* checks) {
  if (!b || !depth || !checks) return fail(FNNUE_E_ARG, "null argument");
  std::lock_guard<std::mutex> lk(b->run_mu);
  *depth = b->vquiesce;
  *checks = b->vquiesce_checks ? 1 : 0;
  return FNNUE_OK;
}

int fnnue_backend_draw_rules(fnnue_backend* b, int* on) {
  if (!b || !on) return fail(FNNUE_E_ARG, "null argument");
  std::lock_guard<std::mutex> lk(b->run_mu);
  *on = b->draw_rules ? 1 : 0;
  return FNNUE_OK;
}

int fnnue_backend_set_variant_draw_rules(fnnue_backend* b, int on) {
  if (!b) return fail(FNNUE_E_ARG, "null argument");
  std::lock_guard<std::mutex> lk(b->run_mu);  // after the call in flight
  b->variant_draw_rules = on != 0;
  return FNNUE_OK;
}

int fnnue_backend_variant_draw_rules(fnnue_backend* b, int* on) {
  if (!b || !on) return fail(FNNUE_E_ARG, "null argument");
  std::lock_guard<std::mutex> lk(b->run_mu);
  *on = b->variant_draw_rules ? 1 : 0;
  return FNNUE_OK;
}

int fnnue_backend_set_variant_analysis_depth(fnnue_backend* b, int depth) {
  if (!b) return fail(FNNUE_E_ARG, "null argument");
  if (depth != 0 && depth != 1) return fail(FNNUE_E_ARG, "variant analysis depth 0 or 1, not " + std::to_string(depth));
  std::lock_guard<std::mutex> lk(b->run_mu);  // after the call in flight
  b->variant_analysis_depth = depth;
  return FNNUE_OK;
}

int fnnue_backend_set_variant_analysis_plies(fnnue_backend* b, int plies) {
  if (!b) return fail(FNNUE_E_ARG, "null argument");
  if (plies < 0 || plies > 2)
    return fail(FNNUE_E_ARG, "variant analysis plies 0, 1 or 2, not " + std::to_string(plies));
  std::lock_guard<std::mutex> lk(b->run_mu);  // after the call in flight
  b->variant_analysis_depth = plies;
  return FNNUE_OK;
}

int fnnue_backend_last_stats(fnnue_backend* b, fnnue_backend_stats* out) {
  if (!b || !out) return fail(FNNUE_E_ARG, "null argument");
  std::lock_guard<std::mutex> lk(b->stats_mu);
  *out = b->stats;
  return FNNUE_OK;
}

}  // extern "C"

namespace {
// Both JSON forms: without `lines` every response has its own one line.
int analysis_json(const fnnue_position_response* r, size_t n, const fnnue_pv_line* lines, const uint32_t* line_off,
                  char* buf, size_t cap, size_t* len, const fnnue_move* reply = nullptr,
                  const fnnue_pv_line2* lines2 = nullptr) {
  std::string s = "[";
  char tmp[192];
  for (size_t i = 0; i < n; ++i) {
    if (i) s += ',';
    if (r[i].skipped) {
      s += "{\"skipped\":true}";
      continue;
    }
    // AnalysisPart::Best: pv omitted when empty, nps omitted when None.
    // AnalysisPart::Matrix: pv / score matrices [multipv - 1][depth]; static
    // eval fills multipv 1 at depth 0 with an empty pv.
    const char* kind = r[i].score_kind == FNNUE_SCORE_MATE ? "mate" : "cp";
    // The pv is the best move (a one-ply search has no second one): Best omits
    // an empty pv; Matrix::set puts its line at column `depth`, the columns
    // before it null ([ref] src/ipc.rs:77-86).
    char pv[8];
    std::memcpy(pv, r[i].best_move, 8);
    pv[7] = 0;
    for (char* c = pv; *c; ++c)
      if (*c == '"' || *c == '\\' || (unsigned char)*c < 0x20) *c = '?';  // never from this library
    // the pv's second move (fnnue_backend_go_pv): only behind a first one
    char pv2[8] = {0};
    // a variant's reply may be a drop ("N@f3"); every chess code prints as fnnue_move_uci prints it
    if (reply && reply[i] && pv[0] && fnnue_vmove_uci(reply[i], pv2) != FNNUE_OK) pv2[0] = 0;
    const size_t nl = line_off && r[i].matrix ? line_off[i + 1] - line_off[i] : 0;  // lines are rows of the matrix form
    if (nl) {
      // Matrix::set per line: row l is `depth` nulls and then the entry
      const fnnue_pv_line* L = lines ? lines + (line_off[i] - line_off[0]) : nullptr;
      const fnnue_pv_line2* L2 = lines2 ? lines2 + (line_off[i] - line_off[0]) : nullptr;
      std::string nulls;
      for (unsigned d = 0; d < r[i].depth; ++d) nulls += "null,";
      s += "{\"pv\":[";
      for (size_t l = 0; l < nl; ++l) {
        // the line's own pv: one move (fnnue_pv_line), or one or two separated by a space (fnnue_pv_line2)
        char mv[16] = {0};
        if (L2) std::memcpy(mv, L2[l].pv, sizeof(L2[l].pv) - 1);
        else std::memcpy(mv, L[l].move, 6);
        std::string entry;
        for (char* c = mv; *c; ++c) {
          if (*c == '"' || *c == '\\' || (unsigned char)*c < 0x20) *c = '?';
          if (*c == ' ') entry += "\",\"";
          else entry += *c;
        }
        s += (l ? ",[" : "[") + nulls + (mv[0] ? "[\"" + entry + "\"]" : std::string("[]")) + "]";
      }
      s += "],\"score\":[";
      for (size_t l = 0; l < nl; ++l) {
        std::snprintf(tmp, sizeof(tmp), "{\"%s\":%lld}]",
                      (L2 ? L2[l].score_kind : L[l].score_kind) == FNNUE_SCORE_MATE ? "mate" : "cp",
                      (long long)(L2 ? L2[l].score : L[l].score));
        s += (l ? ",[" : "[") + nulls + tmp;
      }
      std::snprintf(tmp, sizeof(tmp), "],\"depth\":%u,\"nodes\":%llu,\"time\":%llu", (unsigned)r[i].depth,
                    (unsigned long long)r[i].nodes, (unsigned long long)r[i].time_ms);
    } else if (r[i].matrix) {
      s += "{\"pv\":[[";
      for (unsigned d = 0; d < r[i].depth; ++d) s += "null,";
      s += pv[0] ? std::string("[\"") + pv + (pv2[0] ? std::string("\",\"") + pv2 : std::string()) + "\"]"
                 : std::string("[]");
      s += "]],\"score\":[[";
      for (unsigned d = 0; d < r[i].depth; ++d) s += "null,";
      std::snprintf(tmp, sizeof(tmp), "{\"%s\":%lld}]],\"depth\":%u,\"nodes\":%llu,\"time\":%llu", kind,
                    (long long)r[i].score, (unsigned)r[i].depth, (unsigned long long)r[i].nodes,
                    (unsigned long long)r[i].time_ms);
    } else {
      if (pv[0]) s += std::string("{\"pv\":\"") + pv + (pv2[0] ? std::string(" ") + pv2 : std::string()) + "\",";
      else s += '{';
      std::snprintf(tmp, sizeof(tmp), "\"score\":{\"%s\":%lld},\"depth\":%u,\"nodes\":%llu,\"time\":%llu", kind,
                    (long long)r[i].score, (unsigned)r[i].depth, (unsigned long long)r[i].nodes,
                    (unsigned long long)r[i].time_ms);
    }
    s += tmp;
    if (r[i].nps) {
      std::snprintf(tmp, sizeof(tmp), ",\"nps\":%u", r[i].nps);
      s += tmp;
    }
    s += '}';
  }
  s += ']';
  *len = s.size();
  if (cap < s.size() + 1) {
    if (cap) buf[0] = 0;
    return fail(FNNUE_E_CAPACITY, "JSON buffer too small");
  }
  std::memcpy(buf, s.c_str(), s.size() + 1);
  return FNNUE_OK;
}
}  // namespace

extern "C" {

int fnnue_backend_analysis_json(const fnnue_position_response* r, size_t n, char* buf, size_t cap, size_t* len) {
  if ((n && !r) || !len || (cap && !buf)) return fail(FNNUE_E_ARG, "null argument");
  return analysis_json(r, n, nullptr, nullptr, buf, cap, len);
}

int fnnue_backend_analysis_json_pv(const fnnue_position_response* r, size_t n, const fnnue_move* reply, char* buf,
                                   size_t cap, size_t* len) {
  if ((n && !r) || !len || (cap && !buf)) return fail(FNNUE_E_ARG, "null argument");
  return analysis_json(r, n, nullptr, nullptr, buf, cap, len, reply);
}

int fnnue_backend_analysis_json_lines(const fnnue_position_response* r, size_t n, const fnnue_pv_line* lines,
                                      const uint32_t* line_off, char* buf, size_t cap, size_t* len) {
  if ((n && !r) || !line_off || !len || (cap && !buf)) return fail(FNNUE_E_ARG, "null argument");
  if (line_off[n] != line_off[0] && !lines) return fail(FNNUE_E_ARG, "null argument");
  for (size_t i = 0; i < n; ++i)
    if (line_off[i] > line_off[i + 1]) return fail(FNNUE_E_ARG, "line offsets decrease");
  return analysis_json(r, n, lines, line_off, buf, cap, len);
}

int fnnue_backend_analysis_json_lines_pv(const fnnue_position_response* r, size_t n, const fnnue_pv_line2* lines,
                                         const uint32_t* line_off, char* buf, size_t cap, size_t* len) {
  if ((n && !r) || !line_off || !len || (cap && !buf)) return fail(FNNUE_E_ARG, "null argument");
  if (line_off[n] != line_off[0] && !lines) return fail(FNNUE_E_ARG, "null argument");
  for (size_t i = 0; i < n; ++i)
    if (line_off[i] > line_off[i + 1]) return fail(FNNUE_E_ARG, "line offsets decrease");
  return analysis_json(r, n, nullptr, line_off, buf, cap, len, nullptr, lines);
}

}  // extern "C"
