// builder.h — device-side batch builder (builder.hip): FEN parse, UCI replay
// and legal children on the GPU.  Same semantics as the host builder
// (board.h / board.cpp), which the tests hold it to record for record.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <vector>

#include "../../include/fnnue.h"
#include "board.h"

namespace fnnue {

__host__ __device__ inline int make_piece_d(int c, int pt) { return (c << 3) | pt; }

// Board state a ply needs for move generation: bitboards, castling rooks,
// en-passant square, side to move.  The small fields are whole 32-bit words
// (the replay's board chain runs on the scalar unit, which has no 8- or
// 16-bit compares): castling rook of [colour c][side s] (0 king side, 1 queen
// side) in byte 2c + s of `cr`, 0xFF none (accessors in builder.hip).
struct DBoard {
  uint64_t bc[2];   // by colour
  uint64_t bt[7];   // by piece type (1..6); [0]: threecheck's remaining checks (vboard.h checks_word), else 0
  uint32_t cr;
  int32_t ep;
  uint32_t stm;
  uint32_t c960;    // castling rights need Chess960 notation (non-standard rook/king files)
};

DBoard to_dboard(const Board& b);

// kBuildErrCount: a game's move tokens differ from the count its offsets were
// sized for (the host's count; never for offsets from the builder's own count).
constexpr uint32_t kBuildErrFen = 1, kBuildErrMove = 2, kBuildErrCount = 3;

// State of a game's last position (optional builder output, one byte per
// game): a game that ended on the board ends there, since no move can follow.
// The engine answers such a root with `bestmove (none)` and `score mate 0`
// (checkmated, or atomic: its king exploded) or `score cp 0` (stalemate)
// ([ref] src/stockfish.rs:359-376 parses them to Score::Mate(0) / Cp(0)).
constexpr uint8_t kFinalNoMoves = 1, kFinalCheck = 2, kFinalExtinct = 4;
// The game was decided by the variant's own rule (kingofthehill: a king on the
// hill; racingkings: one king on rank 8; threecheck: a check counter at 0):
// `score mate 0`.  (The racingkings
// draw with both kings on rank 8 is kFinalNoMoves alone.)
constexpr uint8_t kFinalVariant = 8;
// On a child only (move work, the variant one-ply search): the decided game is
// won by its side to move (racingkings: black missed its catch-up move), so
// the parent's mover lost by playing it.
constexpr uint8_t kFinalWon = 0x40;
// On a searched record only (draws.hip): drawn by repetition or the fifty-move
// rule with the game before the root counted; ranks as kFinalNoMoves alone.
constexpr uint8_t kFinalDraw = 0x10;
static_assert(kFinalNoMoves == FNNUE_END_NO_MOVES && kFinalVariant == FNNUE_END_VARIANT &&
                  kFinalWon == FNNUE_END_WON && kFinalDraw == FNNUE_END_DRAW,
              "fnnue.h FNNUE_END_*");
// A game the replay rejected: kFinalFailed | its kBuildErr* code (replay_games_device).
constexpr uint8_t kFinalFailed = 0x80;

struct BuildResult {
  hipError_t hip = hipSuccess;
  bool capacity = false;   // outputs too small: n_out / n_groups say what is needed
  size_t n_out = 0, n_groups = 0;
  uint32_t err_code = 0, err_game = 0, err_ply = 0;  // kBuildErr*: first failing game, ply (1-based move)
};

// Grow-only device scratch of the batch builder (one per context, one per
// backend): per-game ply counts and offsets, the error word, the scan's
// temporary storage, per-ply boards and children counts.  A steady stream of
// batches allocates nothing; buffers are freed by release() only.
struct BuilderScratch {
  enum {
    kPlies, kPlyOff, kErr, kScan, kStates, kCnt, kCoff,
    kKids, kKidMoves, kKidEnd, kKidPsqt, kKidPositional,  // the one-ply search's children and their evaluation
    // the two-ply search: the children's boards, counts, STAR offsets and depth-1 records (whole call), the
    // plies' spans in them, then one chunk's offsets, grandchild records, moves, end flags and terms
    kKidStates, kKidCnt, kKidOff, kKidBest, kPlySpans, kChunkOff, kGrand, kGrandMoves, kGrandEnd, kGrandPsqt,
    kGrandPositional,
    // the draw rules (draws.hip): per game its root clock, per ply its key, window start and history, the list
    kDrawClock0, kDrawKeys, kDrawLo, kDrawHist, kDrawList,
    // capture quiescence (quiesce.hip): the roots (boards, their records in the leaves' arrays, which of them are
    // searched, their results), one level's temporaries, then per level (FNNUE_QUIESCE_MAX slots each) the nodes'
    // record offsets and group numbers, the records' moves, the children's results and boards
    kQRoots, kQMap, kQActive, kQRes0, kQCnt, kQHas, kQGoff, kQPos, kQPsqt, kQPositional,
    kQRoff, kQGidx = kQRoff + FNNUE_QUIESCE_MAX, kQMoves = kQGidx + FNNUE_QUIESCE_MAX,
    kQRes = kQMoves + FNNUE_QUIESCE_MAX, kQBoards = kQRes + FNNUE_QUIESCE_MAX,
    kQEnd = kQBoards + FNNUE_QUIESCE_MAX,
    // quiescence checks (ABI 3.14): per level the nodes' flag bytes (in check / mated), the trace's counters
    kQFlag = kQEnd, kQEvasions = kQFlag + FNNUE_QUIESCE_MAX,
    kSlots
  };
  void* p[kSlots] = {};
  size_t bytes[kSlots] = {};
  // p[slot] with at least `want` bytes (grows by a quarter beyond the request)
  hipError_t get(int slot, size_t want, void** out);
  void release();
};

// text: game g's FEN in [fen_off[g], mv_off[g]), its space-separated UCI moves
// in [mv_off[g], fen_off[g + 1]).  children = false: every ply of every game,
// group g = game g; children = true: one group per ply = the ply's position
// followed by its legal children (Board::legal_moves order).  d_final
// (optional, ngames bytes): kFinal* flags of each game's last position.
// Sizes the outputs on the device and reads the sizes back: synchronises `s`.
//
// The one-ply search's form of the children expansion: with d_moves / d_end
// (both, children only; cap entries each) every record also gets the move that
// leads to it (fnnue_move; 0 for a ply's own record) and its own kFinalNoMoves /
// kFinalCheck flags.  With `own` the outputs live in the scratch instead (d_out,
// d_group_off, d_moves, d_end ignored; no capacity but own->max_groups plies,
// checked before any ply is expanded) and `own` says where.
struct ChildrenBufs {
  size_t max_groups = 0;            // in: plies the caller has room for
  fnnue_pos* pos = nullptr;         // out: records, group offsets (plies + 1), moves, end flags
  const uint32_t* off = nullptr;
  uint16_t* moves = nullptr;
  uint8_t* end = nullptr;
  const uint32_t* ply_off = nullptr;  // out: each game's first ply (ngames + 1)
};
BuildResult build_batch_device(const char* d_text, const uint32_t* d_fen_off, const uint32_t* d_mv_off,
                               uint32_t ngames, bool children, fnnue_pos* d_out, size_t cap, uint32_t* d_group_off,
                               size_t off_cap, hipStream_t s, BuilderScratch& ws, uint8_t* d_final = nullptr,
                               uint16_t* d_moves = nullptr, uint8_t* d_end = nullptr, ChildrenBufs* own = nullptr);

// The two halves of the children expansion over boards already replayed (the
// backend's pieces): sizes (cnt and off: n + 1 words each; off[n] = records),
// then the records with their moves and end flags.  Stream-ordered, no sync.
hipError_t children_count_device(const DBoard* d_states, uint32_t n, uint32_t* d_cnt, uint32_t* d_off, hipStream_t s,
                                 BuilderScratch& ws);
hipError_t children_write_device(const DBoard* d_states, uint32_t n, const uint32_t* d_off, uint32_t total,
                                 fnnue_pos* d_out, uint16_t* d_moves, uint8_t* d_end, hipStream_t s);
// Two forms of children_write_device, same output: one thread per record, each
// regenerating its ply's moves up to its own (1, the default: as fast as the
// other on 400k plies and three times faster on the backend's pieces), or one
// thread per ply (0).  FNNUE_CHILDREN_IMPL=ply|record in the environment picks
// one (measurements: DESIGN.md §4.14).
int children_impl();

// The two-ply search's child states: the boards of the children of n plies'
// STAR groups (d_off: n + 1 offsets, total = d_off[n] records) as a dense array
// in record order, the plies' own records skipped: child j (1-based) of ply i
// is entry d_off[i] - i + j - 1, total - n entries in all.  d_map (optional):
// entry -> (ply, child index).  children_count_device / children_write_device
// expand the array like any other.  Stream-ordered, no sync.
hipError_t child_states_device(const DBoard* d_states, uint32_t n, const uint32_t* d_off, uint32_t total,
                               DBoard* d_out, uint2* d_map, hipStream_t s);
// Per ply p in 0..n: d_first_child[p] = d_off[p] - p, d_first_rec[p] =
// d_kid_off[d_first_child[p]] (the children's STAR offsets): what the host
// needs to cut the plies into chunks of bounded grandchild records.
hipError_t ply_spans_device(const uint32_t* d_off, const uint32_t* d_kid_off, uint32_t n, uint32_t* d_first_child,
                            uint32_t* d_first_rec, hipStream_t s);
// d_dst[i] = d_src[i] - d_src[0], i < n: a chunk's offsets from the whole array's.
hipError_t rebase_offsets_device(const uint32_t* d_src, uint32_t n, uint32_t* d_dst, hipStream_t s);

// The replay alone, into the scratch: every ply's board (kStates: DBoard for
// kVariantChess, vstate_bytes(variant) each for a variant) and the games' ply
// offsets (kPlyOff, ngames + 1).  More than max_plies plies: capacity, with
// n_out = the plies, before any is replayed.  Synchronises `s` (sizes, errors).
BuildResult replay_states_device(int variant, const char* d_text, const uint32_t* d_fen_off, const uint32_t* d_mv_off,
                                 uint32_t ngames, size_t max_plies, hipStream_t s, BuilderScratch& ws,
                                 const void** d_states, const uint32_t** d_ply_off);

// ---- draws.hip: repetition and fifty-move draws (include/fnnue.h, ABI 3.12; the variants: 3.16) ----
// The history of n plies (game_history_device, search_steps.h) in the scratch:
// per ply its fnnue_ply_history, its 63-bit identity key (bit 63: the move that
// led to it was irreversible), the first ply of its window (the last
// irreversible move, or the game's root; crazyhouse: always the root), and the
// compacted list of the plies with a descendant that can be drawn at all
// (list[0] = their number).
struct DrawHistory {
  const fnnue_ply_history* hist = nullptr;
  const uint64_t* keys = nullptr;
  const uint32_t* lo = nullptr;
  const uint32_t* list = nullptr;
  uint32_t key_bits = 63;
};
uint32_t draw_key_bits();  // FNNUE_DRAW_KEY_BITS in the environment, read per call (tests); 63 without
// A drawn child's own terms (its group's first record) into its depth-1 record,
// behind the first reduction; board-independent.
hipError_t draw_own_terms(const DrawHistory& h, uint32_t p0, uint32_t p1, const uint32_t* d_off, const uint8_t* d_end,
                          const uint32_t* d_kid_off, uint32_t rec0, const int32_t* d_gps, const int32_t* d_gpo,
                          fnnue_best* d_kid_best, hipStream_t s);

// ---- quiesce.hip: capture quiescence below the leaves (include/fnnue.h, ABI 3.13) ----
// What a call did, for FNNUE_SEARCH2_TRACE and the tests: the records of every
// level summed over the slices, and the slices of the root frontier.
struct QuiesceStats {
  uint64_t level_records[FNNUE_QUIESCE_MAX] = {};
  // quiescence checks, with `timed` only: of those records the evasions, and the nodes in check that had one
  uint64_t level_evasions[FNNUE_QUIESCE_MAX] = {};
  uint64_t level_in_check[FNNUE_QUIESCE_MAX] = {};
  uint64_t slices = 0;
  uint64_t redone = 0;  // slices cut down and started again after a level passed the bound
  uint64_t syncs = 0;   // blocking waits for a level's size
  // with `timed` (FNNUE_SEARCH2_TRACE): device time between HIP events, summed over levels and slices, redone
  // work included: the roots' boards and the scatter, generation (count, scans, write), the STAR evaluation,
  // the results' kernels (quiet_leaves, quiet_reduce)
  bool timed = false;
  double roots_ms = 0, gen_ms = 0, eval_ms = 0, reduce_ms = 0;
};
// The most records one level of one slice may hold: FNNUE_QUIESCE_RECORDS in
// the environment, read per call, 16M without and at most (a level's records
// and its children's then stay far below 2^32), at least kQuiesceMinRecords.
// A slice of one root is never cut, whatever its tree holds.
constexpr size_t kQuiesceMinRecords = 256;
size_t quiesce_budget();

// The chess replay with both outputs: the packed plies and their boards.
hipError_t replay_chess_states_device(const char* d_text, const uint32_t* d_fen_off, const uint32_t* d_mv_off,
                                      const uint32_t* d_ply_off, uint32_t ngames, fnnue_pos* d_out, DBoard* d_states,
                                      uint8_t* d_final, uint32_t* d_err, hipStream_t s);

// search1.hip: the STAR-group reduction (fnnue_best_children_device) and the
// gather of each group's first record's terms (the backend's terminal plies).
hipError_t launch_best_children(const int32_t* d_psqt, const int32_t* d_positional, const uint8_t* d_end,
                                const uint16_t* d_moves, const uint32_t* d_off, uint32_t ngroups, uint32_t npos,
                                fnnue_best* d_out, hipStream_t s);
// The same with a childless group's own terms in its record (the two-ply
// search's children: fnnue_best_replies reads them for a one-move pv).
hipError_t launch_best_children_own(const int32_t* d_psqt, const int32_t* d_positional, const uint8_t* d_end,
                                    const uint16_t* d_moves, const uint32_t* d_off, uint32_t ngroups, uint32_t npos,
                                    fnnue_best* d_out, hipStream_t s);
// The second reduction (fnnue_best_replies_device).  d_base: group g's first
// entry in d_child_best (launch_child_counts' d_cnt, ngroups + 1 words, scanned),
// or null when no group is empty: d_off[g] - g.
hipError_t launch_child_counts(const uint32_t* d_off, uint32_t ngroups, uint32_t npos, uint32_t* d_cnt, hipStream_t s);
hipError_t launch_best_replies(const uint8_t* d_end, const uint16_t* d_moves, const uint32_t* d_off, uint32_t ngroups,
                               uint32_t npos, const fnnue_best* d_child_best, const uint32_t* d_base,
                               fnnue_best2* d_out, hipStream_t s);
// The same with the variant ranks (fnnue_vbest_replies_device): FNNUE_END_WON
// children and children whose every reply loses at once.
hipError_t launch_vbest_replies(const uint8_t* d_end, const uint16_t* d_moves, const uint32_t* d_off, uint32_t ngroups,
                                uint32_t npos, const fnnue_best* d_child_best, const uint32_t* d_base,
                                fnnue_best2* d_out, hipStream_t s);
// The k best children of every group as fnnue_line records: group g's slots are
// [d_line_off[g], d_line_off[g + 1]), or [g * uniform_k, (g + 1) * uniform_k)
// when d_line_off is null; nothing is written at or beyond lines_cap.
hipError_t launch_topk_children(const int32_t* d_psqt, const int32_t* d_positional, const uint8_t* d_end,
                                const uint16_t* d_moves, const uint32_t* d_off, uint32_t ngroups, uint32_t npos,
                                const uint32_t* d_line_off, uint32_t uniform_k, fnnue_line* d_lines, size_t lines_cap,
                                hipStream_t s);
// The k best lines of every ply at two plies as fnnue_line2 records: the second
// reduction's inputs and key (vranks: the variants'), launch_topk_children's slots.
hipError_t launch_topk_replies(bool vranks, const uint8_t* d_end, const uint16_t* d_moves, const uint32_t* d_off,
                               uint32_t ngroups, uint32_t npos, const fnnue_best* d_child_best, const uint32_t* d_base,
                               const uint32_t* d_line_off, uint32_t uniform_k, fnnue_line2* d_lines, size_t lines_cap,
                               hipStream_t s);
hipError_t launch_gather_parents(const int32_t* d_psqt, const int32_t* d_positional, const uint32_t* d_off,
                                 uint32_t ngroups, uint32_t npos, int32_t* d_ps_out, int32_t* d_po_out, hipStream_t s);

// Exclusive scan of cnt[0..n) into off[0..n], off[n] = total (hipcub, temporary
// storage from ws); stream-ordered, no host sync.
hipError_t builder_exclusive_scan(const uint32_t* cnt, uint32_t* off, uint32_t n, hipStream_t s, BuilderScratch& ws);

// The same expansion for Fairy-Stockfish variants (vbuilder.hip, vboard.h):
// crazyhouse / atomic FENs and UCI moves (drops "P@e4"), fnnue_vpos records.
// The one-ply search's form, as build_batch_device's: with d_moves / d_end
// every record also gets its move (fnnue_vmove_uci's codes: drops included) and
// its own kFinal* flags under the variant's rules, a child with kFinalWon when
// its side to move has already won; with `own` the outputs live in the scratch.
struct VChildrenBufs {
  size_t max_groups = 0;
  fnnue_vpos* pos = nullptr;
  const uint32_t* off = nullptr;
  uint16_t* moves = nullptr;
  uint8_t* end = nullptr;
  const uint32_t* ply_off = nullptr;
};
BuildResult build_vbatch_device(int variant, const char* d_text, const uint32_t* d_fen_off, const uint32_t* d_mv_off,
                                uint32_t ngames, bool children, fnnue_vpos* d_out, size_t cap, uint32_t* d_group_off,
                                size_t off_cap, hipStream_t s, BuilderScratch& ws, uint8_t* d_final = nullptr,
                                uint16_t* d_moves = nullptr, uint8_t* d_end = nullptr, VChildrenBufs* own = nullptr);
// children_count_device / children_write_device over a variant's boards
// (vstate_bytes(variant) each: DBoard for kingofthehill / racingkings /
// threecheck, vb::VBoard otherwise), one thread per record.  Stream-ordered, no sync.
size_t vstate_bytes(int variant);
hipError_t vchildren_count_device(int variant, const void* d_states, uint32_t n, uint32_t* d_cnt, uint32_t* d_off,
                                  hipStream_t s, BuilderScratch& ws);
hipError_t vchildren_write_device(int variant, const void* d_states, uint32_t n, const uint32_t* d_off, uint32_t total,
                                  fnnue_vpos* d_out, uint16_t* d_moves, uint8_t* d_end, hipStream_t s);
// child_states_device over a variant's boards (vstate_bytes(variant) each, in
// and out; a threecheck child carries its counters): child j of ply i is entry
// d_off[i] - i + j - 1, total - n entries in all.  Stream-ordered, no sync.
hipError_t vchild_states_device(int variant, const void* d_states, uint32_t n, const uint32_t* d_off, uint32_t total,
                                void* d_out, uint2* d_map, hipStream_t s);

// Every ply of every game with offsets the caller already knows (ply_off:
// ngames + 1 entries, ply_off[g + 1] - ply_off[g] = 1 + the game's move
// tokens, as fnnue_backend_batch_size counts them): one launch, no sizing
// pass, no allocation, no host sync.  variant = kVariantChess (d_out:
// fnnue_pos) or a variant (fnnue_vpos).  d_err: 4 words, zero before the
// launch; afterwards err[0] = kBuildErr* of a failing game (0: none), err[1]
// that game, err[2] its ply.  d_final: optional kFinal* per game.
hipError_t replay_games_device(int variant, const char* d_text, const uint32_t* d_fen_off, const uint32_t* d_mv_off,
                               const uint32_t* d_ply_off, uint32_t ngames, void* d_out, uint8_t* d_final,
                               uint32_t* d_err, hipStream_t s);
// vbuilder.hip's launcher of the same (variants only).
hipError_t replay_vgames_device(int variant, const char* d_text, const uint32_t* d_fen_off, const uint32_t* d_mv_off,
                                const uint32_t* d_ply_off, uint32_t ngames, fnnue_vpos* d_out, void* d_states,
                                uint8_t* d_final, uint32_t* d_err, hipStream_t s);

// Leaf count of perft(depth) summed over the frontier boards (1 <= depth <= 3).
hipError_t perft_device(const std::vector<DBoard>& frontier, int depth, uint64_t* nodes);

}  // namespace fnnue
