// search_steps.h — the device search's host steps, once for both callers: the C API (search_api.cpp:
// BuilderScratch buffers, sizes behind a stream synchronise, the plies cut into chunks under a budget) and the
// backend (backend.cpp: DevBufs, sizes behind its timed wait, a piece as one chunk).  A step that needs a buffer
// gets the pointer; nothing here allocates, waits for a size or reads a caller's settings.
#pragma once
#include "internal.h"

namespace fnnue {

// The rules a search runs under.  Boards and records travel as void*: DBoard and
// fnnue_pos for chess, vstate_bytes(variant) boards and fnnue_vpos for a variant.
// Only the functions below choose between the chess kernels and the variants'.
struct SearchRules {
  int variant = kVariantChess;
  bool chess() const { return variant == kVariantChess; }
  size_t state_bytes() const { return chess() ? sizeof(DBoard) : vstate_bytes(variant); }
  size_t record_bytes() const { return chess() ? sizeof(fnnue_pos) : sizeof(fnnue_vpos); }
  // the variant ranks in the second reduction: FNNUE_END_WON children, every reply loses at once
  bool vranks() const { return !chess(); }
};

// children_count_device / children_write_device / child_states_device, or their variant forms.
hipError_t count_children(SearchRules r, const void* d_states, uint32_t n, uint32_t* d_cnt, uint32_t* d_off,
                          hipStream_t s, BuilderScratch& ws);
hipError_t write_children(SearchRules r, const void* d_states, uint32_t n, const uint32_t* d_off, uint32_t total,
                          void* d_out, uint16_t* d_moves, uint8_t* d_end, hipStream_t s);
hipError_t child_states(SearchRules r, const void* d_states, uint32_t n, const uint32_t* d_off, uint32_t total,
                        void* d_out, uint2* d_map, hipStream_t s);
// fnnue_eval_[v]groups_device in `mode` (FNNUE_GROUP_STAR for a search's groups); an FNNUE_* code.
int eval_groups(SearchRules r, fnnue_ctx* ctx, const void* d_pos, const uint32_t* d_off, size_t ngroups, size_t npos,
                int mode, int32_t* d_psqt, int32_t* d_positional, hipStream_t s);
// The second reduction, and the k best lines over the same arrays (builder.h).
hipError_t best_replies(bool vranks, const uint8_t* d_end, const uint16_t* d_moves, const uint32_t* d_off,
                        uint32_t ngroups, uint32_t npos, const fnnue_best* d_child_best, const uint32_t* d_base,
                        fnnue_best2* d_out, hipStream_t s);
hipError_t topk_replies(bool vranks, const uint8_t* d_end, const uint16_t* d_moves, const uint32_t* d_off,
                        uint32_t ngroups, uint32_t npos, const fnnue_best* d_child_best, const uint32_t* d_base,
                        const uint32_t* d_line_off, uint32_t uniform_k, fnnue_line2* d_lines, size_t lines_cap,
                        hipStream_t s);

// A caller's copy of its search settings: the draws and the quiescence are the caller's
// settings for the rules it searches under (the chess ones or the variants').
struct SearchSettings {
  const DrawHistory* draws = nullptr;  // the plies' history (draw_history_level1), or none
  int quiesce = 0;                     // capture quiescence depth below the leaves
  bool quiesce_checks = false;         // evasions and mates inside that tree
};

// quiesce.hip.  The search's form: the leaves are the records j >= 1 of the n
// parents' STAR groups (d_off: n + 1, total = d_off[n]; d_parents: the groups'
// first records' boards, r.state_bytes() each); every leaf whose end byte has
// neither kFinalNoMoves nor kFinalDraw (a variant's kFinalWon children have
// kFinalNoMoves too) gets its two terms replaced in place by the reported terms
// of Q_depth.  Runs behind the groups' evaluation on `s`, reads each level's size
// back (synchronises `s`), evaluates through ctx, temporaries from ws.
// checks: the rule Q'_depth (ABI 3.14; a variant: chk() of ABI 3.15).  A decided
// leaf gets (0, 16 * v) with v `ply` further from the mate value (the leaves'
// depth in the search, 1 or 2), a decided draw (0, 0).
int quiesce_leaves_device(fnnue_ctx* ctx, BuilderScratch& ws, SearchRules r, const void* d_parents, uint32_t n,
                          const uint32_t* d_off, uint32_t total, const uint8_t* d_end, int32_t* d_psqt,
                          int32_t* d_positional, int depth, bool checks, int ply, hipStream_t s, QuiesceStats* st);
// fnnue_[v]quiesce_device's form: the n boards themselves are the roots, one
// fnnue_quiet each (their own evaluation included).
int quiesce_nodes_device(fnnue_ctx* ctx, BuilderScratch& ws, SearchRules r, const void* d_states, uint32_t n, int depth,
                         bool checks, fnnue_quiet* d_out, hipStream_t s, QuiesceStats* st);

// The phases FNNUE_SEARCH2_TRACE times (search_api.cpp); a step that begins one
// tells the hook, when there is one.  kSearchPhases: the end of the call.
enum SearchPhase {
  kPhaseLevel1, kPhaseChildStates, kPhaseCount, kPhaseExpand, kPhaseEval, kPhaseReduce1, kPhaseReduce2, kPhaseTopk,
  kPhaseHistory, kPhaseMark, kPhaseQuiesce, kSearchPhases
};
struct PhaseHook {
  void (*begin)(void* arg, int phase);
  void* arg;
};
inline void begin_phase(const PhaseHook* h, int phase) {
  if (h) h->begin(h->arg, phase);
}

// draws.hip, under r's rule (include/fnnue.h: chess ABI 3.12, the variants ABI
// 3.16).  The history of n plies (d_states: the replay's boards, r.state_bytes()
// each; d_ply_off: ngames + 1) into the scratch and *out (builder.h
// DrawHistory).  key_bits: 1..63.  A few small kernels, stream-ordered, no sync.
hipError_t game_history_device(SearchRules r, const char* d_text, const uint32_t* d_fen_off, const uint32_t* d_mv_off,
                               const uint32_t* d_ply_off, uint32_t ngames, const void* d_states, uint32_t n,
                               uint32_t key_bits, hipStream_t s, BuilderScratch& ws, DrawHistory* out);
// The marking passes, over the listed plies alone (an early-out on an empty
// list).  Level 1: the children of the plies' STAR groups (d_off: n + 1), each
// record's move code applied to its ply's board.  Level 2: the grandchildren of
// the plies [p0, p1), parents d_kid_states (dense, child j of ply i at
// d_off[i] - i + j - 1), their STAR offsets d_kid_off (whole array), the
// records' arrays starting at record rec0 (a chunk).
hipError_t mark_draws_level1(SearchRules r, const DrawHistory& h, const void* d_states, uint32_t n,
                             const uint32_t* d_off, const uint16_t* d_moves, uint8_t* d_end, hipStream_t s);
hipError_t mark_draws_level2(SearchRules r, const DrawHistory& h, const void* d_states, uint32_t p0, uint32_t p1,
                             const uint32_t* d_off, const void* d_kid_states, const uint32_t* d_kid_off, uint32_t rec0,
                             const uint16_t* d_gmoves, uint8_t* d_gend, hipStream_t s);

// The draw rules at level 1: the history of the n plies (d_states: the
// replay's boards, d_ply_off: ngames + 1) into *hist, then the marks on the
// end bytes of the listed plies' children (d_off: the plies' STAR offsets).
int draw_history_level1(SearchRules r, const char* d_text, const uint32_t* d_fen_off, const uint32_t* d_mv_off,
                        const uint32_t* d_ply_off, uint32_t ngames, const void* d_states, uint32_t n,
                        const uint32_t* d_off, const uint16_t* d_moves, uint8_t* d_end, hipStream_t s,
                        BuilderScratch& ws, DrawHistory* hist, const PhaseHook* hook);

// The n plies' STAR groups (d_off: n + 1, total records), evaluated: what every level shares.
struct StarGroups {
  const void* states = nullptr;  // the groups' first records' boards
  uint32_t n = 0;
  const uint32_t* off = nullptr;
  uint32_t total = 0;
  const uint16_t* moves = nullptr;
  uint8_t* end = nullptr;
  int32_t* psqt = nullptr;
  int32_t* positional = nullptr;
};

// The end of a one-ply search over evaluated groups: the quiescence of the
// children's terms (set.quiesce > 0), the reduction into d_out, and with
// d_lines the k best children (slots: launch_topk_children's).
int reduce_level1(fnnue_ctx* ctx, BuilderScratch& ws, SearchRules r, const SearchSettings& set, const StarGroups& g,
                  fnnue_best* d_out, const uint32_t* d_line_off, uint32_t uniform_k, fnnue_line* d_lines,
                  size_t lines_cap, hipStream_t s, QuiesceStats* qs);

// One chunk of level 2: the grandchildren of the plies [p0, p1), in today's order:
// written, their draws marked, evaluated, quiesced, reduced into d_kid_best[k0 ..],
// and a drawn child given its own terms.  l1: the call's level-1 groups (states,
// off, end).  d_kid_states / d_kid_off: the dense child boards and their STAR
// offsets, whole arrays; the chunk's nk children start at k0 and their nr records
// at rec0; ch_off (nk + 1): d_kid_off from k0 on less rec0 (d_kid_off itself for a
// piece that is one chunk).  The record arrays hold the chunk's nr entries.
struct Level2Chunk {
  uint32_t p0 = 0, p1 = 0, k0 = 0, nk = 0, rec0 = 0, nr = 0;
  const uint32_t* ch_off = nullptr;
  void* pos = nullptr;
  uint16_t* moves = nullptr;
  uint8_t* end = nullptr;
  int32_t* psqt = nullptr;
  int32_t* positional = nullptr;
};
int search_level2_chunk(fnnue_ctx* ctx, BuilderScratch& ws, SearchRules r, const SearchSettings& set,
                        const StarGroups& l1, const void* d_kid_states, const uint32_t* d_kid_off,
                        const Level2Chunk& c, fnnue_best* d_kid_best, hipStream_t s, QuiesceStats* qs,
                        const PhaseHook* hook);

}  // namespace fnnue
