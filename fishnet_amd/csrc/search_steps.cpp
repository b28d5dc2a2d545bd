// search_steps.cpp — the device search's host steps (search_steps.h).
#include "search_steps.h"

using namespace fnnue::detail;

namespace fnnue {

hipError_t count_children(SearchRules r, const void* d_states, uint32_t n, uint32_t* d_cnt, uint32_t* d_off,
                          hipStream_t s, BuilderScratch& ws) {
  return r.chess() ? children_count_device(static_cast<const DBoard*>(d_states), n, d_cnt, d_off, s, ws)
                   : vchildren_count_device(r.variant, d_states, n, d_cnt, d_off, s, ws);
}

hipError_t write_children(SearchRules r, const void* d_states, uint32_t n, const uint32_t* d_off, uint32_t total,
                          void* d_out, uint16_t* d_moves, uint8_t* d_end, hipStream_t s) {
  return r.chess() ? children_write_device(static_cast<const DBoard*>(d_states), n, d_off, total,
                                           static_cast<fnnue_pos*>(d_out), d_moves, d_end, s)
                   : vchildren_write_device(r.variant, d_states, n, d_off, total, static_cast<fnnue_vpos*>(d_out),
                                            d_moves, d_end, s);
}

hipError_t child_states(SearchRules r, const void* d_states, uint32_t n, const uint32_t* d_off, uint32_t total,
                        void* d_out, uint2* d_map, hipStream_t s) {
  return r.chess() ? child_states_device(static_cast<const DBoard*>(d_states), n, d_off, total,
                                         static_cast<DBoard*>(d_out), d_map, s)
                   : vchild_states_device(r.variant, d_states, n, d_off, total, d_out, d_map, s);
}

int eval_groups(SearchRules r, fnnue_ctx* ctx, const void* d_pos, const uint32_t* d_off, size_t ngroups, size_t npos,
                int mode, int32_t* d_psqt, int32_t* d_positional, hipStream_t s) {
  return r.chess() ? fnnue_eval_groups_device(ctx, static_cast<const fnnue_pos*>(d_pos), d_off, ngroups, npos, mode,
                                              d_psqt, d_positional, s)
                   : fnnue_eval_vgroups_device(ctx, static_cast<const fnnue_vpos*>(d_pos), d_off, ngroups, npos, mode,
                                               d_psqt, d_positional, s);
}

hipError_t best_replies(bool vranks, const uint8_t* d_end, const uint16_t* d_moves, const uint32_t* d_off,
                        uint32_t ngroups, uint32_t npos, const fnnue_best* d_child_best, const uint32_t* d_base,
                        fnnue_best2* d_out, hipStream_t s) {
  return (vranks ? launch_vbest_replies : launch_best_replies)(d_end, d_moves, d_off, ngroups, npos, d_child_best,
                                                               d_base, d_out, s);
}

hipError_t topk_replies(bool vranks, const uint8_t* d_end, const uint16_t* d_moves, const uint32_t* d_off,
                        uint32_t ngroups, uint32_t npos, const fnnue_best* d_child_best, const uint32_t* d_base,
                        const uint32_t* d_line_off, uint32_t uniform_k, fnnue_line2* d_lines, size_t lines_cap,
                        hipStream_t s) {
  return launch_topk_replies(vranks, d_end, d_moves, d_off, ngroups, npos, d_child_best, d_base, d_line_off,
                             uniform_k, d_lines, lines_cap, s);
}

int draw_history_level1(SearchRules r, const char* d_text, const uint32_t* d_fen_off, const uint32_t* d_mv_off,
                        const uint32_t* d_ply_off, uint32_t ngames, const void* d_states, uint32_t n,
                        const uint32_t* d_off, const uint16_t* d_moves, uint8_t* d_end, hipStream_t s,
                        BuilderScratch& ws, DrawHistory* hist, const PhaseHook* hook) {
  begin_phase(hook, kPhaseHistory);
  HIP_TRY(game_history_device(r, d_text, d_fen_off, d_mv_off, d_ply_off, ngames, d_states, n, draw_key_bits(), s, ws,
                              hist),
          "game history launch");
  begin_phase(hook, kPhaseMark);
  HIP_TRY(mark_draws_level1(r, *hist, d_states, n, d_off, d_moves, d_end, s), "draw marks launch");
  return FNNUE_OK;
}

int reduce_level1(fnnue_ctx* ctx, BuilderScratch& ws, SearchRules r, const SearchSettings& set, const StarGroups& g,
                  fnnue_best* d_out, const uint32_t* d_line_off, uint32_t uniform_k, fnnue_line* d_lines,
                  size_t lines_cap, hipStream_t s, QuiesceStats* qs) {
  if (set.quiesce > 0) {  // the children's terms become those of their capture lines' ends, before any reduction
    if (int rc = quiesce_leaves_device(ctx, ws, r, g.states, g.n, g.off, g.total, g.end, g.psqt, g.positional,
                                       set.quiesce, set.quiesce_checks, 1, s, qs))
      return rc;
  }
  HIP_TRY(launch_best_children(g.psqt, g.positional, g.end, g.moves, g.off, g.n, g.total, d_out, s),
          "best_children launch");
  if (d_lines)
    HIP_TRY(launch_topk_children(g.psqt, g.positional, g.end, g.moves, g.off, g.n, g.total, d_line_off, uniform_k,
                                 d_lines, lines_cap, s),
            "topk_children launch");
  return FNNUE_OK;
}

int search_level2_chunk(fnnue_ctx* ctx, BuilderScratch& ws, SearchRules r, const SearchSettings& set,
                        const StarGroups& l1, const void* d_kid_states, const uint32_t* d_kid_off,
                        const Level2Chunk& c, fnnue_best* d_kid_best, hipStream_t s, QuiesceStats* qs,
                        const PhaseHook* hook) {
  const char* chunk_states = static_cast<const char*>(d_kid_states) + (size_t)c.k0 * r.state_bytes();
  HIP_TRY(write_children(r, chunk_states, c.nk, c.ch_off, c.nr, c.pos, c.moves, c.end, s), "children write");
  if (set.draws) {  // behind the expansion, before the reduction reads the end bytes; offsets relative to the chunk
    begin_phase(hook, kPhaseMark);
    HIP_TRY(mark_draws_level2(r, *set.draws, l1.states, c.p0, c.p1, l1.off, d_kid_states, d_kid_off, c.rec0, c.moves,
                              c.end, s),
            "draw marks launch");
  }
  begin_phase(hook, kPhaseEval);
  if (int rc = eval_groups(r, ctx, c.pos, c.ch_off, c.nk, c.nr, FNNUE_GROUP_STAR, c.psqt, c.positional, s)) return rc;
  if (set.quiesce > 0) {  // the grandchildren's terms become those of their capture lines' ends
    begin_phase(hook, kPhaseQuiesce);
    if (int rc = quiesce_leaves_device(ctx, ws, r, chunk_states, c.nk, c.ch_off, c.nr, c.end, c.psqt, c.positional,
                                       set.quiesce, set.quiesce_checks, 2, s, qs))
      return rc;
  }
  begin_phase(hook, kPhaseReduce1);
  HIP_TRY(launch_best_children_own(c.psqt, c.positional, c.end, c.moves, c.ch_off, c.nk, c.nr, d_kid_best + c.k0, s),
          "best_children launch");
  if (set.draws) {  // a drawn child's pv ends at it: its own terms, while the chunk still holds them
    begin_phase(hook, kPhaseMark);
    HIP_TRY(draw_own_terms(*set.draws, c.p0, c.p1, l1.off, l1.end, d_kid_off, c.rec0, c.psqt, c.positional,
                           d_kid_best, s),
            "draw terms launch");
  }
  return FNNUE_OK;
}

}  // namespace fnnue
