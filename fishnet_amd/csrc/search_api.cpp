// search_api.cpp — the C ABI's device builder, search, replies, quiescence and draw-history entry points
// (include/fnnue.h): argument checks, the context's scratch, size read-backs, chunk cuts; the steps: search_steps.cpp.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <type_traits>
#include <utility>
#include <vector>

#include "../../include/fnnue.h"
#include "builder.h"
#include "internal.h"
#include "search_steps.h"

using namespace fnnue;
using namespace fnnue::detail;

namespace {

// What a builder or replay call found, as the entry point's answer: the counts, its first error, then capacity
// (a replay that lacks room says so before it replays anything, so no game's error comes with it).  Every code
// but kBuildErrFen reads as an illegal move: kBuildErrCount needs a caller's own counts, which none here has.
int builder_result(const BuildResult& R, bool variant, size_t* n_out, size_t* n_groups) {
  if (R.hip != hipSuccess) return hip_fail(R.hip, variant ? "device variant batch builder" : "device batch builder");
  *n_out = R.n_out;
  *n_groups = R.n_groups;
  if (R.err_code == kBuildErrFen)
    return fail(FNNUE_E_FEN, std::string("unparsable ") + (variant ? "variant " : "") + "FEN in game " +
                                 std::to_string(R.err_game));
  if (R.err_code)
    return fail(FNNUE_E_MOVE, "illegal move at ply " + std::to_string(R.err_ply) + " of game " +
                                  std::to_string(R.err_game));
  if (R.capacity) return fail(FNNUE_E_CAPACITY, "output buffer too small");
  return FNNUE_OK;
}

// Level 1 of both searches: the plies' boards (kStates) and their STAR groups'
// records, offsets, moves and end flags in the context's scratch, at most
// max_plies plies (checked before any is expanded).
struct Level1 {
  size_t max_plies = 0;
  const void* pos = nullptr;
  const uint32_t* off = nullptr;
  uint16_t* moves = nullptr;
  uint8_t* end = nullptr;
  const uint32_t* ply_off = nullptr;  // each game's first ply (ngames + 1)
};

// fnnue_build_batch_device, with d_moves / d_end fnnue_build_[v]children_device (records: fnnue_pos for chess,
// fnnue_vpos for a variant), and with `own` the searches' level 1, the caller's buffers ignored.
int build_device(fnnue_ctx* ctx, int variant, const char* d_text, const uint32_t* d_fen_off,
                 const uint32_t* d_moves_off, size_t ngames, bool children, void* d_out, size_t cap, uint32_t* d_off,
                 size_t off_cap, uint16_t* d_moves, uint8_t* d_end, size_t* n_out, size_t* n_groups, void* stream,
                 Level1* own = nullptr) {
  if (!ctx || !n_out || !n_groups) return fail(FNNUE_E_ARG, "null argument");
  *n_out = *n_groups = 0;
  if (!variant_known(variant)) return fail(FNNUE_E_ARG, "unknown variant " + std::to_string(variant));
  if (ngames == 0) return FNNUE_OK;
  if (!d_text || !d_fen_off || !d_moves_off) return fail(FNNUE_E_ARG, "null buffer");
  if (ngames > (1u << 26)) return fail(FNNUE_E_ARG, "too many games");
  DeviceGuard g(ctx->device);
  hipStream_t s = stream ? static_cast<hipStream_t>(stream) : ctx->stream;
  BuildResult R;
  if (variant == kVariantChess) {
    ChildrenBufs kids;
    kids.max_groups = own ? own->max_plies : 0;
    R = build_batch_device(d_text, d_fen_off, d_moves_off, (uint32_t)ngames, children, static_cast<fnnue_pos*>(d_out),
                           cap, d_off, off_cap, s, ctx->bscratch, nullptr, d_moves, d_end, own ? &kids : nullptr);
    if (own) *own = {own->max_plies, kids.pos, kids.off, kids.moves, kids.end, kids.ply_off};
  } else {
    VChildrenBufs kids;
    kids.max_groups = own ? own->max_plies : 0;
    R = build_vbatch_device(variant, d_text, d_fen_off, d_moves_off, (uint32_t)ngames, children,
                            static_cast<fnnue_vpos*>(d_out), cap, d_off, off_cap, s, ctx->bscratch, nullptr, d_moves,
                            d_end, own ? &kids : nullptr);
    if (own) *own = {own->max_plies, kids.pos, kids.off, kids.moves, kids.end, kids.ply_off};
  }
  return builder_result(R, variant != kVariantChess, n_out, n_groups);
}

// A host game text and its offsets, staged in the context's builder input on its stream.
struct StagedGames {
  char* text = nullptr;
  uint32_t *fen_off = nullptr, *moves_off = nullptr;
};
int stage_games(fnnue_ctx* ctx, const char* text, size_t text_len, const uint32_t* fen_off, const uint32_t* moves_off,
                size_t ngames, StagedGames* d) {
  if (fen_off[ngames] > text_len) return fail(FNNUE_E_ARG, "offsets exceed the text");
  for (size_t i = 0; i < ngames; ++i)
    if (fen_off[i] > moves_off[i] || moves_off[i] > fen_off[i + 1]) return fail(FNNUE_E_ARG, "offsets out of order");
  const size_t text_bytes = (text_len + 255) / 256 * 256;
  const size_t fo_bytes = (ngames + 1) * 4, mo_bytes = ngames * 4;
  if (int rc = ensure_builder_input(ctx, text_bytes + fo_bytes + mo_bytes)) return rc;
  d->text = ctx->d_btext;
  d->fen_off = reinterpret_cast<uint32_t*>(ctx->d_btext + text_bytes);
  d->moves_off = d->fen_off + (ngames + 1);
  hipStream_t s = ctx->stream;
  HIP_TRY(hipMemcpyAsync(d->text, text, text_len, hipMemcpyHostToDevice, s), "H2D");
  HIP_TRY(hipMemcpyAsync(d->fen_off, fen_off, fo_bytes, hipMemcpyHostToDevice, s), "H2D");
  HIP_TRY(hipMemcpyAsync(d->moves_off, moves_off, mo_bytes, hipMemcpyHostToDevice, s), "H2D");
  return FNNUE_OK;
}

// A device buffer for the length of one host-buffer call, as a packed layout:
// part(&ptr, n) appends n entries of ptr's type (the caller lists the 4-byte
// parts first) and nulls ptr; get() allocates what the parts add up to and
// points every ptr at its part.
struct TempDev {
  void* p = nullptr;
  size_t bytes = 0;
  std::vector<std::pair<void**, size_t>> parts;
  ~TempDev() {
    if (p) (void)hipFree(p);
  }
  int get(size_t n) { return hipMalloc(&p, n ? n : 1) == hipSuccess ? FNNUE_OK : fail(FNNUE_E_OOM, "device allocation"); }
  template <class T>
  void part(T** ptr, size_t n) {
    *ptr = nullptr;
    parts.emplace_back(reinterpret_cast<void**>(ptr), bytes);
    bytes += n * sizeof(T);
  }
  int get() {
    if (int rc = get(bytes)) return rc;
    for (auto& [ptr, at] : parts) *ptr = static_cast<char*>(p) + at;
    return FNNUE_OK;
  }
};

// The host form of fnnue_build_[v]children_device (`device`: that call on the
// staged games): a sizing pass, which is always "too small" with no outputs,
// then the records through [records | off | moves | end] (chess: [moves | end] beside the context's staging).
template <class Rec, class Device>
int build_children_host(fnnue_ctx* ctx, const char* text, size_t text_len, const uint32_t* fen_off,
                        const uint32_t* moves_off, size_t ngames, Rec* out, size_t cap, uint32_t* off, size_t off_cap,
                        fnnue_move* moves, uint8_t* end, size_t* n_out, size_t* n_groups, Device device) {
  DeviceGuard g(ctx->device);
  StagedGames d;
  int rc = stage_games(ctx, text, text_len, fen_off, moves_off, ngames, &d);
  if (rc) return rc;
  hipStream_t s = ctx->stream;
  rc = device(d, s, static_cast<Rec*>(nullptr), 0, nullptr, 0, nullptr, nullptr);
  if (rc != FNNUE_E_CAPACITY) return rc;
  if (!out || !off || !moves || !end || cap < *n_out || off_cap < *n_groups + 1)
    return fail(FNNUE_E_CAPACITY, "output buffer too small");
  const size_t nrec = *n_out, ng = *n_groups;
  Rec* d_out;
  uint32_t* d_off;
  fnnue_move* d_mv;
  uint8_t* d_end;
  TempDev buf;
  if constexpr (std::is_same_v<Rec, fnnue_pos>) {  // chess: the context's grow-only staging, as fnnue_build_batch
    if ((rc = ensure_stage(ctx, nrec, ng + 1))) return rc;
    d_out = ctx->d_pos, d_off = ctx->d_off;
  } else buf.part(&d_out, nrec), buf.part(&d_off, ng + 1);
  buf.part(&d_mv, nrec), buf.part(&d_end, nrec);
  if ((rc = buf.get()) || (rc = device(d, s, d_out, nrec, d_off, ng + 1, d_mv, d_end))) return rc;
  HIP_TRY(hipMemcpyAsync(out, d_out, *n_out * sizeof(Rec), hipMemcpyDeviceToHost, s), "D2H");
  HIP_TRY(hipMemcpyAsync(off, d_off, (*n_groups + 1) * 4, hipMemcpyDeviceToHost, s), "D2H");
  HIP_TRY(hipMemcpyAsync(moves, d_mv, *n_out * 2, hipMemcpyDeviceToHost, s), "D2H");
  HIP_TRY(hipMemcpyAsync(end, d_end, *n_out, hipMemcpyDeviceToHost, s), "D2H");
  HIP_TRY(hipStreamSynchronize(s), "hipStreamSynchronize");
  return FNNUE_OK;
}

// What fnnue_[v]quiesce_device and fnnue_game_history_device share: the games'
// plies replayed into the context's scratch (ordered like its workspace),
// body(boards, plies, ply_off, s) over them, then the games' offsets to d_off.
template <class Body>
int replayed_plies(fnnue_ctx* ctx, int variant, const char* d_text, const uint32_t* d_fen_off, const uint32_t* d_moves_off,
                   size_t ngames, size_t room, uint32_t* d_off, size_t* n_out, size_t* n_groups, void* stream,
                   Body body) {
  if (ngames == 0) return FNNUE_OK;
  if (!d_text || !d_fen_off || !d_moves_off) return fail(FNNUE_E_ARG, "null buffer");
  if (ngames > (1u << 26)) return fail(FNNUE_E_ARG, "too many games");
  DeviceGuard g(ctx->device);
  hipStream_t s = stream ? static_cast<hipStream_t>(stream) : ctx->stream;
  int rc = order_workspace(ctx, s);
  if (rc) return rc;
  WorkspaceUse use{ctx, s};
  const void* states = nullptr;
  const uint32_t* ply_off = nullptr;
  const BuildResult R = replay_states_device(variant, d_text, d_fen_off, d_moves_off, (uint32_t)ngames, room, s,
                                             ctx->bscratch, &states, &ply_off);
  if ((rc = builder_result(R, variant != kVariantChess, n_out, n_groups)) || (rc = body(states, R.n_out, ply_off, s)))
    return rc;
  HIP_TRY(hipMemcpyAsync(d_off, ply_off, (ngames + 1) * 4, hipMemcpyDeviceToDevice, s), "D2D(offsets)");
  return FNNUE_OK;
}

// The host form of a device call that answers one record per ply (`device`:
// that call on the staged games, with no room when the caller has none):
// through [records | off, 16-byte aligned], then the error word if `latch`.
template <class Rec, class Device>
int plies_host(fnnue_ctx* ctx, const char* text, size_t text_len, const uint32_t* fen_off, const uint32_t* moves_off,
               size_t ngames, Rec* out, size_t cap, uint32_t* off, size_t off_cap, size_t* n_out, bool latch,
               Device device) {
  DeviceGuard g(ctx->device);
  StagedGames d;
  int rc = stage_games(ctx, text, text_len, fen_off, moves_off, ngames, &d);
  if (rc) return rc;
  const bool room = out && off && off_cap >= ngames + 1;
  Rec* d_out;
  uint32_t* d_off;
  TempDev buf;
  buf.part(&d_out, cap), buf.bytes = (buf.bytes + 15) / 16 * 16, buf.part(&d_off, ngames + 1);
  if (room && (rc = buf.get())) return rc;
  hipStream_t s = ctx->stream;
  if ((rc = device(d, s, d_out, room ? cap : 0, d_off, room ? off_cap : 0))) return rc;
  HIP_TRY(hipMemcpyAsync(out, d_out, *n_out * sizeof(Rec), hipMemcpyDeviceToHost, s), "D2H");
  HIP_TRY(hipMemcpyAsync(off, d_off, (ngames + 1) * 4, hipMemcpyDeviceToHost, s), "D2H");
  HIP_TRY(hipStreamSynchronize(s), "hipStreamSynchronize");
  return latch ? latched(ctx) : (int)FNNUE_OK;
}

}  // namespace

extern "C" {

int fnnue_build_batch_device(fnnue_ctx* ctx, const char* d_text, const uint32_t* d_fen_off,
                             const uint32_t* d_moves_off, size_t ngames, int mode, fnnue_pos* d_out, size_t cap,
                             uint32_t* d_off, size_t off_cap, size_t* n_out, size_t* n_groups, void* stream) {
  if (!ctx || !n_out || !n_groups) return fail(FNNUE_E_ARG, "null argument");
  if (mode != FNNUE_PLAYOUT_PLIES && mode != FNNUE_PLAYOUT_CHILDREN) return fail(FNNUE_E_ARG, "bad build mode");
  return build_device(ctx, kVariantChess, d_text, d_fen_off, d_moves_off, ngames, mode == FNNUE_PLAYOUT_CHILDREN, d_out,
                      cap, d_off, off_cap, nullptr, nullptr, n_out, n_groups, stream);
}

int fnnue_build_children_device(fnnue_ctx* ctx, const char* d_text, const uint32_t* d_fen_off,
                                const uint32_t* d_moves_off, size_t ngames, fnnue_pos* d_out, size_t cap,
                                uint32_t* d_off, size_t off_cap, fnnue_move* d_moves, uint8_t* d_end, size_t* n_out,
                                size_t* n_groups, void* stream) {
  if (!ctx || !n_out || !n_groups) return fail(FNNUE_E_ARG, "null argument");
  if (d_out && (!d_moves || !d_end)) return fail(FNNUE_E_ARG, "null moves / end buffer");
  return build_device(ctx, kVariantChess, d_text, d_fen_off, d_moves_off, ngames, true, d_out, cap, d_off, off_cap,
                      d_moves, d_end, n_out, n_groups, stream);
}

int fnnue_build_children(fnnue_ctx* ctx, const char* text, size_t text_len, const uint32_t* fen_off,
                         const uint32_t* moves_off, size_t ngames, fnnue_pos* out, size_t cap, uint32_t* off,
                         size_t off_cap, fnnue_move* moves, uint8_t* end, size_t* n_out, size_t* n_groups) {
  if (!ctx || !n_out || !n_groups || (ngames && (!text || !fen_off || !moves_off)))
    return fail(FNNUE_E_ARG, "null argument");
  *n_out = *n_groups = 0;
  if (ngames == 0) return FNNUE_OK;
  return build_children_host(ctx, text, text_len, fen_off, moves_off, ngames, out, cap, off, off_cap, moves, end, n_out,
                             n_groups, [&](const StagedGames& d, hipStream_t s, auto... outputs) {
                               return fnnue_build_children_device(ctx, d.text, d.fen_off, d.moves_off, ngames,
                                                                  outputs..., n_out, n_groups, s);
                             });
}

int fnnue_best_children_device(fnnue_ctx* ctx, const int32_t* d_psqt, const int32_t* d_positional,
                               const uint8_t* d_end, const fnnue_move* d_moves, const uint32_t* d_off, size_t ngroups,
                               size_t npos, fnnue_best* d_out, void* stream) {
  if (!ctx) return fail(FNNUE_E_ARG, "null ctx");
  if (ngroups == 0) return FNNUE_OK;
  if (!d_psqt || !d_positional || !d_end || !d_off || !d_out) return fail(FNNUE_E_ARG, "null buffer");
  if (ngroups > 0xFFFFFFFEu || npos > 0xFFFFFFFFu) return fail(FNNUE_E_ARG, "batch too large");
  DeviceGuard g(ctx->device);
  hipStream_t s = stream ? static_cast<hipStream_t>(stream) : ctx->stream;
  HIP_TRY(launch_best_children(d_psqt, d_positional, d_end, d_moves, d_off, (uint32_t)ngroups, (uint32_t)npos, d_out,
                               s),
          "best_children launch");
  return FNNUE_OK;
}

int fnnue_best_children(fnnue_ctx* ctx, const int32_t* psqt, const int32_t* positional, const uint8_t* end,
                        const fnnue_move* moves, const uint32_t* off, size_t ngroups, size_t npos, fnnue_best* out) {
  if (!ctx) return fail(FNNUE_E_ARG, "null ctx");
  if (ngroups == 0) return FNNUE_OK;
  if (!off || !out || (npos && (!psqt || !positional || !end))) return fail(FNNUE_E_ARG, "null buffer");
  if (ngroups > 0xFFFFFFFEu || npos > 0xFFFFFFFFu) return fail(FNNUE_E_ARG, "batch too large");
  DeviceGuard g(ctx->device);
  int32_t *d_ps, *d_po;
  uint32_t* d_off;
  fnnue_best* d_out;
  fnnue_move* d_mv;
  uint8_t* d_end;
  TempDev buf;  // [psqt | positional | off | out | moves | end]
  buf.part(&d_ps, npos), buf.part(&d_po, npos), buf.part(&d_off, ngroups + 1), buf.part(&d_out, ngroups);
  buf.part(&d_mv, npos), buf.part(&d_end, npos);
  if (int rc = buf.get()) return rc;
  if (!moves) d_mv = nullptr;
  hipStream_t s = ctx->stream;
  if (npos) {
    HIP_TRY(hipMemcpyAsync(d_ps, psqt, npos * 4, hipMemcpyHostToDevice, s), "H2D");
    HIP_TRY(hipMemcpyAsync(d_po, positional, npos * 4, hipMemcpyHostToDevice, s), "H2D");
    HIP_TRY(hipMemcpyAsync(d_end, end, npos, hipMemcpyHostToDevice, s), "H2D");
    if (moves) HIP_TRY(hipMemcpyAsync(d_mv, moves, npos * 2, hipMemcpyHostToDevice, s), "H2D");
  }
  HIP_TRY(hipMemcpyAsync(d_off, off, (ngroups + 1) * 4, hipMemcpyHostToDevice, s), "H2D");
  const int rc = fnnue_best_children_device(ctx, d_ps, d_po, d_end, d_mv, d_off, ngroups, npos, d_out, s);
  if (rc) return rc;
  HIP_TRY(hipMemcpyAsync(out, d_out, ngroups * sizeof(fnnue_best), hipMemcpyDeviceToHost, s), "D2H");
  HIP_TRY(hipStreamSynchronize(s), "hipStreamSynchronize");
  return FNNUE_OK;
}

int fnnue_topk_children_device(fnnue_ctx* ctx, const int32_t* d_psqt, const int32_t* d_positional,
                               const uint8_t* d_end, const fnnue_move* d_moves, const uint32_t* d_off, size_t ngroups,
                               size_t npos, const uint32_t* d_line_off, fnnue_line* d_lines, size_t lines_cap,
                               void* stream) {
  if (!ctx) return fail(FNNUE_E_ARG, "null ctx");
  if (ngroups == 0) return FNNUE_OK;
  if (!d_psqt || !d_positional || !d_end || !d_off || !d_line_off || (lines_cap && !d_lines))
    return fail(FNNUE_E_ARG, "null buffer");
  if (ngroups > 0xFFFFFFFEu || npos > 0xFFFFFFFFu) return fail(FNNUE_E_ARG, "batch too large");
  if (lines_cap == 0) return FNNUE_OK;  // no slot may be written
  DeviceGuard g(ctx->device);
  hipStream_t s = stream ? static_cast<hipStream_t>(stream) : ctx->stream;
  HIP_TRY(launch_topk_children(d_psqt, d_positional, d_end, d_moves, d_off, (uint32_t)ngroups, (uint32_t)npos,
                               d_line_off, 0, d_lines, lines_cap, s),
          "topk_children launch");
  return FNNUE_OK;
}

int fnnue_topk_children(fnnue_ctx* ctx, const int32_t* psqt, const int32_t* positional, const uint8_t* end,
                        const fnnue_move* moves, const uint32_t* off, size_t ngroups, size_t npos,
                        const uint32_t* line_off, fnnue_line* lines, size_t lines_cap) {
  if (!ctx) return fail(FNNUE_E_ARG, "null ctx");
  if (ngroups == 0) return FNNUE_OK;
  if (!off || !line_off || (npos && (!psqt || !positional || !end))) return fail(FNNUE_E_ARG, "null buffer");
  if (ngroups > 0xFFFFFFFEu || npos > 0xFFFFFFFFu) return fail(FNNUE_E_ARG, "batch too large");
  for (size_t g = 0; g < ngroups; ++g)
    if (line_off[g] > line_off[g + 1]) return fail(FNNUE_E_ARG, "line offsets decrease");
  const size_t nl = line_off[ngroups];
  if (nl > lines_cap) return fail(FNNUE_E_CAPACITY, "line buffer too small");
  if (nl && !lines) return fail(FNNUE_E_ARG, "null buffer");
  if (nl == 0) return FNNUE_OK;
  DeviceGuard g(ctx->device);
  int32_t *d_ps, *d_po;
  uint32_t *d_off, *d_loff;
  fnnue_line* d_lines;
  fnnue_move* d_mv;
  uint8_t* d_end;
  TempDev buf;  // [psqt | positional | off | line_off | lines | moves | end]
  buf.part(&d_ps, npos), buf.part(&d_po, npos), buf.part(&d_off, ngroups + 1), buf.part(&d_loff, ngroups + 1);
  buf.part(&d_lines, nl), buf.part(&d_mv, npos), buf.part(&d_end, npos);
  if (int rc = buf.get()) return rc;
  if (!moves) d_mv = nullptr;
  hipStream_t s = ctx->stream;
  if (npos) {
    HIP_TRY(hipMemcpyAsync(d_ps, psqt, npos * 4, hipMemcpyHostToDevice, s), "H2D");
    HIP_TRY(hipMemcpyAsync(d_po, positional, npos * 4, hipMemcpyHostToDevice, s), "H2D");
    HIP_TRY(hipMemcpyAsync(d_end, end, npos, hipMemcpyHostToDevice, s), "H2D");
    if (moves) HIP_TRY(hipMemcpyAsync(d_mv, moves, npos * 2, hipMemcpyHostToDevice, s), "H2D");
  }
  HIP_TRY(hipMemcpyAsync(d_off, off, (ngroups + 1) * 4, hipMemcpyHostToDevice, s), "H2D");
  HIP_TRY(hipMemcpyAsync(d_loff, line_off, (ngroups + 1) * 4, hipMemcpyHostToDevice, s), "H2D");
  // the caller's lines go up first, so that slots no group writes (empty groups) come back as they were
  HIP_TRY(hipMemcpyAsync(d_lines, lines, nl * sizeof(fnnue_line), hipMemcpyHostToDevice, s), "H2D");
  const int rc = fnnue_topk_children_device(ctx, d_ps, d_po, d_end, d_mv, d_off, ngroups, npos, d_loff, d_lines, nl, s);
  if (rc) return rc;
  HIP_TRY(hipMemcpyAsync(lines, d_lines, nl * sizeof(fnnue_line), hipMemcpyDeviceToHost, s), "D2H");
  HIP_TRY(hipStreamSynchronize(s), "hipStreamSynchronize");
  return FNNUE_OK;
}

}  // extern "C"

namespace {

// The net a one-ply search of `variant` needs: fnnue_search1* a chess net,
// fnnue_vsearch1* one whose feature set and game-over records are the
// variant's (its own net; the atomic net also for kingofthehill, racingkings, threecheck).
int search1_arch(const fnnue_ctx* ctx, int variant) {
  if (variant == kVariantChess)
    return ctx->variant == kVariantChess ? (int)FNNUE_OK : fail(FNNUE_E_ARCH, "the one-ply search needs a chess net");
  if (!variant_known(variant)) return fail(FNNUE_E_ARCH, "unknown variant " + std::to_string(variant));
  if (ctx->variant == variant || (ctx->variant == kVariantAtomic && variant_board_only(variant))) return FNNUE_OK;
  return fail(FNNUE_E_ARCH, std::string("the context's net (") + variant_name(ctx->variant) + ") does not evaluate " +
                                variant_name(variant));
}

// fnnue_search1_device, and with k >= 1 fnnue_search1_lines_device: ply p's k
// best children at d_lines[p * k ..] from the same scratch, behind the reduction.
int search1_device(fnnue_ctx* ctx, int variant, const char* d_text, const uint32_t* d_fen_off,
                   const uint32_t* d_moves_off, size_t ngames, uint32_t k, fnnue_best* d_out, size_t cap,
                   uint32_t* d_off, size_t off_cap, fnnue_line* d_lines, size_t lines_cap, size_t* n_out,
                   size_t* n_groups, void* stream) {
  if (!ctx || !n_out || !n_groups) return fail(FNNUE_E_ARG, "null argument");
  *n_out = *n_groups = 0;
  if (int rc = search1_arch(ctx, variant)) return rc;
  if (ngames == 0) return FNNUE_OK;
  DeviceGuard g(ctx->device);
  hipStream_t s = stream ? static_cast<hipStream_t>(stream) : ctx->stream;
  // the children and their terms live in the context's scratch: ordered like its workspace
  int rc = order_workspace(ctx, s);
  if (rc) return rc;
  WorkspaceUse use{ctx, s};
  BuilderScratch& ws = ctx->bscratch;
  const SearchRules rules{variant};
  size_t max_plies = d_out && d_off && off_cap >= ngames + 1 ? cap : 0;
  if (k) max_plies = d_lines ? std::min(max_plies, lines_cap / k) : 0;
  Level1 kids{max_plies};
  size_t nrec = 0, nply = 0;
  rc = build_device(ctx, variant, d_text, d_fen_off, d_moves_off, ngames, true, nullptr, 0, nullptr, 0, nullptr, nullptr,
                    &nrec, &nply, s, &kids);
  *n_out = nply;
  *n_groups = nply || rc == FNNUE_OK ? ngames : 0;
  if (rc) return rc;
  int32_t *ps = nullptr, *po = nullptr;
  HIP_TRY(ws.get(BuilderScratch::kKidPsqt, nrec * 4, (void**)&ps), "device allocation (search scratch)");
  HIP_TRY(ws.get(BuilderScratch::kKidPositional, nrec * 4, (void**)&po), "device allocation (search scratch)");
  if ((rc = eval_groups(rules, ctx, kids.pos, kids.off, nply, nrec, FNNUE_GROUP_STAR, ps, po, s))) return rc;
  SearchSettings set{nullptr, rules.chess() ? ctx->search_quiesce : ctx->search_vquiesce,
                     rules.chess() ? ctx->search_quiesce_checks : ctx->search_vquiesce_checks};
  if (set.quiesce > 0 && nrec > 0xFFFFFFFFu) return fail(FNNUE_E_ARG, "batch too large");
  const StarGroups l1{ws.p[BuilderScratch::kStates], (uint32_t)nply, kids.off, (uint32_t)nrec, kids.moves, kids.end, ps, po};
  DrawHistory hist;
  if (rules.chess() ? ctx->search_draws : ctx->search_vdraws) {  // the plies' history from the boards the replay left
    if ((rc = draw_history_level1(rules, d_text, d_fen_off, d_moves_off, kids.ply_off, (uint32_t)ngames, l1.states, l1.n, l1.off,
                                  l1.moves, l1.end, s, ws, &hist, nullptr)))
      return rc;
    set.draws = &hist;
  }
  if ((rc = reduce_level1(ctx, ws, rules, set, l1, d_out, nullptr, k, k ? d_lines : nullptr, lines_cap, s, nullptr))) return rc;
  HIP_TRY(hipMemcpyAsync(d_off, kids.ply_off, (ngames + 1) * 4, hipMemcpyDeviceToDevice, s), "D2D(offsets)");
  return FNNUE_OK;
}

// The host-buffer forms: staged through the ctx's stream.
int search1_host(fnnue_ctx* ctx, int variant, const char* text, size_t text_len, const uint32_t* fen_off,
                 const uint32_t* moves_off, size_t ngames, uint32_t k, fnnue_best* out, size_t cap, uint32_t* off,
                 size_t off_cap, fnnue_line* lines, size_t lines_cap, size_t* n_out, size_t* n_groups) {
  if (!ctx || !n_out || !n_groups || (ngames && (!text || !fen_off || !moves_off)))
    return fail(FNNUE_E_ARG, "null argument");
  *n_out = *n_groups = 0;
  if (int rc = search1_arch(ctx, variant)) return rc;
  if (ngames == 0) return FNNUE_OK;
  DeviceGuard g(ctx->device);
  StagedGames d;
  int rc = stage_games(ctx, text, text_len, fen_off, moves_off, ngames, &d);
  if (rc) return rc;
  const bool room = out && off && off_cap >= ngames + 1 && (!k || lines);
  // [best | lines | off]: the lines' room is cut to whole plies the records have room for
  const size_t nl = k ? std::min(lines_cap / k, cap) * k : 0;
  fnnue_best* d_out;
  fnnue_line* d_lines;
  uint32_t* d_off;
  TempDev buf;
  buf.part(&d_out, cap), buf.part(&d_lines, nl), buf.part(&d_off, ngames + 1);
  if (room && (rc = buf.get())) return rc;
  if (!k) d_lines = nullptr;
  hipStream_t s = ctx->stream;
  rc = search1_device(ctx, variant, d.text, d.fen_off, d.moves_off, ngames, k, d_out, room ? cap : 0, d_off, room ? off_cap : 0,
                      d_lines, room ? nl : 0, n_out, n_groups, s);
  if (rc) return rc;
  HIP_TRY(hipMemcpyAsync(out, d_out, *n_out * sizeof(fnnue_best), hipMemcpyDeviceToHost, s), "D2H");
  if (k) HIP_TRY(hipMemcpyAsync(lines, d_lines, *n_out * k * sizeof(fnnue_line), hipMemcpyDeviceToHost, s), "D2H");
  HIP_TRY(hipMemcpyAsync(off, d_off, (ngames + 1) * 4, hipMemcpyDeviceToHost, s), "D2H");
  HIP_TRY(hipStreamSynchronize(s), "hipStreamSynchronize");
  return latched(ctx);
}

}  // namespace

extern "C" {

int fnnue_search1_device(fnnue_ctx* ctx, const char* d_text, const uint32_t* d_fen_off, const uint32_t* d_moves_off,
                         size_t ngames, fnnue_best* d_out, size_t cap, uint32_t* d_off, size_t off_cap, size_t* n_out,
                         size_t* n_groups, void* stream) {
  return search1_device(ctx, kVariantChess, d_text, d_fen_off, d_moves_off, ngames, 0, d_out, cap, d_off, off_cap, nullptr, 0, n_out,
                        n_groups, stream);
}

int fnnue_search1_lines_device(fnnue_ctx* ctx, const char* d_text, const uint32_t* d_fen_off,
                               const uint32_t* d_moves_off, size_t ngames, uint32_t k, fnnue_best* d_out, size_t cap,
                               uint32_t* d_off, size_t off_cap, fnnue_line* d_lines, size_t lines_cap, size_t* n_out,
                               size_t* n_groups, void* stream) {
  if (k < 1 || k > FNNUE_MAX_CHILDREN) return fail(FNNUE_E_ARG, "k must be 1.." + std::to_string(FNNUE_MAX_CHILDREN));
  return search1_device(ctx, kVariantChess, d_text, d_fen_off, d_moves_off, ngames, k, d_out, cap, d_off, off_cap, d_lines, lines_cap,
                        n_out, n_groups, stream);
}

int fnnue_search1_lines(fnnue_ctx* ctx, const char* text, size_t text_len, const uint32_t* fen_off,
                        const uint32_t* moves_off, size_t ngames, uint32_t k, fnnue_best* out, size_t cap,
                        uint32_t* off, size_t off_cap, fnnue_line* lines, size_t lines_cap, size_t* n_out,
                        size_t* n_groups) {
  if (k < 1 || k > FNNUE_MAX_CHILDREN) return fail(FNNUE_E_ARG, "k must be 1.." + std::to_string(FNNUE_MAX_CHILDREN));
  return search1_host(ctx, kVariantChess, text, text_len, fen_off, moves_off, ngames, k, out, cap, off, off_cap, lines, lines_cap,
                      n_out, n_groups);
}

int fnnue_search1(fnnue_ctx* ctx, const char* text, size_t text_len, const uint32_t* fen_off,
                  const uint32_t* moves_off, size_t ngames, fnnue_best* out, size_t cap, uint32_t* off, size_t off_cap,
                  size_t* n_out, size_t* n_groups) {
  return search1_host(ctx, kVariantChess, text, text_len, fen_off, moves_off, ngames, 0, out, cap, off, off_cap, nullptr, 0, n_out,
                      n_groups);
}

}  // extern "C"

namespace {

// fnnue_[v]best_replies_device (topk = false: one fnnue_best2 per group into
// d_out) and fnnue_[v]topk_replies_device (the ranked lines into d_lines): the
// groups' first entries in d_child_best (a caller's groups may be empty) go to
// the context's scratch, then the one kernel or the other.
int replies_device(fnnue_ctx* ctx, bool vranks, bool topk, const uint8_t* d_end, const fnnue_move* d_moves,
                   const uint32_t* d_off, size_t ngroups, size_t npos, const fnnue_best* d_child_best,
                   fnnue_best2* d_out, const uint32_t* d_line_off, fnnue_line2* d_lines, size_t lines_cap,
                   void* stream) {
  if (!ctx) return fail(FNNUE_E_ARG, "null ctx");
  if (ngroups == 0) return FNNUE_OK;
  if (!d_end || !d_off || !d_child_best || (topk ? !d_line_off || (lines_cap && !d_lines) : !d_out))
    return fail(FNNUE_E_ARG, "null buffer");
  if (ngroups > 0xFFFFFFFEu || npos > 0xFFFFFFFFu) return fail(FNNUE_E_ARG, "batch too large");
  if (topk && lines_cap == 0) return FNNUE_OK;  // no slot may be written
  DeviceGuard g(ctx->device);
  hipStream_t s = stream ? static_cast<hipStream_t>(stream) : ctx->stream;
  int rc = order_workspace(ctx, s);
  if (rc) return rc;
  WorkspaceUse use{ctx, s};
  uint32_t *cnt = nullptr, *base = nullptr;
  HIP_TRY(ctx->bscratch.get(BuilderScratch::kKidCnt, (ngroups + 1) * 4, (void**)&cnt), "device allocation (scratch)");
  HIP_TRY(ctx->bscratch.get(BuilderScratch::kKidOff, (ngroups + 1) * 4, (void**)&base), "device allocation (scratch)");
  HIP_TRY(launch_child_counts(d_off, (uint32_t)ngroups, (uint32_t)npos, cnt, s), "child_counts launch");
  HIP_TRY(builder_exclusive_scan(cnt, base, (uint32_t)ngroups, s, ctx->bscratch), "scan");
  if (topk)
    HIP_TRY(topk_replies(vranks, d_end, d_moves, d_off, (uint32_t)ngroups, (uint32_t)npos, d_child_best, base,
                         d_line_off, 0, d_lines, lines_cap, s),
            "topk_replies launch");
  else
    HIP_TRY(best_replies(vranks, d_end, d_moves, d_off, (uint32_t)ngroups, (uint32_t)npos, d_child_best, base, d_out, s),
            "best_replies launch");
  return FNNUE_OK;
}

// Their host-buffer forms.  topk: the caller's lines go up first, so that slots
// no group writes (empty groups) come back as they were.
int replies_host(fnnue_ctx* ctx, bool vranks, bool topk, const uint8_t* end, const fnnue_move* moves,
                 const uint32_t* off, size_t ngroups, size_t npos, const fnnue_best* child_best, fnnue_best2* out,
                 const uint32_t* line_off, fnnue_line2* lines, size_t lines_cap) {
  if (!ctx) return fail(FNNUE_E_ARG, "null ctx");
  if (ngroups == 0) return FNNUE_OK;
  if (!off || (topk ? !line_off : !out) || (npos && !end)) return fail(FNNUE_E_ARG, "null buffer");
  if (ngroups > 0xFFFFFFFEu || npos > 0xFFFFFFFFu) return fail(FNNUE_E_ARG, "batch too large");
  size_t nl = 0;
  if (topk) {
    for (size_t g = 0; g < ngroups; ++g)
      if (line_off[g] > line_off[g + 1]) return fail(FNNUE_E_ARG, "line offsets decrease");
    nl = line_off[ngroups];
    if (nl > lines_cap) return fail(FNNUE_E_CAPACITY, "line buffer too small");
    if (nl && !lines) return fail(FNNUE_E_ARG, "null buffer");
  }
  size_t nchild = 0;  // as the kernel clamps the offsets
  for (size_t i = 0; i < ngroups; ++i) {
    const size_t e = std::min<size_t>(off[i + 1], npos), o = std::min<size_t>(off[i], e);
    if (e > o) nchild += e - o - 1;
  }
  if (nchild && !child_best) return fail(FNNUE_E_ARG, "null buffer");
  if (topk && nl == 0) return FNNUE_OK;
  DeviceGuard g(ctx->device);
  fnnue_best* d_cb;
  uint32_t *d_off, *d_loff;
  fnnue_best2* d_out;
  fnnue_line2* d_lines;
  fnnue_move* d_mv;
  uint8_t* d_end;
  TempDev buf;  // [child_best | off | out, or line_off | lines | moves | end]
  buf.part(&d_cb, nchild + 1), buf.part(&d_off, ngroups + 1);
  buf.part(&d_out, topk ? 0 : ngroups), buf.part(&d_loff, topk ? ngroups + 1 : 0), buf.part(&d_lines, nl);
  buf.part(&d_mv, npos), buf.part(&d_end, npos);
  if (int rc = buf.get()) return rc;
  if (!moves) d_mv = nullptr;
  hipStream_t s = ctx->stream;
  if (nchild) HIP_TRY(hipMemcpyAsync(d_cb, child_best, nchild * sizeof(fnnue_best), hipMemcpyHostToDevice, s), "H2D");
  if (npos) {
    HIP_TRY(hipMemcpyAsync(d_end, end, npos, hipMemcpyHostToDevice, s), "H2D");
    if (moves) HIP_TRY(hipMemcpyAsync(d_mv, moves, npos * 2, hipMemcpyHostToDevice, s), "H2D");
  }
  HIP_TRY(hipMemcpyAsync(d_off, off, (ngroups + 1) * 4, hipMemcpyHostToDevice, s), "H2D");
  if (topk) {
    HIP_TRY(hipMemcpyAsync(d_loff, line_off, (ngroups + 1) * 4, hipMemcpyHostToDevice, s), "H2D");
    HIP_TRY(hipMemcpyAsync(d_lines, lines, nl * sizeof(fnnue_line2), hipMemcpyHostToDevice, s), "H2D");
  }
  const int rc = replies_device(ctx, vranks, topk, d_end, d_mv, d_off, ngroups, npos, d_cb, d_out, d_loff, d_lines, nl, s);
  if (rc) return rc;
  if (topk)
    HIP_TRY(hipMemcpyAsync(lines, d_lines, nl * sizeof(fnnue_line2), hipMemcpyDeviceToHost, s), "D2H");
  else
    HIP_TRY(hipMemcpyAsync(out, d_out, ngroups * sizeof(fnnue_best2), hipMemcpyDeviceToHost, s), "D2H");
  HIP_TRY(hipStreamSynchronize(s), "hipStreamSynchronize");
  return FNNUE_OK;
}

}  // namespace

extern "C" {

int fnnue_topk_replies_device(fnnue_ctx* ctx, const uint8_t* d_end, const fnnue_move* d_moves, const uint32_t* d_off,
                              size_t ngroups, size_t npos, const fnnue_best* d_child_best, const uint32_t* d_line_off,
                              fnnue_line2* d_lines, size_t lines_cap, void* stream) {
  return replies_device(ctx, false, true, d_end, d_moves, d_off, ngroups, npos, d_child_best, nullptr, d_line_off, d_lines,
                        lines_cap, stream);
}

int fnnue_topk_replies(fnnue_ctx* ctx, const uint8_t* end, const fnnue_move* moves, const uint32_t* off, size_t ngroups,
                       size_t npos, const fnnue_best* child_best, const uint32_t* line_off, fnnue_line2* lines,
                       size_t lines_cap) {
  return replies_host(ctx, false, true, end, moves, off, ngroups, npos, child_best, nullptr, line_off, lines, lines_cap);
}

int fnnue_vtopk_replies_device(fnnue_ctx* ctx, const uint8_t* d_end, const fnnue_move* d_moves, const uint32_t* d_off,
                               size_t ngroups, size_t npos, const fnnue_best* d_child_best, const uint32_t* d_line_off,
                               fnnue_line2* d_lines, size_t lines_cap, void* stream) {
  return replies_device(ctx, true, true, d_end, d_moves, d_off, ngroups, npos, d_child_best, nullptr, d_line_off, d_lines,
                        lines_cap, stream);
}

int fnnue_vtopk_replies(fnnue_ctx* ctx, const uint8_t* end, const fnnue_move* moves, const uint32_t* off,
                        size_t ngroups, size_t npos, const fnnue_best* child_best, const uint32_t* line_off,
                        fnnue_line2* lines, size_t lines_cap) {
  return replies_host(ctx, true, true, end, moves, off, ngroups, npos, child_best, nullptr, line_off, lines, lines_cap);
}

int fnnue_best_replies_device(fnnue_ctx* ctx, const uint8_t* d_end, const fnnue_move* d_moves, const uint32_t* d_off,
                              size_t ngroups, size_t npos, const fnnue_best* d_child_best, fnnue_best2* d_out,
                              void* stream) {
  return replies_device(ctx, false, false, d_end, d_moves, d_off, ngroups, npos, d_child_best, d_out, nullptr, nullptr, 0,
                        stream);
}

int fnnue_best_replies(fnnue_ctx* ctx, const uint8_t* end, const fnnue_move* moves, const uint32_t* off,
                       size_t ngroups, size_t npos, const fnnue_best* child_best, fnnue_best2* out) {
  return replies_host(ctx, false, false, end, moves, off, ngroups, npos, child_best, out, nullptr, nullptr, 0);
}

int fnnue_vbest_replies_device(fnnue_ctx* ctx, const uint8_t* d_end, const fnnue_move* d_moves, const uint32_t* d_off,
                               size_t ngroups, size_t npos, const fnnue_best* d_child_best, fnnue_best2* d_out,
                               void* stream) {
  return replies_device(ctx, true, false, d_end, d_moves, d_off, ngroups, npos, d_child_best, d_out, nullptr, nullptr, 0,
                        stream);
}

int fnnue_vbest_replies(fnnue_ctx* ctx, const uint8_t* end, const fnnue_move* moves, const uint32_t* off,
                        size_t ngroups, size_t npos, const fnnue_best* child_best, fnnue_best2* out) {
  return replies_host(ctx, true, false, end, moves, off, ngroups, npos, child_best, out, nullptr, nullptr, 0);
}

}  // extern "C"

namespace {

// One ply's most records two plies down: 218 children of 1 + 218 records each.
constexpr size_t kSearch2MinRecords = (size_t)(FNNUE_MAX_CHILDREN + 1) * (FNNUE_MAX_CHILDREN + 1);

size_t search2_budget() {
  size_t n = (size_t)16 << 20;
  if (const char* e = std::getenv("FNNUE_SEARCH2_RECORDS")) n = (size_t)std::max(0LL, std::atoll(e));
  return std::min<size_t>(std::max(n, kSearch2MinRecords), 0xFFFFFFFFu);
}

// FNNUE_SEARCH2_TRACE=1 in the environment (read per call): HIP events between
// the phases of a fnnue_search2 call; the call then waits for its work and
// prints the phases' device times to stderr, one JSON line — diagnostics only
// (tools/search2_bench.py).
struct Search2Trace {
  bool on = false;
  hipStream_t s = nullptr;
  std::vector<std::pair<int, hipEvent_t>> marks;
  Search2Trace(hipStream_t stream) : s(stream) {
    const char* e = std::getenv("FNNUE_SEARCH2_TRACE");
    on = e && *e && *e != '0';
  }
  void mark(int phase) {  // SearchPhase `phase` starts here (kSearchPhases: the end)
    if (!on) return;
    hipEvent_t ev = nullptr;
    if (hipEventCreate(&ev) != hipSuccess || hipEventRecord(ev, s) != hipSuccess) on = false;
    if (ev) marks.emplace_back(phase, ev);
  }
  // the shared steps' marks (search_steps.h)
  PhaseHook hook() { return {[](void* t, int phase) { static_cast<Search2Trace*>(t)->mark(phase); }, this}; }
  long listed = -1;  // the plies on the draw rules' list (read back for the report only)
  int quiesce = 0;   // the quiescence depth, with what the levels held and the slices of leaves
  bool quiesce_checks = false;  // with the evasion records and the nodes in check per level
  QuiesceStats qstats;
  void report(size_t plies, size_t kids, size_t records, size_t chunks) {
    static const char* const kName[kSearchPhases] = {"level1", "child_states", "count", "expand", "eval", "reduce1",
                                                     "reduce2", "topk", "history", "mark", "quiesce"};
    if (on && !marks.empty() && hipEventSynchronize(marks.back().second) == hipSuccess) {
      double ms[kSearchPhases] = {};
      for (size_t i = 0; i + 1 < marks.size(); ++i) {
        float t = 0;
        if (hipEventElapsedTime(&t, marks[i].second, marks[i + 1].second) == hipSuccess) ms[marks[i].first] += t;
      }
      std::string line = "FNNUE_SEARCH2_TRACE {\"plies\":" + std::to_string(plies) + ",\"children\":" +
                         std::to_string(kids) + ",\"grandchild_records\":" + std::to_string(records) +
                         ",\"chunks\":" + std::to_string(chunks);
      if (listed >= 0) line += ",\"draw_list\":" + std::to_string(listed);
      if (quiesce > 0) {
        line += ",\"quiesce\":" + std::to_string(quiesce) + ",\"quiesce_slices\":" + std::to_string(qstats.slices) +
                ",\"quiesce_records\":[";
        for (int l = 0; l < quiesce; ++l) line += (l ? "," : "") + std::to_string(qstats.level_records[l]);
        if (quiesce_checks) {
          line += "],\"quiesce_evasions\":[";
          for (int l = 0; l < quiesce; ++l) line += (l ? "," : "") + std::to_string(qstats.level_evasions[l]);
          line += "],\"quiesce_in_check\":[";
          for (int l = 0; l < quiesce; ++l) line += (l ? "," : "") + std::to_string(qstats.level_in_check[l]);
        }
        line += "],\"quiesce_redone\":" + std::to_string(qstats.redone) + ",\"quiesce_roots_ms\":" +
                std::to_string(qstats.roots_ms) + ",\"quiesce_gen_ms\":" + std::to_string(qstats.gen_ms) +
                ",\"quiesce_eval_ms\":" + std::to_string(qstats.eval_ms) + ",\"quiesce_reduce_ms\":" +
                std::to_string(qstats.reduce_ms);
      }
      for (int k = 0; k < kSearchPhases; ++k) line += std::string(",\"") + kName[k] + "_ms\":" + std::to_string(ms[k]);
      std::fprintf(stderr, "%s}\n", line.c_str());
    }
  }
  ~Search2Trace() {
    for (auto& m : marks) (void)hipEventDestroy(m.second);
  }
};

// The net a two-ply search of `variant` needs: fnnue_search2* (vcall = false) a
// chess net, fnnue_vsearch2* fnnue_vsearch1's (never a chess context).
int search2_arch(const fnnue_ctx* ctx, int variant, bool vcall) {
  if (!vcall)
    return ctx->variant == kVariantChess ? (int)FNNUE_OK : fail(FNNUE_E_ARCH, "the two-ply search needs a chess net");
  if (ctx->variant == kVariantChess || variant == kVariantChess)
    return fail(FNNUE_E_ARCH, "the variant two-ply search needs a variant net");
  return search1_arch(ctx, variant);
}

// The variant entry points hand their counts back zeroed on every error path, a null context included.
void zero_counts(size_t* n_out, size_t* n_groups, size_t* n_children) {
  if (n_out) *n_out = 0;
  if (n_groups) *n_groups = 0;
  if (n_children) *n_children = 0;
}

// fnnue_search2_device (variant = chess) and fnnue_vsearch2_device; with
// d_child_best / d_child_map (child_cap entries each) also the children's
// depth-1 records (fnnue_[v]search2_children); with k >= 1 also ply p's k best
// lines at d_lines[p * k ..] (fnnue_[v]search2_lines_device): one more kernel
// behind the second reduction, over the same arrays.
int search2_device(fnnue_ctx* ctx, int variant, bool vcall, const char* d_text, const uint32_t* d_fen_off, const uint32_t* d_moves_off,
                   size_t ngames, fnnue_best2* d_out, size_t cap, uint32_t* d_off, size_t off_cap,
                   fnnue_best* d_child_best, uint32_t* d_child_map, size_t child_cap, size_t* n_out, size_t* n_groups,
                   size_t* n_children, void* stream, uint32_t k = 0, fnnue_line2* d_lines = nullptr,
                   size_t lines_cap = 0) {
  if (!ctx || !n_out || !n_groups) return fail(FNNUE_E_ARG, "null argument");
  *n_out = *n_groups = 0;
  if (n_children) *n_children = 0;
  if (int rc = search2_arch(ctx, variant, vcall)) return rc;
  if (ngames == 0) return FNNUE_OK;
  const SearchRules rules{variant};
  DeviceGuard g(ctx->device);
  hipStream_t s = stream ? static_cast<hipStream_t>(stream) : ctx->stream;
  int rc = order_workspace(ctx, s);
  if (rc) return rc;
  WorkspaceUse use{ctx, s};
  using W = BuilderScratch;
  W& ws = ctx->bscratch;
  Search2Trace trace(s);
  const PhaseHook hook = trace.hook();
  trace.mark(kPhaseLevel1);
  // level 1: the plies' boards (scratch) and their STAR groups' offsets, moves and end flags
  size_t max_plies = d_out && d_off && off_cap >= ngames + 1 ? cap : 0;
  if (k) max_plies = d_lines ? std::min(max_plies, lines_cap / k) : 0;
  Level1 kids{max_plies};
  size_t nrec = 0, nply = 0;
  rc = build_device(ctx, variant, d_text, d_fen_off, d_moves_off, ngames, true, nullptr, 0, nullptr, 0, nullptr, nullptr,
                    &nrec, &nply, s, &kids);
  *n_out = nply;
  *n_groups = nply || rc == FNNUE_OK ? ngames : 0;
  if (rc) return rc;
  if (nrec > 0xFFFFFFFFu) return fail(FNNUE_E_ARG, "batch too large");
  const size_t nkid = nrec - nply;
  if (n_children) *n_children = nkid;
  if (n_children && (nkid > child_cap || (nkid && (!d_child_best || !d_child_map))))
    return fail(FNNUE_E_CAPACITY, "child buffers too small");
  const StarGroups l1{ws.p[W::kStates], (uint32_t)nply, kids.off, (uint32_t)nrec, kids.moves, kids.end, nullptr, nullptr};
  char* kid_states = nullptr;
  uint32_t *kid_cnt = nullptr, *kid_off = nullptr, *spans = nullptr;
  fnnue_best* kid_best = nullptr;
  HIP_TRY(ws.get(W::kKidStates, (nkid + 1) * rules.state_bytes(), (void**)&kid_states), "device allocation (search scratch)");
  HIP_TRY(ws.get(W::kKidCnt, (nkid + 1) * 4, (void**)&kid_cnt), "device allocation (search scratch)");
  HIP_TRY(ws.get(W::kKidOff, (nkid + 1) * 4, (void**)&kid_off), "device allocation (search scratch)");
  HIP_TRY(ws.get(W::kKidBest, (nkid + 1) * sizeof(fnnue_best), (void**)&kid_best), "device allocation (search scratch)");
  HIP_TRY(ws.get(W::kPlySpans, (nply + 1) * 8, (void**)&spans), "device allocation (search scratch)");
  // the second reduction over the whole call, then the lines (every slot all-zero when no ply has a child)
  auto reduce = [&]() -> int {
    trace.mark(kPhaseReduce2);
    HIP_TRY(best_replies(rules.vranks(), l1.end, l1.moves, l1.off, l1.n, l1.total, kid_best, nullptr, d_out, s),
            "best_replies launch");
    if (k) {
      trace.mark(kPhaseTopk);
      HIP_TRY(topk_replies(rules.vranks(), l1.end, l1.moves, l1.off, l1.n, l1.total, kid_best, nullptr, nullptr, k,
                           d_lines, lines_cap, s),
              "topk_replies launch");
    }
    trace.mark(kSearchPhases);
    return FNNUE_OK;
  };
  if (nkid == 0) {  // every ply is a finished game's last
    if ((rc = reduce())) return rc;
    HIP_TRY(hipMemcpyAsync(d_off, kids.ply_off, (ngames + 1) * 4, hipMemcpyDeviceToDevice, s), "D2D(offsets)");
    return FNNUE_OK;
  }
  // The draw rules (fnnue_set_search_draws, a variant: fnnue_set_search_vdraws): the plies' history
  // and the marks on the listed plies' children here, their grandchildren per chunk.
  SearchSettings set{nullptr, rules.chess() ? ctx->search_quiesce : ctx->search_vquiesce,
                     rules.chess() ? ctx->search_quiesce_checks : ctx->search_vquiesce_checks};
  DrawHistory hist;
  if (rules.chess() ? ctx->search_draws : ctx->search_vdraws) {
    if ((rc = draw_history_level1(rules, d_text, d_fen_off, d_moves_off, kids.ply_off, (uint32_t)ngames, l1.states, l1.n,
                                  l1.off, l1.moves, l1.end, s, ws, &hist, &hook)))
      return rc;
    set.draws = &hist;
  }
  trace.quiesce = set.quiesce;
  trace.quiesce_checks = set.quiesce_checks;
  trace.qstats.timed = trace.on;
  trace.mark(kPhaseChildStates);
  HIP_TRY(child_states(rules, l1.states, l1.n, l1.off, l1.total, kid_states, reinterpret_cast<uint2*>(d_child_map), s),
          "child_states launch");
  // level 2 sizes: every child's records, and per ply where its children and their records start
  trace.mark(kPhaseCount);
  HIP_TRY(count_children(rules, kid_states, (uint32_t)nkid, kid_cnt, kid_off, s, ws), "children count");
  HIP_TRY(ply_spans_device(kids.off, kid_off, (uint32_t)nply, spans, spans + nply + 1, s), "ply_spans launch");
  std::vector<uint32_t> h((nply + 1) * 2);
  HIP_TRY(hipMemcpyAsync(h.data(), spans, h.size() * 4, hipMemcpyDeviceToHost, s), "D2H(sizes)");
  HIP_TRY(hipStreamSynchronize(s), "hipStreamSynchronize");
  const uint32_t *first_kid = h.data(), *first_rec = h.data() + nply + 1;
  // chunks of whole plies within the budget; a ply larger than the budget (a
  // crazyhouse ply has no fixed bound) is a chunk of its own.  One ply's records
  // are the 32-bit difference of two offsets, as the device takes it (a ply's
  // children times their children: far below 2^32); a chunk's are their sum in
  // 64 bits, so a call whose grandchild records pass 2^32 in all still cuts
  // right and runs chunk by chunk, and no chunk's count wraps (budget < 2^32).
  const size_t budget = search2_budget();
  std::vector<uint32_t> cuts{0};
  size_t max_rec = 0, max_kid = 0, all_rec = 0;
  for (size_t p = 0; p < nply;) {
    size_t q = p + 1;
    uint64_t sum = (uint32_t)(first_rec[q] - first_rec[p]);
    while (q < nply && sum + (uint32_t)(first_rec[q + 1] - first_rec[q]) <= budget) {
      sum += (uint32_t)(first_rec[q + 1] - first_rec[q]);
      ++q;
    }
    max_rec = std::max<size_t>(max_rec, sum);
    all_rec += sum;
    max_kid = std::max<size_t>(max_kid, first_kid[q] - first_kid[p]);
    cuts.push_back((uint32_t)q);
    p = q;
  }
  Level2Chunk c;
  uint32_t* ch_off = nullptr;
  HIP_TRY(ws.get(W::kChunkOff, (max_kid + 1) * 4, (void**)&ch_off), "device allocation (search scratch)");
  HIP_TRY(ws.get(W::kGrand, max_rec * rules.record_bytes(), &c.pos), "device allocation (search scratch)");
  HIP_TRY(ws.get(W::kGrandMoves, max_rec * 2, (void**)&c.moves), "device allocation (search scratch)");
  HIP_TRY(ws.get(W::kGrandEnd, max_rec, (void**)&c.end), "device allocation (search scratch)");
  HIP_TRY(ws.get(W::kGrandPsqt, max_rec * 4, (void**)&c.psqt), "device allocation (search scratch)");
  HIP_TRY(ws.get(W::kGrandPositional, max_rec * 4, (void**)&c.positional), "device allocation (search scratch)");
  c.ch_off = ch_off;
  for (size_t i = 0; i + 1 < cuts.size(); ++i) {
    c.p0 = cuts[i], c.p1 = cuts[i + 1];
    c.k0 = first_kid[c.p0], c.nk = first_kid[c.p1] - c.k0;
    c.rec0 = first_rec[c.p0], c.nr = first_rec[c.p1] - c.rec0;
    if (c.nk == 0) continue;  // plies without a legal move
    trace.mark(kPhaseExpand);
    HIP_TRY(rebase_offsets_device(kid_off + c.k0, c.nk + 1, ch_off, s), "rebase_offsets launch");
    if ((rc = search_level2_chunk(ctx, ws, rules, set, l1, kid_states, kid_off, c, kid_best, s, &trace.qstats, &hook)))
      return rc;
  }
  if ((rc = reduce())) return rc;
  if (set.draws && trace.on) {
    uint32_t listed = 0;
    HIP_TRY(hipMemcpyAsync(&listed, hist.list, 4, hipMemcpyDeviceToHost, s), "D2H(draw list)");
    HIP_TRY(hipStreamSynchronize(s), "hipStreamSynchronize");
    trace.listed = (long)listed;
  }
  trace.report(nply, nkid, all_rec, cuts.size() - 1);
  if (n_children && nkid)
    HIP_TRY(hipMemcpyAsync(d_child_best, kid_best, nkid * sizeof(fnnue_best), hipMemcpyDeviceToDevice, s),
            "D2D(children)");
  HIP_TRY(hipMemcpyAsync(d_off, kids.ply_off, (ngames + 1) * 4, hipMemcpyDeviceToDevice, s), "D2D(offsets)");
  return FNNUE_OK;
}

int search2_host(fnnue_ctx* ctx, int variant, bool vcall, const char* text, size_t text_len, const uint32_t* fen_off, const uint32_t* moves_off,
                 size_t ngames, fnnue_best2* out, size_t cap, uint32_t* off, size_t off_cap, fnnue_best* child_best,
                 uint32_t* child_map, size_t child_cap, size_t* n_out, size_t* n_groups, size_t* n_children,
                 uint32_t k = 0, fnnue_line2* lines = nullptr, size_t lines_cap = 0) {
  if (!ctx || !n_out || !n_groups || (ngames && (!text || !fen_off || !moves_off)))
    return fail(FNNUE_E_ARG, "null argument");
  *n_out = *n_groups = 0;
  if (n_children) *n_children = 0;
  if (int rc = search2_arch(ctx, variant, vcall)) return rc;
  if (ngames == 0) return FNNUE_OK;
  DeviceGuard g(ctx->device);
  StagedGames d;
  int rc = stage_games(ctx, text, text_len, fen_off, moves_off, ngames, &d);
  if (rc) return rc;
  const bool room = out && off && off_cap >= ngames + 1 && (!k || lines);
  const bool kroom = n_children && child_best && child_map;
  if (!kroom) child_cap = 0;
  // the lines' room is cut to whole plies the records have room for
  const size_t nl = k ? std::min(lines_cap / k, cap) * k : 0;
  fnnue_best2* d_out;
  fnnue_best* d_cb;
  uint2* d_cm;
  fnnue_line2* d_lines;
  uint32_t* d_off;
  TempDev buf;  // [best2 | child_best | child_map | lines | off]
  buf.part(&d_out, cap), buf.part(&d_cb, child_cap), buf.part(&d_cm, child_cap), buf.part(&d_lines, nl);
  buf.part(&d_off, ngames + 1);
  if (room && (rc = buf.get())) return rc;
  if (!kroom) d_cb = nullptr, d_cm = nullptr;
  if (!k) d_lines = nullptr;
  hipStream_t s = ctx->stream;
  rc = search2_device(ctx, variant, vcall, d.text, d.fen_off, d.moves_off, ngames, d_out, room ? cap : 0, d_off, room ? off_cap : 0,
                      d_cb, reinterpret_cast<uint32_t*>(d_cm), room ? child_cap : 0, n_out, n_groups, n_children, s, k,
                      d_lines, room ? nl : 0);
  if (rc) return rc;
  HIP_TRY(hipMemcpyAsync(out, d_out, *n_out * sizeof(fnnue_best2), hipMemcpyDeviceToHost, s), "D2H");
  if (k) HIP_TRY(hipMemcpyAsync(lines, d_lines, *n_out * k * sizeof(fnnue_line2), hipMemcpyDeviceToHost, s), "D2H");
  if (n_children && *n_children) {
    HIP_TRY(hipMemcpyAsync(child_best, d_cb, *n_children * sizeof(fnnue_best), hipMemcpyDeviceToHost, s), "D2H");
    HIP_TRY(hipMemcpyAsync(child_map, d_cm, *n_children * 8, hipMemcpyDeviceToHost, s), "D2H");
  }
  HIP_TRY(hipMemcpyAsync(off, d_off, (ngames + 1) * 4, hipMemcpyDeviceToHost, s), "D2H");
  HIP_TRY(hipStreamSynchronize(s), "hipStreamSynchronize");
  return latched(ctx);
}

}  // namespace

extern "C" {

int fnnue_search2_device(fnnue_ctx* ctx, const char* d_text, const uint32_t* d_fen_off, const uint32_t* d_moves_off,
                         size_t ngames, fnnue_best2* d_out, size_t cap, uint32_t* d_off, size_t off_cap, size_t* n_out,
                         size_t* n_groups, void* stream) {
  return search2_device(ctx, kVariantChess, false, d_text, d_fen_off, d_moves_off, ngames, d_out, cap, d_off, off_cap,
                        nullptr, nullptr, 0, n_out, n_groups, nullptr, stream);
}

int fnnue_search2(fnnue_ctx* ctx, const char* text, size_t text_len, const uint32_t* fen_off,
                  const uint32_t* moves_off, size_t ngames, fnnue_best2* out, size_t cap, uint32_t* off, size_t off_cap,
                  size_t* n_out, size_t* n_groups) {
  return search2_host(ctx, kVariantChess, false, text, text_len, fen_off, moves_off, ngames, out, cap, off, off_cap,
                      nullptr, nullptr, 0, n_out, n_groups, nullptr);
}

int fnnue_search2_children(fnnue_ctx* ctx, const char* text, size_t text_len, const uint32_t* fen_off,
                           const uint32_t* moves_off, size_t ngames, fnnue_best2* out, size_t cap, uint32_t* off,
                           size_t off_cap, fnnue_best* child_best, uint32_t* child_map, size_t child_cap,
                           size_t* n_out, size_t* n_groups, size_t* n_children) {
  if (!n_children) return fail(FNNUE_E_ARG, "null argument");
  return search2_host(ctx, kVariantChess, false, text, text_len, fen_off, moves_off, ngames, out, cap, off, off_cap,
                      child_best, child_map, child_cap, n_out, n_groups, n_children);
}

int fnnue_vsearch2_device(fnnue_ctx* ctx, int variant, const char* d_text, const uint32_t* d_fen_off,
                          const uint32_t* d_moves_off, size_t ngames, fnnue_best2* d_out, size_t cap, uint32_t* d_off,
                          size_t off_cap, size_t* n_out, size_t* n_groups, void* stream) {
  zero_counts(n_out, n_groups, nullptr);
  return search2_device(ctx, variant, true, d_text, d_fen_off, d_moves_off, ngames, d_out, cap, d_off, off_cap,
                        nullptr, nullptr, 0, n_out, n_groups, nullptr, stream);
}

int fnnue_vsearch2(fnnue_ctx* ctx, int variant, const char* text, size_t text_len, const uint32_t* fen_off,
                   const uint32_t* moves_off, size_t ngames, fnnue_best2* out, size_t cap, uint32_t* off,
                   size_t off_cap, size_t* n_out, size_t* n_groups) {
  zero_counts(n_out, n_groups, nullptr);
  return search2_host(ctx, variant, true, text, text_len, fen_off, moves_off, ngames, out, cap, off, off_cap, nullptr,
                      nullptr, 0, n_out, n_groups, nullptr);
}

int fnnue_vsearch2_children(fnnue_ctx* ctx, int variant, const char* text, size_t text_len, const uint32_t* fen_off,
                            const uint32_t* moves_off, size_t ngames, fnnue_best2* out, size_t cap, uint32_t* off,
                            size_t off_cap, fnnue_best* child_best, uint32_t* child_map, size_t child_cap,
                            size_t* n_out, size_t* n_groups, size_t* n_children) {
  zero_counts(n_out, n_groups, n_children);
  if (!n_children) return fail(FNNUE_E_ARG, "null argument");
  return search2_host(ctx, variant, true, text, text_len, fen_off, moves_off, ngames, out, cap, off, off_cap,
                      child_best, child_map, child_cap, n_out, n_groups, n_children);
}

static int lines2_k(uint32_t k, size_t* n_out, size_t* n_groups) {
  zero_counts(n_out, n_groups, nullptr);
  if (k < 1 || k > FNNUE_MAX_CHILDREN) return fail(FNNUE_E_ARG, "k must be 1.." + std::to_string(FNNUE_MAX_CHILDREN));
  return FNNUE_OK;
}

int fnnue_search2_lines_device(fnnue_ctx* ctx, const char* d_text, const uint32_t* d_fen_off,
                               const uint32_t* d_moves_off, size_t ngames, uint32_t k, fnnue_best2* d_out, size_t cap,
                               uint32_t* d_off, size_t off_cap, fnnue_line2* d_lines, size_t lines_cap, size_t* n_out,
                               size_t* n_groups, void* stream) {
  if (int rc = lines2_k(k, n_out, n_groups)) return rc;
  return search2_device(ctx, kVariantChess, false, d_text, d_fen_off, d_moves_off, ngames, d_out, cap, d_off, off_cap,
                        nullptr, nullptr, 0, n_out, n_groups, nullptr, stream, k, d_lines, lines_cap);
}

int fnnue_search2_lines(fnnue_ctx* ctx, const char* text, size_t text_len, const uint32_t* fen_off,
                        const uint32_t* moves_off, size_t ngames, uint32_t k, fnnue_best2* out, size_t cap,
                        uint32_t* off, size_t off_cap, fnnue_line2* lines, size_t lines_cap, size_t* n_out,
                        size_t* n_groups) {
  if (int rc = lines2_k(k, n_out, n_groups)) return rc;
  return search2_host(ctx, kVariantChess, false, text, text_len, fen_off, moves_off, ngames, out, cap, off, off_cap,
                      nullptr, nullptr, 0, n_out, n_groups, nullptr, k, lines, lines_cap);
}

int fnnue_vsearch2_lines_device(fnnue_ctx* ctx, int variant, const char* d_text, const uint32_t* d_fen_off,
                                const uint32_t* d_moves_off, size_t ngames, uint32_t k, fnnue_best2* d_out, size_t cap,
                                uint32_t* d_off, size_t off_cap, fnnue_line2* d_lines, size_t lines_cap, size_t* n_out,
                                size_t* n_groups, void* stream) {
  if (int rc = lines2_k(k, n_out, n_groups)) return rc;
  return search2_device(ctx, variant, true, d_text, d_fen_off, d_moves_off, ngames, d_out, cap, d_off, off_cap,
                        nullptr, nullptr, 0, n_out, n_groups, nullptr, stream, k, d_lines, lines_cap);
}

int fnnue_vsearch2_lines(fnnue_ctx* ctx, int variant, const char* text, size_t text_len, const uint32_t* fen_off,
                         const uint32_t* moves_off, size_t ngames, uint32_t k, fnnue_best2* out, size_t cap,
                         uint32_t* off, size_t off_cap, fnnue_line2* lines, size_t lines_cap, size_t* n_out,
                         size_t* n_groups) {
  if (int rc = lines2_k(k, n_out, n_groups)) return rc;
  return search2_host(ctx, variant, true, text, text_len, fen_off, moves_off, ngames, out, cap, off, off_cap, nullptr,
                      nullptr, 0, n_out, n_groups, nullptr, k, lines, lines_cap);
}

int fnnue_build_vchildren_device(fnnue_ctx* ctx, int variant, const char* d_text, const uint32_t* d_fen_off,
                                 const uint32_t* d_moves_off, size_t ngames, fnnue_vpos* d_out, size_t cap,
                                 uint32_t* d_off, size_t off_cap, fnnue_move* d_moves, uint8_t* d_end, size_t* n_out,
                                 size_t* n_groups, void* stream) {
  if (!ctx || !n_out || !n_groups) return fail(FNNUE_E_ARG, "null argument");
  if (d_out && (!d_moves || !d_end)) return fail(FNNUE_E_ARG, "null moves / end buffer");
  *n_out = *n_groups = 0;
  if (!variant_known(variant) || variant == kVariantChess)
    return fail(FNNUE_E_ARG, "unknown variant " + std::to_string(variant));
  return build_device(ctx, variant, d_text, d_fen_off, d_moves_off, ngames, true, d_out, cap, d_off, off_cap, d_moves,
                      d_end, n_out, n_groups, stream);
}

int fnnue_build_vchildren(fnnue_ctx* ctx, int variant, const char* text, size_t text_len, const uint32_t* fen_off,
                          const uint32_t* moves_off, size_t ngames, fnnue_vpos* out, size_t cap, uint32_t* off,
                          size_t off_cap, fnnue_move* moves, uint8_t* end, size_t* n_out, size_t* n_groups) {
  if (!ctx || !n_out || !n_groups || (ngames && (!text || !fen_off || !moves_off)))
    return fail(FNNUE_E_ARG, "null argument");
  *n_out = *n_groups = 0;
  if (!variant_known(variant) || variant == kVariantChess) return fail(FNNUE_E_ARG, "unknown variant " + std::to_string(variant));
  if (ngames == 0) return FNNUE_OK;
  return build_children_host(ctx, text, text_len, fen_off, moves_off, ngames, out, cap, off, off_cap, moves, end, n_out,
                             n_groups, [&](const StagedGames& d, hipStream_t s, auto... outputs) {
                               return fnnue_build_vchildren_device(ctx, variant, d.text, d.fen_off, d.moves_off, ngames,
                                                                   outputs..., n_out, n_groups, s);
                             });
}

int fnnue_vsearch1_device(fnnue_ctx* ctx, int variant, const char* d_text, const uint32_t* d_fen_off,
                          const uint32_t* d_moves_off, size_t ngames, fnnue_best* d_out, size_t cap, uint32_t* d_off,
                          size_t off_cap, size_t* n_out, size_t* n_groups, void* stream) {
  return search1_device(ctx, variant, d_text, d_fen_off, d_moves_off, ngames, 0, d_out, cap, d_off, off_cap, nullptr,
                        0, n_out, n_groups, stream);
}

int fnnue_vsearch1_lines_device(fnnue_ctx* ctx, int variant, const char* d_text, const uint32_t* d_fen_off,
                                const uint32_t* d_moves_off, size_t ngames, uint32_t k, fnnue_best* d_out, size_t cap,
                                uint32_t* d_off, size_t off_cap, fnnue_line* d_lines, size_t lines_cap, size_t* n_out,
                                size_t* n_groups, void* stream) {
  if (k < 1 || k > FNNUE_MAX_CHILDREN) return fail(FNNUE_E_ARG, "k must be 1.." + std::to_string(FNNUE_MAX_CHILDREN));
  return search1_device(ctx, variant, d_text, d_fen_off, d_moves_off, ngames, k, d_out, cap, d_off, off_cap, d_lines,
                        lines_cap, n_out, n_groups, stream);
}

int fnnue_vsearch1_lines(fnnue_ctx* ctx, int variant, const char* text, size_t text_len, const uint32_t* fen_off,
                         const uint32_t* moves_off, size_t ngames, uint32_t k, fnnue_best* out, size_t cap,
                         uint32_t* off, size_t off_cap, fnnue_line* lines, size_t lines_cap, size_t* n_out,
                         size_t* n_groups) {
  if (k < 1 || k > FNNUE_MAX_CHILDREN) return fail(FNNUE_E_ARG, "k must be 1.." + std::to_string(FNNUE_MAX_CHILDREN));
  return search1_host(ctx, variant, text, text_len, fen_off, moves_off, ngames, k, out, cap, off, off_cap, lines,
                      lines_cap, n_out, n_groups);
}

int fnnue_vsearch1(fnnue_ctx* ctx, int variant, const char* text, size_t text_len, const uint32_t* fen_off,
                   const uint32_t* moves_off, size_t ngames, fnnue_best* out, size_t cap, uint32_t* off,
                   size_t off_cap, size_t* n_out, size_t* n_groups) {
  return search1_host(ctx, variant, text, text_len, fen_off, moves_off, ngames, 0, out, cap, off, off_cap, nullptr, 0,
                      n_out, n_groups);
}

int fnnue_build_batch(fnnue_ctx* ctx, const char* text, size_t text_len, const uint32_t* fen_off,
                      const uint32_t* moves_off, size_t ngames, int mode, fnnue_pos* out, size_t cap, uint32_t* off,
                      size_t off_cap, size_t* n_out, size_t* n_groups) {
  if (!ctx || !n_out || !n_groups || (ngames && (!text || !fen_off || !moves_off)))
    return fail(FNNUE_E_ARG, "null argument");
  *n_out = *n_groups = 0;
  if (ngames == 0) return FNNUE_OK;
  DeviceGuard g(ctx->device);
  // Input and output staging are per-context and grow-only (host-API calls are
  // synchronous), so a steady stream of batches allocates nothing.
  StagedGames d;
  int rc = stage_games(ctx, text, text_len, fen_off, moves_off, ngames, &d);
  if (rc) return rc;
  hipStream_t s = ctx->stream;
  rc = fnnue_build_batch_device(ctx, d.text, d.fen_off, d.moves_off, ngames, mode, nullptr, 0, nullptr, 0, n_out, n_groups, s);
  if (rc != FNNUE_E_CAPACITY) return rc;  // sizing pass: always "too small" with no outputs
  if (!out || !off || cap < *n_out || off_cap < *n_groups + 1) return fail(FNNUE_E_CAPACITY, "output buffer too small");
  if ((rc = ensure_stage(ctx, *n_out, *n_groups + 1))) return rc;
  fnnue_pos* d_out = ctx->d_pos;
  uint32_t* d_off = ctx->d_off;
  rc = fnnue_build_batch_device(ctx, d.text, d.fen_off, d.moves_off, ngames, mode, d_out, *n_out, d_off, *n_groups + 1, n_out,
                                n_groups, s);
  if (rc) return rc;
  HIP_TRY(hipMemcpyAsync(out, d_out, *n_out * sizeof(fnnue_pos), hipMemcpyDeviceToHost, s), "D2H");
  HIP_TRY(hipMemcpyAsync(off, d_off, (*n_groups + 1) * 4, hipMemcpyDeviceToHost, s), "D2H");
  HIP_TRY(hipStreamSynchronize(s), "hipStreamSynchronize");
  return FNNUE_OK;
}

}  // extern "C"

// ---- capture quiescence (ABI 3.13; the kernels: quiesce.hip) ----
extern "C" {

int fnnue_set_search_quiesce(fnnue_ctx* ctx, int depth) {
  if (!ctx) return fail(FNNUE_E_ARG, "null ctx");
  if (depth < 0 || depth > FNNUE_QUIESCE_MAX)
    return fail(FNNUE_E_ARG, "quiescence depth must be 0.." + std::to_string(FNNUE_QUIESCE_MAX));
  ctx->search_quiesce = depth;
  return FNNUE_OK;
}

int fnnue_get_search_quiesce(const fnnue_ctx* ctx, int* depth) {
  if (!ctx || !depth) return fail(FNNUE_E_ARG, "null argument");
  *depth = ctx->search_quiesce;
  return FNNUE_OK;
}

int fnnue_set_search_quiesce_checks(fnnue_ctx* ctx, int on) {
  if (!ctx) return fail(FNNUE_E_ARG, "null ctx");
  ctx->search_quiesce_checks = on != 0;
  return FNNUE_OK;
}

int fnnue_get_search_quiesce_checks(const fnnue_ctx* ctx, int* on) {
  if (!ctx || !on) return fail(FNNUE_E_ARG, "null argument");
  *on = ctx->search_quiesce_checks ? 1 : 0;
  return FNNUE_OK;
}

int fnnue_quiesce_slices(const fnnue_ctx* ctx, uint64_t* slices) {
  if (!ctx || !slices) return fail(FNNUE_E_ARG, "null argument");
  *slices = ctx->quiesce_slices;
  return FNNUE_OK;
}

int fnnue_quiesce_device(fnnue_ctx* ctx, const char* d_text, const uint32_t* d_fen_off, const uint32_t* d_moves_off,
                         size_t ngames, uint32_t depth, fnnue_quiet* d_out, size_t cap, uint32_t* d_off,
                         size_t off_cap, size_t* n_out, size_t* n_groups, void* stream) {
  if (!ctx || !n_out || !n_groups) return fail(FNNUE_E_ARG, "null argument");
  *n_out = *n_groups = 0;
  if (depth > FNNUE_QUIESCE_MAX)
    return fail(FNNUE_E_ARG, "quiescence depth must be 0.." + std::to_string(FNNUE_QUIESCE_MAX));
  if (ctx->variant != kVariantChess) return fail(FNNUE_E_ARCH, "quiescence needs a chess net");
  const size_t room = d_out && d_off && off_cap >= ngames + 1 ? cap : 0;
  return replayed_plies(ctx, kVariantChess, d_text, d_fen_off, d_moves_off, ngames, room, d_off, n_out, n_groups, stream,
                        [&](const void* states, size_t n, const uint32_t*, hipStream_t s) {
                          if (n > 0xFFFFFFFFu) return fail(FNNUE_E_ARG, "batch too large");
                          return quiesce_nodes_device(ctx, ctx->bscratch, SearchRules{}, states, (uint32_t)n,
                                                      (int)depth, ctx->search_quiesce_checks, d_out, s, nullptr);
                        });
}

int fnnue_quiesce(fnnue_ctx* ctx, const char* text, size_t text_len, const uint32_t* fen_off,
                  const uint32_t* moves_off, size_t ngames, uint32_t depth, fnnue_quiet* out, size_t cap,
                  uint32_t* off, size_t off_cap, size_t* n_out, size_t* n_groups) {
  if (!ctx || !n_out || !n_groups || (ngames && (!text || !fen_off || !moves_off)))
    return fail(FNNUE_E_ARG, "null argument");
  *n_out = *n_groups = 0;
  if (depth > FNNUE_QUIESCE_MAX)
    return fail(FNNUE_E_ARG, "quiescence depth must be 0.." + std::to_string(FNNUE_QUIESCE_MAX));
  if (ctx->variant != kVariantChess) return fail(FNNUE_E_ARCH, "quiescence needs a chess net");
  if (ngames == 0) return FNNUE_OK;
  return plies_host(ctx, text, text_len, fen_off, moves_off, ngames, out, cap, off, off_cap, n_out, true,
                    [&](const StagedGames& d, hipStream_t s, auto... outputs) {
                      return fnnue_quiesce_device(ctx, d.text, d.fen_off, d.moves_off, ngames, depth, outputs...,
                                                  n_out, n_groups, s);
                    });
}

// ---- the variants' capture quiescence (ABI 3.15) ----
int fnnue_set_search_vquiesce(fnnue_ctx* ctx, int depth, int checks) {
  if (!ctx) return fail(FNNUE_E_ARG, "null ctx");
  if (depth < 0 || depth > FNNUE_QUIESCE_MAX)
    return fail(FNNUE_E_ARG, "quiescence depth must be 0.." + std::to_string(FNNUE_QUIESCE_MAX));
  ctx->search_vquiesce = depth;
  ctx->search_vquiesce_checks = checks != 0;
  return FNNUE_OK;
}

int fnnue_get_search_vquiesce(const fnnue_ctx* ctx, int* depth, int* checks) {
  if (!ctx || !depth || !checks) return fail(FNNUE_E_ARG, "null argument");
  *depth = ctx->search_vquiesce;
  *checks = ctx->search_vquiesce_checks ? 1 : 0;
  return FNNUE_OK;
}

int fnnue_vquiesce_device(fnnue_ctx* ctx, int variant, const char* d_text, const uint32_t* d_fen_off,
                          const uint32_t* d_moves_off, size_t ngames, uint32_t depth, int checks, fnnue_quiet* d_out,
                          size_t cap, uint32_t* d_off, size_t off_cap, size_t* n_out, size_t* n_groups, void* stream) {
  if (!ctx || !n_out || !n_groups) return fail(FNNUE_E_ARG, "null argument");
  *n_out = *n_groups = 0;
  if (depth > FNNUE_QUIESCE_MAX)
    return fail(FNNUE_E_ARG, "quiescence depth must be 0.." + std::to_string(FNNUE_QUIESCE_MAX));
  if (variant == kVariantChess) return fail(FNNUE_E_ARCH, "the variants' quiescence needs a variant");
  if (int rc = search1_arch(ctx, variant)) return rc;
  const size_t room = d_out && d_off && off_cap >= ngames + 1 ? cap : 0;
  return replayed_plies(ctx, variant, d_text, d_fen_off, d_moves_off, ngames, room, d_off, n_out, n_groups, stream,
                        [&](const void* states, size_t n, const uint32_t*, hipStream_t s) {
                          if (n > 0xFFFFFFFFu) return fail(FNNUE_E_ARG, "batch too large");
                          return quiesce_nodes_device(ctx, ctx->bscratch, SearchRules{variant}, states, (uint32_t)n,
                                                      (int)depth, checks != 0, d_out, s, nullptr);
                        });
}

int fnnue_vquiesce(fnnue_ctx* ctx, int variant, const char* text, size_t text_len, const uint32_t* fen_off,
                   const uint32_t* moves_off, size_t ngames, uint32_t depth, int checks, fnnue_quiet* out, size_t cap,
                   uint32_t* off, size_t off_cap, size_t* n_out, size_t* n_groups) {
  if (!ctx || !n_out || !n_groups || (ngames && (!text || !fen_off || !moves_off)))
    return fail(FNNUE_E_ARG, "null argument");
  *n_out = *n_groups = 0;
  if (depth > FNNUE_QUIESCE_MAX)
    return fail(FNNUE_E_ARG, "quiescence depth must be 0.." + std::to_string(FNNUE_QUIESCE_MAX));
  if (variant == kVariantChess) return fail(FNNUE_E_ARCH, "the variants' quiescence needs a variant");
  if (int rc = search1_arch(ctx, variant)) return rc;
  if (ngames == 0) return FNNUE_OK;
  return plies_host(ctx, text, text_len, fen_off, moves_off, ngames, out, cap, off, off_cap, n_out, true,
                    [&](const StagedGames& d, hipStream_t s, auto... outputs) {
                      return fnnue_vquiesce_device(ctx, variant, d.text, d.fen_off, d.moves_off, ngames, depth, checks,
                                                   outputs..., n_out, n_groups, s);
                    });
}

}  // extern "C"

// ---- repetition and fifty-move draws (ABI 3.12; the kernels: draws.hip) ----
extern "C" {

int fnnue_set_search_draws(fnnue_ctx* ctx, int on) {
  if (!ctx) return fail(FNNUE_E_ARG, "null ctx");
  ctx->search_draws = on != 0;
  return FNNUE_OK;
}

int fnnue_get_search_draws(const fnnue_ctx* ctx, int* on) {
  if (!ctx || !on) return fail(FNNUE_E_ARG, "null argument");
  *on = ctx->search_draws ? 1 : 0;
  return FNNUE_OK;
}

int fnnue_set_search_vdraws(fnnue_ctx* ctx, int on) {
  if (!ctx) return fail(FNNUE_E_ARG, "null ctx");
  ctx->search_vdraws = on != 0;
  return FNNUE_OK;
}

int fnnue_get_search_vdraws(const fnnue_ctx* ctx, int* on) {
  if (!ctx || !on) return fail(FNNUE_E_ARG, "null argument");
  *on = ctx->search_vdraws ? 1 : 0;
  return FNNUE_OK;
}

}  // extern "C"

namespace {

// fnnue_game_history_device / fnnue_game_vhistory_device: the replay of `variant`, then its history.
int history_device(fnnue_ctx* ctx, int variant, const char* d_text, const uint32_t* d_fen_off,
                   const uint32_t* d_moves_off, size_t ngames, fnnue_ply_history* d_out, size_t cap, uint32_t* d_off,
                   size_t off_cap, size_t* n_out, size_t* n_groups, void* stream) {
  const size_t room = d_out && d_off && off_cap >= ngames + 1 ? cap : 0;
  return replayed_plies(ctx, variant, d_text, d_fen_off, d_moves_off, ngames, room, d_off, n_out, n_groups, stream,
                        [&](const void* states, size_t n, const uint32_t* ply_off, hipStream_t s) {
                          DrawHistory hist;
                          HIP_TRY(game_history_device(SearchRules{variant}, d_text, d_fen_off, d_moves_off, ply_off,
                                                      (uint32_t)ngames, states, (uint32_t)n, draw_key_bits(), s,
                                                      ctx->bscratch, &hist),
                                  "game history launch");
                          HIP_TRY(hipMemcpyAsync(d_out, hist.hist, n * sizeof(fnnue_ply_history),
                                                 hipMemcpyDeviceToDevice, s),
                                  "D2D(history)");
                          return (int)FNNUE_OK;
                        });
}

}  // namespace

extern "C" {

int fnnue_game_history_device(fnnue_ctx* ctx, const char* d_text, const uint32_t* d_fen_off,
                              const uint32_t* d_moves_off, size_t ngames, fnnue_ply_history* d_out, size_t cap,
                              uint32_t* d_off, size_t off_cap, size_t* n_out, size_t* n_groups, void* stream) {
  if (!ctx || !n_out || !n_groups) return fail(FNNUE_E_ARG, "null argument");
  *n_out = *n_groups = 0;
  return history_device(ctx, kVariantChess, d_text, d_fen_off, d_moves_off, ngames, d_out, cap, d_off, off_cap, n_out,
                        n_groups, stream);
}

int fnnue_game_vhistory_device(fnnue_ctx* ctx, int variant, const char* d_text, const uint32_t* d_fen_off,
                               const uint32_t* d_moves_off, size_t ngames, fnnue_ply_history* d_out, size_t cap,
                               uint32_t* d_off, size_t off_cap, size_t* n_out, size_t* n_groups, void* stream) {
  if (!ctx || !n_out || !n_groups) return fail(FNNUE_E_ARG, "null argument");
  *n_out = *n_groups = 0;
  if (!variant_known(variant) || variant == kVariantChess)
    return fail(FNNUE_E_ARG, "unknown variant " + std::to_string(variant));
  return history_device(ctx, variant, d_text, d_fen_off, d_moves_off, ngames, d_out, cap, d_off, off_cap, n_out,
                        n_groups, stream);
}

int fnnue_ctx_game_vhistory(fnnue_ctx* ctx, int variant, const char* text, size_t text_len, const uint32_t* fen_off,
                            const uint32_t* moves_off, size_t ngames, fnnue_ply_history* out, size_t cap,
                            uint32_t* off, size_t off_cap, size_t* n_out, size_t* n_groups) {
  if (!ctx || !n_out || !n_groups || (ngames && (!text || !fen_off || !moves_off)))
    return fail(FNNUE_E_ARG, "null argument");
  *n_out = *n_groups = 0;
  if (!variant_known(variant) || variant == kVariantChess)
    return fail(FNNUE_E_ARG, "unknown variant " + std::to_string(variant));
  if (ngames == 0) return FNNUE_OK;
  return plies_host(ctx, text, text_len, fen_off, moves_off, ngames, out, cap, off, off_cap, n_out, false,
                    [&](const StagedGames& d, hipStream_t s, auto... outputs) {
                      return fnnue_game_vhistory_device(ctx, variant, d.text, d.fen_off, d.moves_off, ngames,
                                                        outputs..., n_out, n_groups, s);
                    });
}

int fnnue_ctx_game_history(fnnue_ctx* ctx, const char* text, size_t text_len, const uint32_t* fen_off,
                           const uint32_t* moves_off, size_t ngames, fnnue_ply_history* out, size_t cap, uint32_t* off,
                           size_t off_cap, size_t* n_out, size_t* n_groups) {
  if (!ctx || !n_out || !n_groups || (ngames && (!text || !fen_off || !moves_off)))
    return fail(FNNUE_E_ARG, "null argument");
  *n_out = *n_groups = 0;
  if (ngames == 0) return FNNUE_OK;
  return plies_host(ctx, text, text_len, fen_off, moves_off, ngames, out, cap, off, off_cap, n_out, false,
                    [&](const StagedGames& d, hipStream_t s, auto... outputs) {
                      return fnnue_game_history_device(ctx, d.text, d.fen_off, d.moves_off, ngames, outputs..., n_out,
                                                       n_groups, s);
                    });
}

}  // extern "C"
