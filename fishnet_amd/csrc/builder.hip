// builder.hip — device-side batch builder: FEN parse, UCI-move replay
// (standard + Chess960 castling, en passant, promotion) and legal 1-ply
// children, producing packed fnnue_pos records in HBM.
//
// Replaces on the device what board.cpp does on the host, i.e. the role
// shakmaty 0.23.0 plays in the reference's batch expansion
// ([ref] src/queue.rs:518-627: VariantPosition::from_setup, Uci::to_move,
// play_unchecked; wire format src/api.rs:293-309).  Semantics are those of the
// host builder (board.cpp), which is perft-checked; tests compare the two
// record for record, and fnnue_perft_device pins the move generator on the
// published perft counts.
//
// Replay is one 64-lane wave per game (replay_wave.h, rules in chess_rules.h: the board chain plays a
// window of moves wave-uniformly, lanes then check the moves and pack the
// boards in parallel); children are one thread per ply.  Boards are bitboards
// in registers: no tables, attacks from shifts and ray walks.
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>

#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "board.h"
#include "builder.h"
#include "net.h"
#include "chess_rules.h"
#include "replay_wave.h"

namespace fnnue {

namespace {

// The board rules and ChessRules (the wave replay's chess rule set): chess_rules.h.

// ---- kernels ----
// text layout of game g: FEN in [fen_off[g], mv_off[g]), moves in [mv_off[g], fen_off[g + 1]).
__global__ void count_plies_kernel(const char* __restrict__ text, const uint32_t* __restrict__ fen_off,
                                   const uint32_t* __restrict__ mv_off, uint32_t ngames, uint32_t* __restrict__ plies) {
  const uint32_t g = blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= ngames) return;
  plies[g] = 1u + (uint32_t)count_tokens(text, mv_off[g], fen_off[g + 1]);
}

__global__ void count_children_kernel(const DBoard* __restrict__ states, uint32_t n, uint32_t* __restrict__ cnt) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const DBoard b = states[i];
  uint32_t c = 0;
  for_each_legal(b, [&](const DMove&) -> bool {
    ++c;
    return true;
  });
  cnt[i] = 1u + c;
}

__global__ void write_children_kernel(const DBoard* __restrict__ states, uint32_t n, const uint32_t* __restrict__ off,
                                      fnnue_pos* __restrict__ out) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const DBoard b = states[i];
  uint32_t o = off[i];
  out[o++] = pack(b);
  for_each_legal(b, [&](const DMove& m) -> bool {
    DBoard c = b;
    do_move(c, m);
    out[o++] = pack(c);
    return true;
  });
}

// ---- the one-ply search's children: records, moves, end flags ----

// fnnue_move of m on b: Board::uci(m, b.chess960) as a code (a castling move's
// destination is the king's unless the game needs Chess960 notation).
__device__ __forceinline__ uint16_t move_code(const DBoard& b, const DMove& m) {
  int to = m.to;
  if (m.castle && !b.c960) to = (m.from & 56) + (m.to > m.from ? 6 : 2);
  return (uint16_t)((uint32_t)m.from | (uint32_t)to << 6 | (uint32_t)m.promo << 12);
}

// kFinalNoMoves / kFinalCheck of b: a second ply of move generation that
// stops at the first legal move.
__device__ __forceinline__ uint8_t end_of(const DBoard& b) {
  bool any = false;
  const DBoard c = b;  // a copy for the generator's reference (ChessRules::any_legal_from)
  for_each_legal(c, [&](const DMove&) -> bool {
    any = true;
    return false;
  });
  return ChessRules::end_flags(b, any);
}

// One thread per ply: write_children_kernel plus each record's move and flags.
__global__ __launch_bounds__(64) void write_children_ply_kernel(const DBoard* __restrict__ states, uint32_t n,
                                          const uint32_t* __restrict__ off, fnnue_pos* __restrict__ out,
                                          uint16_t* __restrict__ moves, uint8_t* __restrict__ end) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const DBoard b = states[i];
  const uint32_t o0 = off[i];
  uint32_t o = o0;
  out[o] = pack(b);
  moves[o] = 0;
  ++o;
  for_each_legal(b, [&](const DMove& m) -> bool {
    DBoard c = b;
    do_move(c, m);
    out[o] = pack(c);
    moves[o] = move_code(b, m);
    end[o] = end_of(c);
    ++o;
    return true;
  });
  end[o0] = ChessRules::end_flags(b, o > o0 + 1);
}

// One thread per record: record r belongs to the ply i with off[i] <= r <
// off[i + 1]; r - off[i] = 0 is the ply itself, j > 0 its j-th legal move,
// found by generating the ply's moves up to it.
__global__ __launch_bounds__(64) void write_children_record_kernel(const DBoard* __restrict__ states, uint32_t n,
                                             const uint32_t* __restrict__ off, uint32_t total,
                                             fnnue_pos* __restrict__ out, uint16_t* __restrict__ moves,
                                             uint8_t* __restrict__ end) {
  const uint32_t r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= total) return;
  uint32_t lo = 0, hi = n;  // off[lo] <= r < off[hi]
  while (hi - lo > 1) {
    const uint32_t mid = (lo + hi) >> 1;
    if (off[mid] <= r) lo = mid;
    else hi = mid;
  }
  const uint32_t o0 = off[lo], j = r - o0;
  const DBoard b = states[lo];
  DBoard c = b;
  uint16_t mv = 0;
  if (j) {
    uint32_t k = 0;
    for_each_legal(b, [&](const DMove& m) -> bool {
      if (++k < j) return true;
      do_move(c, m);
      mv = move_code(b, m);
      return false;
    });
  }
  out[r] = pack(c);
  moves[r] = mv;
  end[r] = j ? end_of(c) : ChessRules::end_flags(b, off[lo + 1] - o0 > 1);
}

// ---- the two-ply search's child states ----
// One thread per record of the plies' STAR groups, as write_children_record_kernel
// finds its ply and its move; a child's board is stored as it is (not packed),
// the ply's own record is skipped.  Child j of ply i is entry off[i] - i + j - 1:
// a dense array in record order, which children_count_device and
// children_write_device expand like any array of boards.  map (optional):
// entry d -> (ply, 1-based child index).
__global__ __launch_bounds__(64) void child_states_kernel(const DBoard* __restrict__ states, uint32_t n,
                                                          const uint32_t* __restrict__ off, uint32_t total,
                                                          DBoard* __restrict__ out, uint2* __restrict__ map) {
  const uint32_t r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= total) return;
  uint32_t lo = 0, hi = n;  // off[lo] <= r < off[hi]
  while (hi - lo > 1) {
    const uint32_t mid = (lo + hi) >> 1;
    if (off[mid] <= r) lo = mid;
    else hi = mid;
  }
  const uint32_t j = r - off[lo];
  if (j == 0) return;
  const DBoard b = states[lo];
  DBoard c = b;
  uint32_t k = 0;
  for_each_legal(b, [&](const DMove& m) -> bool {
    if (++k < j) return true;
    do_move(c, m);
    return false;
  });
  const uint32_t d = r - lo - 1;
  out[d] = c;
  if (map) map[d] = make_uint2(lo, j);
}

// Per ply p (p = n: the totals): its first entry in the dense child array and
// that entry's first grandchild record (kid_off: the children's STAR offsets).
__global__ void ply_spans_kernel(const uint32_t* __restrict__ off, const uint32_t* __restrict__ kid_off, uint32_t n,
                                 uint32_t* __restrict__ first_child, uint32_t* __restrict__ first_rec) {
  const uint32_t p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p > n) return;
  const uint32_t c = off[p] - p;
  first_child[p] = c;
  first_rec[p] = kid_off[c];
}

// dst[i] = src[i] - src[0]: a chunk's STAR offsets cut out of the whole array's.
__global__ void rebase_offsets_kernel(const uint32_t* __restrict__ src, uint32_t n, uint32_t* __restrict__ dst) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) dst[i] = src[i] - src[0];
}

template <int D>
__device__ uint64_t perft_dev(const DBoard& b) {
  uint64_t n = 0;
  for_each_legal(b, [&](const DMove& m) -> bool {
    if constexpr (D <= 1) {
      ++n;
    } else {
      DBoard c = b;
      do_move(c, m);
      n += perft_dev<D - 1>(c);
    }
    return true;
  });
  return n;
}

template <int D>
__global__ void perft_kernel(const DBoard* __restrict__ states, uint32_t n, unsigned long long* __restrict__ total) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  atomicAdd(total, (unsigned long long)perft_dev<D>(states[i]));
}

}  // namespace

hipError_t BuilderScratch::get(int slot, size_t want, void** out) {
  if (want > bytes[slot]) {
    if (p[slot]) (void)hipFree(p[slot]);
    p[slot] = nullptr;
    bytes[slot] = 0;
    const size_t n = want + want / 4 + 256;
    const hipError_t e = hipMalloc(&p[slot], n);
    if (e != hipSuccess) return e;
    bytes[slot] = n;
  }
  *out = p[slot];
  return hipSuccess;
}

void BuilderScratch::release() {
  for (int i = 0; i < kSlots; ++i) {
    if (p[i]) (void)hipFree(p[i]);
    p[i] = nullptr;
    bytes[i] = 0;
  }
}

// Exclusive scan of cnt[0..n) into off[0..n], off[n] = total (hipcub).
hipError_t builder_exclusive_scan(const uint32_t* cnt, uint32_t* off, uint32_t n, hipStream_t s, BuilderScratch& ws) {
  size_t tmp_bytes = 0;
  hipError_t e = hipcub::DeviceScan::ExclusiveSum(nullptr, tmp_bytes, cnt, off, (int)n + 1, s);
  if (e != hipSuccess) return e;
  void* tmp = nullptr;
  if ((e = ws.get(BuilderScratch::kScan, tmp_bytes, &tmp)) != hipSuccess) return e;
  return hipcub::DeviceScan::ExclusiveSum(tmp, tmp_bytes, cnt, off, (int)n + 1, s);
}

DBoard to_dboard(const Board& h) {
  DBoard b{};
  b.bc[0] = h.byColor[0];
  b.bc[1] = h.byColor[1];
  for (int t = 0; t < 7; ++t) b.bt[t] = t ? h.byType[t] : 0;
  for (int c = 0; c < 2; ++c)
    for (int side = 0; side < 2; ++side) {
      const int sq = h.castle_rook[c][side];
      const int sh = 8 * (2 * c + side);
      b.cr = (b.cr & ~(0xFFu << sh)) | ((uint32_t)(sq < 0 ? 0xFF : sq) << sh);
    }
  b.ep = h.ep;
  b.stm = (uint32_t)h.stm;
  b.c960 = h.chess960 ? 1 : 0;
  return b;
}

namespace {

hipError_t launch_chess_replay(const char* d_text, const uint32_t* d_fen_off, const uint32_t* d_mv_off,
                               const uint32_t* d_ply_off, uint32_t ngames, fnnue_pos* d_out, DBoard* d_states,
                               uint8_t* d_final, uint32_t* d_err, hipStream_t s) {
  return replay::launch_replay<ChessRules>((int)kVariantChess, d_text, d_fen_off, d_mv_off, ngames, d_ply_off, d_out,
                                           d_states, d_err, d_final, s);
}

}  // namespace

hipError_t replay_games_device(int variant, const char* d_text, const uint32_t* d_fen_off, const uint32_t* d_mv_off,
                               const uint32_t* d_ply_off, uint32_t ngames, void* d_out, uint8_t* d_final,
                               uint32_t* d_err, hipStream_t s) {
  if (variant != kVariantChess)
    return replay_vgames_device(variant, d_text, d_fen_off, d_mv_off, d_ply_off, ngames,
                                static_cast<fnnue_vpos*>(d_out), nullptr, d_final, d_err, s);
  return launch_chess_replay(d_text, d_fen_off, d_mv_off, d_ply_off, ngames, static_cast<fnnue_pos*>(d_out), nullptr,
                             d_final, d_err, s);
}

hipError_t replay_chess_states_device(const char* d_text, const uint32_t* d_fen_off, const uint32_t* d_mv_off,
                                      const uint32_t* d_ply_off, uint32_t ngames, fnnue_pos* d_out, DBoard* d_states,
                                      uint8_t* d_final, uint32_t* d_err, hipStream_t s) {
  return launch_chess_replay(d_text, d_fen_off, d_mv_off, d_ply_off, ngames, d_out, d_states, d_final, d_err, s);
}

hipError_t children_count_device(const DBoard* d_states, uint32_t n, uint32_t* d_cnt, uint32_t* d_off, hipStream_t s,
                                 BuilderScratch& ws) {
  hipError_t e;
  if ((e = hipMemsetAsync(d_cnt + n, 0, 4, s)) != hipSuccess) return e;
  const uint32_t bs = 64;
  hipLaunchKernelGGL(count_children_kernel, dim3((n + bs - 1) / bs), dim3(bs), 0, s, d_states, n, d_cnt);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  return builder_exclusive_scan(d_cnt, d_off, n, s, ws);
}

int children_impl() {
  static const int impl = [] {
    const char* e = std::getenv("FNNUE_CHILDREN_IMPL");
    return e && std::strcmp(e, "ply") == 0 ? 0 : 1;
  }();
  return impl;
}

hipError_t children_write_device(const DBoard* d_states, uint32_t n, const uint32_t* d_off, uint32_t total,
                                 fnnue_pos* d_out, uint16_t* d_moves, uint8_t* d_end, hipStream_t s) {
  if (n == 0 || total == 0) return hipSuccess;
  const uint32_t bs = 64;
  if (children_impl() == 1)
    hipLaunchKernelGGL(write_children_record_kernel, dim3((total + bs - 1) / bs), dim3(bs), 0, s, d_states, n, d_off,
                       total, d_out, d_moves, d_end);
  else
    hipLaunchKernelGGL(write_children_ply_kernel, dim3((n + bs - 1) / bs), dim3(bs), 0, s, d_states, n, d_off, d_out,
                       d_moves, d_end);
  return hipGetLastError();
}

hipError_t child_states_device(const DBoard* d_states, uint32_t n, const uint32_t* d_off, uint32_t total,
                               DBoard* d_out, uint2* d_map, hipStream_t s) {
  if (n == 0 || total == 0) return hipSuccess;
  const uint32_t bs = 64;
  hipLaunchKernelGGL(child_states_kernel, dim3((total + bs - 1) / bs), dim3(bs), 0, s, d_states, n, d_off, total, d_out,
                     d_map);
  return hipGetLastError();
}

hipError_t ply_spans_device(const uint32_t* d_off, const uint32_t* d_kid_off, uint32_t n, uint32_t* d_first_child,
                            uint32_t* d_first_rec, hipStream_t s) {
  const uint32_t bs = 256;
  hipLaunchKernelGGL(ply_spans_kernel, dim3((n + 1 + bs - 1) / bs), dim3(bs), 0, s, d_off, d_kid_off, n, d_first_child,
                     d_first_rec);
  return hipGetLastError();
}

hipError_t rebase_offsets_device(const uint32_t* d_src, uint32_t n, uint32_t* d_dst, hipStream_t s) {
  if (n == 0) return hipSuccess;
  const uint32_t bs = 256;
  hipLaunchKernelGGL(rebase_offsets_kernel, dim3((n + bs - 1) / bs), dim3(bs), 0, s, d_src, n, d_dst);
  return hipGetLastError();
}

BuildResult build_batch_device(const char* d_text, const uint32_t* d_fen_off, const uint32_t* d_mv_off,
                               uint32_t ngames, bool children, fnnue_pos* d_out, size_t cap, uint32_t* d_group_off,
                               size_t off_cap, hipStream_t s, BuilderScratch& ws, uint8_t* d_final, uint16_t* d_moves,
                               uint8_t* d_end, ChildrenBufs* own) {
  BuildResult R;
  auto fail = [&](hipError_t e) {
    R.hip = e;
    return R;
  };
  hipError_t e;
  uint32_t *plies = nullptr, *ply_off = nullptr, *err = nullptr, *cnt = nullptr, *coff = nullptr;
  DBoard* states = nullptr;
  using W = BuilderScratch;
  if ((e = ws.get(W::kPlies, (size_t)(ngames + 1) * 4, (void**)&plies)) != hipSuccess) return fail(e);
  if ((e = ws.get(W::kPlyOff, (size_t)(ngames + 1) * 4, (void**)&ply_off)) != hipSuccess) return fail(e);
  if ((e = ws.get(W::kErr, 16, (void**)&err)) != hipSuccess) return fail(e);
  if ((e = hipMemsetAsync(err, 0, 16, s)) != hipSuccess) return fail(e);
  if ((e = hipMemsetAsync(plies + ngames, 0, 4, s)) != hipSuccess) return fail(e);
  const uint32_t bs = 64;
  hipLaunchKernelGGL(count_plies_kernel, dim3((ngames + bs - 1) / bs), dim3(bs), 0, s, d_text, d_fen_off, d_mv_off,
                     ngames, plies);
  if ((e = hipGetLastError()) != hipSuccess) return fail(e);
  if ((e = builder_exclusive_scan(plies, ply_off, ngames, s, ws)) != hipSuccess) return fail(e);
  uint32_t total_plies = 0;
  if ((e = hipMemcpyAsync(&total_plies, ply_off + ngames, 4, hipMemcpyDeviceToHost, s)) != hipSuccess) return fail(e);
  if ((e = hipStreamSynchronize(s)) != hipSuccess) return fail(e);
  if (!children) {
    R.n_out = total_plies;
    R.n_groups = ngames;
    if (cap < total_plies || off_cap < (size_t)ngames + 1 || !d_out || !d_group_off) {
      R.capacity = true;
      return R;
    }
    if ((e = launch_chess_replay(d_text, d_fen_off, d_mv_off, ply_off, ngames, d_out, nullptr, d_final, err, s)) !=
        hipSuccess)
      return fail(e);
    if ((e = hipMemcpyAsync(d_group_off, ply_off, (size_t)(ngames + 1) * 4, hipMemcpyDeviceToDevice, s)) !=
        hipSuccess)
      return fail(e);
  } else {
    if (own && total_plies > own->max_groups) {  // the search's capacity: one record per ply
      R.n_groups = total_plies;
      R.capacity = true;
      return R;
    }
    if ((e = ws.get(W::kStates, (size_t)total_plies * sizeof(DBoard), (void**)&states)) != hipSuccess) return fail(e);
    if ((e = ws.get(W::kCnt, (size_t)(total_plies + 1) * 4, (void**)&cnt)) != hipSuccess) return fail(e);
    if ((e = ws.get(W::kCoff, (size_t)(total_plies + 1) * 4, (void**)&coff)) != hipSuccess) return fail(e);
    if ((e = launch_chess_replay(d_text, d_fen_off, d_mv_off, ply_off, ngames, nullptr, states, d_final, err, s)) !=
        hipSuccess)
      return fail(e);
    uint32_t herr[4];
    if ((e = hipMemcpyAsync(herr, err, 16, hipMemcpyDeviceToHost, s)) != hipSuccess) return fail(e);
    if ((e = hipStreamSynchronize(s)) != hipSuccess) return fail(e);
    if (herr[0]) {
      R.err_code = herr[0];
      R.err_game = herr[1];
      R.err_ply = herr[2];
      return R;
    }
    if ((e = children_count_device(states, total_plies, cnt, coff, s, ws)) != hipSuccess) return fail(e);
    uint32_t total = 0;
    if ((e = hipMemcpyAsync(&total, coff + total_plies, 4, hipMemcpyDeviceToHost, s)) != hipSuccess) return fail(e);
    if ((e = hipStreamSynchronize(s)) != hipSuccess) return fail(e);
    R.n_out = total;
    R.n_groups = total_plies;
    if (own) {
      if ((e = ws.get(W::kKids, (size_t)total * sizeof(fnnue_pos), (void**)&own->pos)) != hipSuccess) return fail(e);
      if ((e = ws.get(W::kKidMoves, (size_t)total * 2, (void**)&own->moves)) != hipSuccess) return fail(e);
      if ((e = ws.get(W::kKidEnd, (size_t)total, (void**)&own->end)) != hipSuccess) return fail(e);
      own->off = coff;
      own->ply_off = ply_off;
      if ((e = children_write_device(states, total_plies, coff, total, own->pos, own->moves, own->end, s)) !=
          hipSuccess)
        return fail(e);
    } else {
      if (cap < total || off_cap < (size_t)total_plies + 1 || !d_out || !d_group_off) {
        R.capacity = true;
        return R;
      }
      if (d_moves && d_end) {
        if ((e = children_write_device(states, total_plies, coff, total, d_out, d_moves, d_end, s)) != hipSuccess)
          return fail(e);
      } else {
        hipLaunchKernelGGL(write_children_kernel, dim3((total_plies + bs - 1) / bs), dim3(bs), 0, s, states,
                           total_plies, coff, d_out);
        if ((e = hipGetLastError()) != hipSuccess) return fail(e);
      }
      if ((e = hipMemcpyAsync(d_group_off, coff, (size_t)(total_plies + 1) * 4, hipMemcpyDeviceToDevice, s)) !=
          hipSuccess)
        return fail(e);
    }
  }
  uint32_t herr[4];
  if ((e = hipMemcpyAsync(herr, err, 16, hipMemcpyDeviceToHost, s)) != hipSuccess) return fail(e);
  if ((e = hipStreamSynchronize(s)) != hipSuccess) return fail(e);
  R.err_code = herr[0];
  R.err_game = herr[1];
  R.err_ply = herr[2];
  return R;
}

BuildResult replay_states_device(int variant, const char* d_text, const uint32_t* d_fen_off, const uint32_t* d_mv_off,
                                 uint32_t ngames, size_t max_plies, hipStream_t s, BuilderScratch& ws,
                                 const void** d_states, const uint32_t** d_ply_off) {
  BuildResult R;
  auto fail = [&](hipError_t e) {
    R.hip = e;
    return R;
  };
  hipError_t e;
  uint32_t *plies = nullptr, *ply_off = nullptr, *err = nullptr;
  void* states = nullptr;
  const size_t state_bytes = variant == kVariantChess ? sizeof(DBoard) : vstate_bytes(variant);
  using W = BuilderScratch;
  if ((e = ws.get(W::kPlies, (size_t)(ngames + 1) * 4, (void**)&plies)) != hipSuccess) return fail(e);
  if ((e = ws.get(W::kPlyOff, (size_t)(ngames + 1) * 4, (void**)&ply_off)) != hipSuccess) return fail(e);
  if ((e = ws.get(W::kErr, 16, (void**)&err)) != hipSuccess) return fail(e);
  if ((e = hipMemsetAsync(err, 0, 16, s)) != hipSuccess) return fail(e);
  if ((e = hipMemsetAsync(plies + ngames, 0, 4, s)) != hipSuccess) return fail(e);
  const uint32_t bs = 64;
  hipLaunchKernelGGL(count_plies_kernel, dim3((ngames + bs - 1) / bs), dim3(bs), 0, s, d_text, d_fen_off, d_mv_off,
                     ngames, plies);
  if ((e = hipGetLastError()) != hipSuccess) return fail(e);
  if ((e = builder_exclusive_scan(plies, ply_off, ngames, s, ws)) != hipSuccess) return fail(e);
  uint32_t total_plies = 0;
  if ((e = hipMemcpyAsync(&total_plies, ply_off + ngames, 4, hipMemcpyDeviceToHost, s)) != hipSuccess) return fail(e);
  if ((e = hipStreamSynchronize(s)) != hipSuccess) return fail(e);
  R.n_out = total_plies;
  R.n_groups = ngames;
  if (total_plies > max_plies) {
    R.capacity = true;
    return R;
  }
  if ((e = ws.get(W::kStates, (size_t)total_plies * state_bytes, &states)) != hipSuccess) return fail(e);
  e = variant == kVariantChess
          ? launch_chess_replay(d_text, d_fen_off, d_mv_off, ply_off, ngames, nullptr, static_cast<DBoard*>(states),
                                nullptr, err, s)
          : replay_vgames_device(variant, d_text, d_fen_off, d_mv_off, ply_off, ngames, nullptr, states, nullptr, err, s);
  if (e != hipSuccess) return fail(e);
  uint32_t herr[4];
  if ((e = hipMemcpyAsync(herr, err, 16, hipMemcpyDeviceToHost, s)) != hipSuccess) return fail(e);
  if ((e = hipStreamSynchronize(s)) != hipSuccess) return fail(e);
  R.err_code = herr[0];
  R.err_game = herr[1];
  R.err_ply = herr[2];
  *d_states = states;
  *d_ply_off = ply_off;
  return R;
}

hipError_t perft_device(const std::vector<DBoard>& frontier, int depth, uint64_t* nodes) {
  *nodes = 0;
  if (frontier.empty()) return hipSuccess;
  if (depth < 1 || depth > 3) return hipErrorInvalidValue;
  DBoard* d = nullptr;
  unsigned long long* tot = nullptr;
  hipError_t e = hipMalloc(&d, frontier.size() * sizeof(DBoard));
  if (e != hipSuccess) return e;
  if ((e = hipMalloc(&tot, 8)) == hipSuccess && (e = hipMemset(tot, 0, 8)) == hipSuccess &&
      (e = hipMemcpy(d, frontier.data(), frontier.size() * sizeof(DBoard), hipMemcpyHostToDevice)) == hipSuccess) {
    const uint32_t n = (uint32_t)frontier.size(), bs = 64;
    if (depth == 1) hipLaunchKernelGGL(perft_kernel<1>, dim3((n + bs - 1) / bs), dim3(bs), 0, 0, d, n, tot);
    else if (depth == 2) hipLaunchKernelGGL(perft_kernel<2>, dim3((n + bs - 1) / bs), dim3(bs), 0, 0, d, n, tot);
    else hipLaunchKernelGGL(perft_kernel<3>, dim3((n + bs - 1) / bs), dim3(bs), 0, 0, d, n, tot);
    if ((e = hipGetLastError()) == hipSuccess) {
      unsigned long long h = 0;
      e = hipMemcpy(&h, tot, 8, hipMemcpyDeviceToHost);
      *nodes = h;
    }
  }
  (void)hipFree(d);
  if (tot) (void)hipFree(tot);
  return e;
}

}  // namespace fnnue
