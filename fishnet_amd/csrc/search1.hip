// search1.hip — the reduction of the one-ply search: the best child of every
// STAR group (fnnue_best_children_device, include/fnnue.h), i.e. the chess rule
// of the backend's move work (backend.cpp fill_roots) on the device.
//
// A group averages about 35 children and has at most 219 records, so a wave
// per group would idle half its lanes: 32 lanes (half a wave) share a group.
// Each lane folds the children lane, lane + 32, ... into one 64-bit key
//   rank (2 mate in one, 1 everything else) << 62 | (value + 2^29) << 32 | ~index
// (|value| <= 2^28: the sum of two int32 over 16), so that the largest key is
// the first maximum whatever lane saw it; five xor-shuffles inside the half
// wave leave it in every lane, and lanes 0-5 store one dword each of the
// 24-byte record.  No atomics, no LDS, no host synchronisation.
#include <hip/hip_runtime.h>

#include "builder.h"

namespace fnnue {

namespace {

constexpr uint32_t kGroupLanes = 32, kBlock = 256;
static_assert(sizeof(fnnue_best) == 24, "fnnue_best is six dwords");

__global__ __launch_bounds__(kBlock) void best_children_kernel(
    const int32_t* __restrict__ psqt, const int32_t* __restrict__ positional, const uint8_t* __restrict__ end,
    const uint16_t* __restrict__ moves, const uint32_t* __restrict__ off, uint32_t ngroups, uint32_t npos,
    uint32_t* __restrict__ out) {
  const uint64_t t = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
  const uint32_t g = (uint32_t)(t / kGroupLanes), lane = (uint32_t)(t % kGroupLanes);
  const bool live = g < ngroups;  // no early return: the shuffles below run with the whole wave
  uint32_t o = 0, e = 0;
  if (live) {
    e = min(off[g + 1], npos);
    o = min(off[g], e);
  }
  const uint32_t nrec = e - o;
  unsigned long long key = 0;  // 0: no child (every child's rank is >= 1)
  for (uint32_t c = 1 + lane; c < nrec; c += kGroupLanes) {
    const uint32_t x = o + c;
    const uint32_t f = end[x];
    uint32_t rank = 1;
    int32_t v = 0;
    if (f & kFinalNoMoves) {
      rank = (f & kFinalCheck) ? 2u : 1u;  // mate in one / stalemate (worth 0)
    } else {
      v = (int32_t)-(((long long)psqt[x] + (long long)positional[x]) / 16);
    }
    const unsigned long long k = (unsigned long long)rank << 62 |
                                 (unsigned long long)(uint32_t)(v + (1 << 29)) << 32 | (0xFFFFFFFFu - c);
    key = k > key ? k : key;
  }
#pragma unroll
  for (int m = kGroupLanes / 2; m >= 1; m >>= 1) {
    const unsigned long long other = (unsigned long long)__shfl_xor((long long)key, m, kGroupLanes);
    key = other > key ? other : key;
  }
  const uint32_t best = key ? 0xFFFFFFFFu - (uint32_t)key : 0u;
  const uint32_t rank = (uint32_t)(key >> 62);
  const int32_t value = (int32_t)((uint32_t)(key >> 32) & 0x3FFFFFFFu) - (1 << 29);
  uint32_t w = 0;
  if (nrec) {  // an empty group: all zero
    const uint32_t kind = !best ? FNNUE_BEST_NONE : rank == 2 ? FNNUE_BEST_MATE : FNNUE_BEST_CP;
    switch (lane) {
      case 0: w = best ? 0u - (uint32_t)psqt[o + best] : 0u; break;        // negated, wrapping
      case 1: w = best ? 0u - (uint32_t)positional[o + best] : 0u; break;
      case 2: w = kind == FNNUE_BEST_CP ? (uint32_t)value : 0u; break;
      case 3: w = nrec - 1; break;
      case 4: w = best; break;
      case 5: w = (best && moves ? (uint32_t)moves[o + best] : 0u) | kind << 16 | (uint32_t)end[o] << 24; break;
      default: break;
    }
  }
  if (live && lane < 6) out[(size_t)g * 6 + lane] = w;
}

__global__ __launch_bounds__(kBlock) void gather_parents_kernel(const int32_t* __restrict__ psqt,
                                                                const int32_t* __restrict__ positional,
                                                                const uint32_t* __restrict__ off, uint32_t ngroups,
                                                                uint32_t npos, int32_t* __restrict__ ps_out,
                                                                int32_t* __restrict__ po_out) {
  const uint32_t g = blockIdx.x * kBlock + threadIdx.x;
  if (g >= ngroups) return;
  const uint32_t o = off[g];
  const bool ok = o < npos && o < off[g + 1];
  ps_out[g] = ok ? psqt[o] : 0;
  po_out[g] = ok ? positional[o] : 0;
}

}  // namespace

hipError_t launch_best_children(const int32_t* d_psqt, const int32_t* d_positional, const uint8_t* d_end,
                                const uint16_t* d_moves, const uint32_t* d_off, uint32_t ngroups, uint32_t npos,
                                fnnue_best* d_out, hipStream_t s) {
  if (ngroups == 0) return hipSuccess;
  const uint64_t threads = (uint64_t)ngroups * kGroupLanes;
  hipLaunchKernelGGL(best_children_kernel, dim3((uint32_t)((threads + kBlock - 1) / kBlock)), dim3(kBlock), 0, s,
                     d_psqt, d_positional, d_end, d_moves, d_off, ngroups, npos, reinterpret_cast<uint32_t*>(d_out));
  return hipGetLastError();
}

hipError_t launch_gather_parents(const int32_t* d_psqt, const int32_t* d_positional, const uint32_t* d_off,
                                 uint32_t ngroups, uint32_t npos, int32_t* d_ps_out, int32_t* d_po_out,
                                 hipStream_t s) {
  if (ngroups == 0) return hipSuccess;
  hipLaunchKernelGGL(gather_parents_kernel, dim3((ngroups + kBlock - 1) / kBlock), dim3(kBlock), 0, s, d_psqt,
                     d_positional, d_off, ngroups, npos, d_ps_out, d_po_out);
  return hipGetLastError();
}

}  // namespace fnnue
