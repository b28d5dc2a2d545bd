// psqt_tile.h — layout of the PSQT tile that the slice-0 workgroups of
// ft_slices keep in LDS (DESIGN §4.2 "PSQT tile").  Plain integer arithmetic
// shared by the fill and the gathers (ft_sliced.hip) and the host test
// (tests/psqt_tile_host.cpp): no HIP types, compiles with any C++14 compiler.
//
// The net holds psqt_w row-major, [row][8 buckets].  Copied like that into
// LDS, word 8 row + bucket lies on bank 8 (row mod 4) + bucket of the 32 that
// ds_read_b32 counts per 32-lane half.  The items of a pass are sorted by piece
// count and so share one bucket nearly always: all gathers of a wave then fall
// on 4 of the 32 banks.  The tile is therefore kept bucket-major,
// [bucket][stride] with stride = the tile's rows rounded up to a multiple of 4:
// 708 (chess, atomic) and 868 (crazyhouse) are both 4 (mod 32), so word
// bucket * stride + row lies on bank (4 bucket + row) mod 32 and the rows of
// one bucket spread over all 32 banks.
#pragma once
#include <stdint.h>

#ifndef FNNUE_HD
#ifdef __HIPCC__
#define FNNUE_HD __host__ __device__
#else
#define FNNUE_HD
#endif
#endif

namespace fnnue {

constexpr int kPsqtTileBuckets = 8;  // = kPsqtBuckets (net.h)

// tile_rows = the feature rows of a king block + the zero row (G::kTileRows).
// Rows from the block's row count up to the stride are zero in every bucket.
FNNUE_HD constexpr int psqt_tile_stride(int tile_rows) { return (tile_rows + 3) & ~3; }
FNNUE_HD constexpr int psqt_tile_words(int tile_rows) { return kPsqtTileBuckets * psqt_tile_stride(tile_rows); }
// The word of (row, bucket): the one index map of the fill and of every gather.
FNNUE_HD constexpr int psqt_tile_word(int row, int bucket, int stride) { return bucket * stride + row; }

// The fill transposes on the way into LDS.  16-byte chunk i of the king block's
// psqt_w rows holds buckets 4 (i & 1) .. + 3 of row i >> 1; the thread that
// loaded it stores its word k to (psqt_fill_row(i), psqt_fill_bucket(i, k)).
// A half-wave's 32 chunks (16 rows x 2) then store word k to 32 different
// banks, (16 (i & 1) + 4 k + row) mod 32.  Chunks from 2 * rows up to
// psqt_fill_chunks() store zeros (the zero row and the rows up to the stride).
FNNUE_HD constexpr int psqt_fill_row(int i) { return i >> 1; }
FNNUE_HD constexpr int psqt_fill_bucket(int i, int k) { return 4 * (i & 1) + k; }
FNNUE_HD constexpr int psqt_fill_chunks(int tile_rows) { return 2 * psqt_tile_stride(tile_rows); }

}  // namespace fnnue
