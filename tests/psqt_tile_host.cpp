// Host driver of fishnet_amd/csrc/psqt_tile.h for tests/test_psqt_tile.py.
// For each geometry given on the command line (feature rows of a king block:
// 704 chess / atomic, 864 crazyhouse) it replays the fill of ft_slices on a
// psqt_w block whose word (row, bucket) holds 8 row + bucket + 1, and checks
//   - every store lands inside the declared array, every word of it is
//     stored exactly once (the map is injective and onto);
//   - a gather through psqt_tile_word finds (row, bucket)'s value, and zero
//     in every bucket for the rows from `rows` up to the stride;
//   - word k of a half-wave's 32 chunks goes to 32 different banks.
// Prints "error ..." lines for violations, then
//   geom <rows> stride <stride> words <words> chunks <chunks> bank0 <bank of (0, b) for b = 0..7>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../fishnet_amd/csrc/psqt_tile.h"

using namespace fnnue;

static_assert(psqt_tile_stride(705) == 708 && psqt_tile_stride(865) == 868, "strides of the shipped geometries");
static_assert(psqt_tile_stride(708) == 708 && psqt_tile_stride(709) == 712, "rounds up to a multiple of 4");

int main(int argc, char** argv) {
  for (int a = 1; a < argc; ++a) {
    const int rows = std::atoi(argv[a]), tile_rows = rows + 1;
    const int stride = psqt_tile_stride(tile_rows), words = psqt_tile_words(tile_rows);
    const int chunks = psqt_fill_chunks(tile_rows);
    std::vector<uint32_t> tile(words, 0xDEADBEEFu);
    std::vector<int> stored(words, 0);
    for (int i = 0; i < chunks; ++i) {
      for (int k = 0; k < 4; ++k) {
        // the chunk's word k in the net's row-major image: row i >> 1, bucket 4 (i & 1) + k
        const uint32_t v = i < 2 * rows ? 8u * (uint32_t)(i >> 1) + 4u * (uint32_t)(i & 1) + (uint32_t)k + 1u : 0u;
        const int w = psqt_tile_word(psqt_fill_row(i), psqt_fill_bucket(i, k), stride);
        if (w < 0 || w >= words) {
          std::printf("error rows %d: chunk %d word %d stored at %d outside [0, %d)\n", rows, i, k, w, words);
          continue;
        }
        tile[w] = v;
        ++stored[w];
      }
    }
    for (int w = 0; w < words; ++w)
      if (stored[w] != 1) std::printf("error rows %d: word %d stored %d times\n", rows, w, stored[w]);
    for (int r = 0; r < stride; ++r)
      for (int b = 0; b < kPsqtTileBuckets; ++b) {
        const int w = psqt_tile_word(r, b, stride);
        const uint32_t want = r < rows ? 8u * (uint32_t)r + (uint32_t)b + 1u : 0u;
        if (w < 0 || w >= words) std::printf("error rows %d: gather (%d, %d) at %d outside the array\n", rows, r, b, w);
        else if (tile[w] != want)
          std::printf("error rows %d: gather (%d, %d) reads %u, wants %u\n", rows, r, b, tile[w], want);
      }
    for (int h = 0; h + 32 <= chunks; h += 32)  // the fill's half-waves: ds_write_b32 counts 32 banks per half
      for (int k = 0; k < 4; ++k) {
        uint32_t seen = 0;
        for (int i = h; i < h + 32; ++i)
          seen |= 1u << (psqt_tile_word(psqt_fill_row(i), psqt_fill_bucket(i, k), stride) & 31);
        if (seen != 0xFFFFFFFFu) std::printf("error rows %d: chunks %d..%d word %d share a bank\n", rows, h, h + 31, k);
      }
    std::printf("geom %d stride %d words %d chunks %d bank0", rows, stride, words, chunks);
    for (int b = 0; b < kPsqtTileBuckets; ++b) std::printf(" %d", psqt_tile_word(0, b, stride) & 31);
    std::printf("\n");
  }
  return 0;
}
