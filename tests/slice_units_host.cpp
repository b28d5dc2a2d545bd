// Host driver of fishnet_amd/csrc/slice_units.h for tests/test_slice_units.py:
// reads a histogram (KB, then KB x 33 item counts by king block and list
// length), builds the unit table with the helper's arithmetic in the order
// plan_scan_body uses it (per block: work, units, rank; then every cut), and prints
//   W <budget> nu <units> bound <slice_max_units>
//   <table entry> <kb> <first item> <end> <written>      one line per entry
// Items are numbered over the whole batch (blocks in order), as in the plan.
// <written> counts the stores to the entry's four words (4 = each once).
#include <cstdio>
#include <vector>

#include "../fishnet_amd/csrc/slice_units.h"

using namespace fnnue;

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  FILE* f = std::fopen(argv[1], "r");
  if (!f) return 2;
  int KB = 0;
  if (std::fscanf(f, "%d", &KB) != 1 || KB < 1 || KB > 64) return 2;
  const int NB = 33;
  std::vector<uint32_t> cnt(KB * NB), s(KB * NB), pb(KB * NB);
  for (auto& c : cnt)
    if (std::fscanf(f, "%u", &c) != 1) return 2;
  std::fclose(f);
  uint32_t items = 0;
  for (int i = 0; i < KB * NB; ++i) {
    s[i] = items;
    items += cnt[i];
  }
  std::vector<uint32_t> bw(KB), bm(KB), ubase(KB);
  uint32_t work = 0;
  for (int kb = 0; kb < KB; ++kb) {
    uint32_t w = 0;
    for (int b = 0; b < NB; ++b) {
      pb[kb * NB + b] = w;
      w += cnt[kb * NB + b] * slice_item_cost(b);
    }
    bw[kb] = w;
    work += w;
  }
  const uint32_t W = slice_budget(work, items);
  uint32_t nu = 0;
  for (int kb = 0; kb < KB; ++kb) nu += bm[kb] = slice_block_units(bw[kb], W);
  for (int t = 0; t < KB; ++t) {
    const uint32_t key = bm[t] ? bw[t] / bm[t] : 0;
    uint32_t first = 0;
    for (int j = 0; j < KB; ++j) {
      const uint32_t kj = bm[j] ? bw[j] / bm[j] : 0;
      if (kj > key || (kj == key && j < t)) first += bm[j];
    }
    ubase[t] = first;
  }
  const uint32_t bound = slice_max_units(items, KB);
  // a table larger than the bound so that a bad slot shows instead of crashing
  std::vector<int> uw(4 * (size_t)(nu > bound ? nu : bound) + 64, -1), written((nu > bound ? nu : bound) + 16, 0);
  auto store = [&](uint32_t entry, int word, int v) {
    if (entry >= written.size()) {
      std::printf("error slot %u out of the table\n", entry);
      return;
    }
    uw[4 * entry + word] = v;
    ++written[entry];
  };
  for (int t = 0; t < KB; ++t) {
    const uint32_t m = bm[t];
    if (!m) continue;
    const uint32_t e0 = slice_table_slot(ubase[t], nu), e1 = slice_table_slot(ubase[t] + m - 1, nu);
    const uint32_t end = t == KB - 1 ? items : s[(t + 1) * NB];
    store(e0, 0, t);
    store(e0, 1, (int)s[t * NB]);
    store(e0, 3, 0);
    store(e1, 2, (int)end);
  }
  for (int kb = 0; kb < KB; ++kb) {
    const uint32_t w = bw[kb], m = bm[kb], first = ubase[kb], b0 = s[kb * NB];
    for (uint32_t u = 1; u < m; ++u) {
      const uint32_t target = slice_cut_work(u, w, m);
      int b = -1;
      for (int k = 0; k < NB; ++k) b += pb[kb * NB + k] <= target ? 1 : 0;
      const int i = kb * NB + b;
      const int at = (int)(b0 + slice_cut_item(target, pb[i], s[i] - b0, slice_item_cost(i % NB)));
      const uint32_t e0 = slice_table_slot(first + u, nu), e1 = slice_table_slot(first + u - 1, nu);
      store(e0, 0, kb);
      store(e0, 1, at);
      store(e0, 3, 0);
      store(e1, 2, at);
    }
  }
  std::printf("W %u nu %u bound %u\n", W, nu, bound);
  for (uint32_t e = 0; e < written.size(); ++e)
    if (written[e]) std::printf("%u %d %d %d %d\n", e, uw[4 * e], uw[4 * e + 1], uw[4 * e + 2], written[e]);
  return 0;
}
