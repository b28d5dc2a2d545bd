// slice_units.h — how the plan cuts the items of ft_slices into units and where
// it puts them in the unit table (DESIGN §4.2 "Schedule").  Plain integer
// arithmetic shared by plan_scan_body (sliced_common.h) and the host test
// (tests/slice_units_host.cpp): no HIP types, compiles with any C++14 compiler.
//
// The items of a king block are sorted by list length n, and a pass of 8 items
// costs a wave about kSliceCostPass + kSliceCostRow * (n - 1) VALU
// instructions, n from 2 to 32: a fixed count of items makes units whose work
// differs 3x.  Here a king block holding work w is cut into m = round(w / W)
// units (at least one) of equal work w / m, so a block ends in no runt unit,
// and each cut is moved to the nearest multiple of 128 items from the block's
// start (whole pass steps; write_rows' parity pairing).
//
// The unit table is then ordered for the grid of ft_slices, which runs table
// entry e on XCD e % 8 and hands an XCD its entries in increasing e: blocks by
// decreasing work per unit (ties: king block), the units of a block in item
// order, dealt over the eight XCDs in snake order (row r of eight goes
// 0..7 for even r, 7..0 for odd r).  Every XCD then runs its units by
// decreasing work, the units of a block stay adjacent on each XCD (they share
// tiles in its L2), a big block is spread over all eight, and the XCD sums
// differ by at most one unit of the lightest row.
#pragma once
#include <stdint.h>

#ifdef __HIPCC__
#define FNNUE_HD __host__ __device__
#else
#define FNNUE_HD
#endif

namespace fnnue {

// Work of one item of list length n (the own king included), in VALU
// instructions of its wave's pass.
constexpr uint32_t kSliceCostPass = 35, kSliceCostRow = 3;
FNNUE_HD constexpr uint32_t slice_item_cost(uint32_t n) { return kSliceCostPass + kSliceCostRow * (n ? n - 1 : 0); }
constexpr uint32_t kSliceCostMax = slice_item_cost(32);

// Work budget of a unit.  6144 items of config 2's mean list (22.15 pieces,
// cost 98.5) are 605,000; see DESIGN §4.2 for the sweep.
#ifndef FT_UNIT_WORK
#define FT_UNIT_WORK 907000
#endif
constexpr uint32_t kUnitWork = FT_UNIT_WORK;
// A batch of long lists would make more units than one of short lists: the
// budget rises with the batch's mean cost so that the units of item ranges stay
// at most one per king block + one per kUnitCapItems items (slice_max_units).
// kUnitCapItems = the items of a budget at list length 20: batches whose mean
// list is shorter keep kUnitWork.
constexpr uint32_t kUnitCapItems = kUnitWork / slice_item_cost(20);
// Cuts are rounded to 128 items, so two cuts must lie at least 128 items
// apart: units hold >= 3/4 of a budget (slice_block_units), i.e. at least
// 3/4 * kUnitWork / kSliceCostMax items.
static_assert(kUnitWork / 4 * 3 / kSliceCostMax >= 256, "units of at least two pass steps");
static_assert(kUnitCapItems >= 128, "cap of at least one pass step");

// The budget for a batch of `items` items holding `work` in all:
// max(unit_work, ceil(work / ceil(items / kUnitCapItems))).
FNNUE_HD inline uint32_t slice_budget(uint32_t work, uint32_t items, uint32_t unit_work = kUnitWork) {
  const uint32_t cap = (items + kUnitCapItems - 1) / kUnitCapItems;
  const uint32_t need = cap ? (work + cap - 1) / cap : 0;
  return need > unit_work ? need : unit_work;
}

// Units of a king block holding work w: round(w / W), at least one; none for
// an empty block.  For m >= 2: m <= w / W + 1/2 and w >= 3 W / 2, so a unit's
// work w / m >= W / (1 + W / 2w) >= 3 W / 4.
FNNUE_HD inline uint32_t slice_block_units(uint32_t w, uint32_t W) {
  if (w == 0) return 0;
  const uint32_t m = (w + W / 2) / W;
  return m ? m : 1;
}

// Upper bound of the unit count of any batch of at most `items` items over
// `blocks` king blocks.  Proof: a non-empty block makes
// m_k = max(1, round(w_k / W)) <= 1 + w_k / W units, so the sum is at most
// blocks + work / W; W >= work / cap with cap = ceil(items / kUnitCapItems)
// (slice_budget), so work / W <= cap, and cap grows with items.
FNNUE_HD constexpr uint32_t slice_max_units(uint32_t items, uint32_t blocks) {
  return blocks + (items + kUnitCapItems - 1) / kUnitCapItems;
}

// Work below which cut u (1 <= u < m) of a block of work w in m units falls:
// floor(u w / m) = u (w / m) + floor(u (w % m) / m), in 32 bits (u, m < 2^16).
// Cut 0 is the block's start.
FNNUE_HD inline uint32_t slice_cut_work(uint32_t u, uint32_t w, uint32_t m) {
  return u * (w / m) + u * (w % m) / m;
}
// Item offset (from the block's start) of a cut at work `target` that falls in
// the bin of items of cost c starting at item offset x0 and work p0 (the last
// bin with p0 <= target; it is not empty, the next bin's offset being larger):
// the item holding that work, rounded to the nearest pass step.
FNNUE_HD inline uint32_t slice_cut_item(uint32_t target, uint32_t p0, uint32_t x0, uint32_t c) {
  return (x0 + (target - p0) / c + 64) / 128 * 128;
}

// Table entry of the unit of rank r (0 = most work) among nu units: snake deal
// over 8 columns.  The last row, when it is partial, is dealt forwards so that
// the table has no holes (its units are the lightest).
FNNUE_HD inline uint32_t slice_table_slot(uint32_t r, uint32_t nu) {
  const uint32_t row = r >> 3, col = r & 7;
  const bool back = (row & 1) && (row + 1) * 8 <= nu;
  return row * 8 + (back ? 7 - col : col);
}

}  // namespace fnnue
