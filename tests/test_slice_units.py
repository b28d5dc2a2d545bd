"""The unit cutting and placement of ft_slices (fishnet_amd/csrc/slice_units.h) on the host.

tests/slice_units_host.cpp is built with the host compiler and run on
histograms chosen to break the helper; the table it prints is checked here:
units tile every king block exactly, starts are multiples of 128 items from the
block's start, the count stays within slice_max_units, every table entry below
the count is written once, and the eight XCDs (entry % 8) get equal work.

XCD balance.  Units enter the table by decreasing work per unit in snake order,
so two XCD sums differ by at most the largest unit's work (each pair of rows
contributes at most its first minus its last, which telescopes), plus what
rounding the cuts to 128 items moves: at most 64 items x cost 128 at each end
of a unit, for one unit per table row on each of the two XCDs compared.  That
absolute bound is asserted for every case.  On config 2's own histogram
(tests/golden/slice_units_config2_hist.txt: bench.py's positions workload,
random_playouts(1, 1_000_000, 0, 160)) the helper reaches max / min = 1.013 at
the shipped budget, and the test asserts 1.02 there.  A smaller batch has fewer
table rows to even out one unit's difference (half of config 2: 1.046), so for
every other input of at least eight budgets the stated ratio is the absolute
bound above over the lightest XCD's load.
"""
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COST = 35 + 3 * np.maximum(np.arange(33) - 1, 0)  # slice_item_cost
COST_MAX = int(COST[32])
BENCH_RATIO = 1.02

pytestmark = pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")


@pytest.fixture(scope="module")
def prog(tmp_path_factory):
    exe = tmp_path_factory.mktemp("slice_units") / "slice_units_host"
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", os.path.join(ROOT, "tests/slice_units_host.cpp"),
                    "-o", str(exe)], check=True)
    return str(exe)


def run(prog, tmp_path, cnt):
    cnt = np.asarray(cnt, dtype=np.int64)
    path = tmp_path / "hist.txt"
    path.write_text(f"{cnt.shape[0]}\n" + "\n".join(" ".join(map(str, r)) for r in cnt) + "\n")
    out = subprocess.run([prog, str(path)], check=True, capture_output=True, text=True).stdout.splitlines()
    assert not [l for l in out if l.startswith("error")], out
    head = out[0].split()
    W, nu, bound = int(head[1]), int(head[3]), int(head[5])
    table = np.array([[int(v) for v in l.split()] for l in out[1:]], dtype=np.int64).reshape(-1, 5)
    return W, nu, bound, table


def check(cnt, W, nu, bound, table):
    """The invariants of any table; returns the eight XCD loads."""
    cnt = np.asarray(cnt, dtype=np.int64)
    assert nu <= bound
    # every entry below the count exactly once (each of its four words stored once), none beyond
    assert sorted(table[:, 0].tolist()) == list(range(nu))
    assert (table[:, 4] == 4).all()
    table = table[np.argsort(table[:, 0])]
    starts = np.concatenate([[0], np.cumsum(cnt.sum(axis=1))])
    work_before = np.concatenate([[0], np.cumsum((cnt * COST[None, :]).reshape(-1))])  # by item bin
    item_before = np.concatenate([[0], np.cumsum(cnt.reshape(-1))])

    def work_at(item):  # work of the items before `item`
        b = int(np.searchsorted(item_before, item, side="right")) - 1
        b = min(b, cnt.size - 1)
        return int(work_before[b]) + (item - int(item_before[b])) * int(COST[b % 33])

    loads = np.zeros(8, dtype=np.int64)
    unit_work = []
    for kb in range(cnt.shape[0]):
        mine = table[table[:, 1] == kb]
        mine = mine[np.argsort(mine[:, 2])]
        if starts[kb + 1] == starts[kb]:
            assert len(mine) == 0
            continue
        assert len(mine) >= 1
        assert mine[0, 2] == starts[kb] and mine[-1, 3] == starts[kb + 1]
        assert (mine[1:, 2] == mine[:-1, 3]).all()      # tile the block exactly
        assert (mine[:, 3] > mine[:, 2]).all()          # no empty unit
        assert ((mine[:, 2] - starts[kb]) % 128 == 0).all()
        for e, _, a, b, _ in mine:
            w = work_at(int(b)) - work_at(int(a))
            loads[e % 8] += w
            unit_work.append(w)
    rows = (nu + 7) // 8
    if nu:
        assert loads.max() - loads.min() <= max(unit_work) + 2 * 2 * 64 * COST_MAX * rows
    return loads


def hist(blocks=32):
    return np.zeros((blocks, 33), dtype=np.int64)


def bench_hist():
    return np.loadtxt(os.path.join(ROOT, "tests/golden/slice_units_config2_hist.txt"), dtype=np.int64).reshape(32, 33)


def cases():
    c = {}
    c["empty"] = hist()
    h = hist(); h[5, 2] = 1; c["one_item"] = h
    h = hist(); h[31, 32] = 20000; c["one_block_one_n"] = h       # test_same_king_block_everywhere's shape
    h = hist(); h[7, 20] = 128 * 90; c["exactly_128k"] = h
    h = hist(); h[7, 20] = 128 * 90 + 1; c["128k_plus_1"] = h
    h = hist(); h[:31, 3] = 1; h[31, 24] = 200_000; c["31_tiny_1_big"] = h
    h = hist(); h[:, 2:] = 700; c["every_n"] = h
    h = hist(); h[:, 10] = 100; c["below_one_budget"] = h
    # the cap binds (every item at the longest list) and 31 blocks hold one item: units = bound or bound - 1
    h = hist(); h[:31, 32] = 1; h[31, 32] = 2_000_000 - 31; c["at_the_bound"] = h
    h = hist(); h[:, 32] = 62_500; c["all_longest"] = h
    return c


@pytest.mark.parametrize("name", list(cases()))
def test_unit_table_invariants(prog, tmp_path, name):
    cnt = cases()[name]
    W, nu, bound, table = run(prog, tmp_path, cnt)
    check(cnt, W, nu, bound, table)
    if name == "empty":
        assert nu == 0
    if name in ("one_item", "below_one_budget", "128k_plus_1", "exactly_128k"):
        assert nu == int((cnt.sum(axis=1) > 0).sum())   # one unit per non-empty block
    if name == "at_the_bound":
        assert nu >= bound - 1


def test_random_histograms(prog, tmp_path):
    rng = np.random.default_rng(7)
    for _ in range(40):
        cnt = hist()
        scale = int(10 ** rng.uniform(0, 5.3))
        mask = rng.random((32, 33)) < rng.uniform(0.05, 1.0)
        cnt[:, 2:] = (rng.integers(0, scale + 1, size=(32, 31)) * mask[:, 2:])
        cnt = (cnt * min(1.0, 2_000_000 / max(1, cnt.sum()))).astype(np.int64)
        check(cnt, *run(prog, tmp_path, cnt))


def test_xcd_balance_on_config2(prog, tmp_path):
    cnt = bench_hist()
    W, nu, bound, table = run(prog, tmp_path, cnt)
    loads = check(cnt, W, nu, bound, table)
    print("XCD loads", loads.tolist(), "max/min", loads.max() / loads.min())
    assert loads.max() / loads.min() <= BENCH_RATIO


@pytest.mark.parametrize("scale", [0.5, 0.1, 0.05])
def test_xcd_balance_on_smaller_batches(prog, tmp_path, scale):
    cnt = (bench_hist() * scale).astype(np.int64)
    W, nu, bound, table = run(prog, tmp_path, cnt)
    loads = check(cnt, W, nu, bound, table)             # asserts the absolute bound
    assert loads.sum() >= 8 * W                         # at least eight budgets
    print("XCD loads", loads.tolist(), "max/min", loads.max() / loads.min())


def test_config2_units_per_block_are_adjacent_per_xcd(prog, tmp_path):
    """On each XCD the units of a king block follow one another (they share tiles in its L2), and a
    block of at least 15 units is on all eight XCDs (a shorter run of ranks can turn at the end of a
    snake row and miss a column)."""
    cnt = bench_hist()
    W, nu, bound, table = run(prog, tmp_path, cnt)
    table = table[np.argsort(table[:, 0])]
    for x in range(8):
        kbs = table[x::8, 1].tolist()
        runs = [k for i, k in enumerate(kbs) if i == 0 or kbs[i - 1] != k]
        assert len(runs) == len(set(runs))
    for kb in range(32):
        mine = table[table[:, 1] == kb]
        if len(mine) >= 15:
            assert len(set((mine[:, 0] % 8).tolist())) == 8
