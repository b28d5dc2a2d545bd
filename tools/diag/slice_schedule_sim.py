"""CPU model of one ft_slices launch: how the plan's units fill 8 XCDs x 32 CUs.

No GPU.  Over config 2's positions (random playouts, seed 1, L ~ U[0, 160], as
bench.py's positions workload) the items are binned by (king block, n) as
plan_count bins them, cut into units by a rule, placed in the unit table by a
rule, and the launch is replayed:

  pass    128 items (16 waves x 8); a wave's pass costs
          --pass-cost + --row-cost * (longest n of its 8 items - 1)
  task    (unit, slice): its slowest wave + a constant for the drain and the
          tile fill, --fill-share of the mean 6144-item task; slice-0 tasks
          cost x --slice0 (PSQT)
  grid    table entry e runs on XCD e % 8; an XCD's tasks are handed in grid
          order (entry, then slice) to whichever of its 32 CUs frees first
  score   makespan / (row work / 256 CUs), and the XCD finish-time spread
          (first XCD to finish / last)

Cutting rules: fixed:<items> (units of that many items from each block's
start, the plan before the work-budget units) and work:<budget> (slice_units.h:
round(w / W) units of equal work per block, cuts on multiples of 128 items; the
budget is in the helper's own cost units, 35 + 3 (n - 1) per item whatever the
task constants given here).  Placement rules: block (table in
block order), snake (blocks by decreasing work per unit, snake deal over the 8
XCDs: slice_table_slot), lpt (units by decreasing cost, each to the least
loaded XCD; holes allowed, the model only).

  usage: python tools/diag/slice_schedule_sim.py [--positions 1000000]
             [--rule fixed:6144:block work:907000:snake ...] [--out file.json]
"""
from __future__ import annotations

import argparse
import heapq
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))

KING_BUCKET = np.full(64, -1, dtype=np.int64)
for _sq in range(64):
    _r, _f = divmod(_sq, 8)
    if _f >= 4:
        KING_BUCKET[_sq] = 4 * (7 - _r) + (7 - _f)

COST_PASS, COST_ROW = 35, 3  # slice_units.h: kSliceCostPass, kSliceCostRow
CAP_N = 20                   # kUnitCapItems = budget / slice_item_cost(20)


def histogram(pos: np.ndarray) -> np.ndarray:
    """cnt[kb, n]: perspective-items per king block and piece count."""
    raw = pos.reshape(-1, 36)
    board = np.empty((len(raw), 64), dtype=np.int64)
    board[:, 0::2], board[:, 1::2] = raw[:, :32] & 15, raw[:, :32] >> 4
    n = (board != 0).sum(axis=1)
    cnt = np.zeros((32, 33), dtype=np.int64)
    for persp in (0, 1):
        ksq = np.argmax(board == (6 if persp == 0 else 14), axis=1)
        flip = (56 if persp else 0) ^ np.where(ksq % 8 < 4, 7, 0)
        np.add.at(cnt, (KING_BUCKET[ksq ^ flip], n), 1)
    return cnt


def item_cost(n):
    return COST_PASS + COST_ROW * np.maximum(n - 1, 0)


def cut_fixed(cnt: np.ndarray, items: int):
    """Units as (kb, first item, end) in block order, items counted from the block's start."""
    units = []
    for kb in range(cnt.shape[0]):
        e = int(cnt[kb].sum())
        units += [(kb, c, min(e, c + items)) for c in range(0, e, items)]
    return units


def cut_work(cnt: np.ndarray, budget: int):
    """slice_units.h: the same integer arithmetic as plan_scan_body."""
    ns = np.arange(cnt.shape[1])
    work = cnt * item_cost(ns)[None, :]
    tot_items, tot_work = int(cnt.sum()), int(work.sum())
    cap_items = budget // int(item_cost(np.int64(CAP_N)))
    cap = -(-tot_items // cap_items)
    W = max(budget, -(-tot_work // cap)) if cap else budget
    units = []
    for kb in range(cnt.shape[0]):
        w = int(work[kb].sum())
        if w == 0:
            continue
        m = max(1, (w + W // 2) // W)
        p = np.concatenate([[0], np.cumsum(work[kb])])
        x = np.concatenate([[0], np.cumsum(cnt[kb])])
        cuts = [0]
        for u in range(1, m):
            t = u * w // m
            b = int(np.searchsorted(p, t, side="right")) - 1
            cuts.append((int(x[b]) + (t - int(p[b])) // int(item_cost(np.int64(b))) + 64) // 128 * 128)
        cuts.append(int(x[-1]))
        units += [(kb, cuts[i], cuts[i + 1], w // m) for i in range(m)]
    return units


def snake_slot(r: int, nu: int) -> int:
    row, col = r >> 3, r & 7
    back = (row & 1) and (row + 1) * 8 <= nu
    return row * 8 + (7 - col if back else col)


def simulate(cnt, units, place, a, slices=16):
    """units: (kb, first, end[, key]).  Returns the score of the launch."""
    # per-unit: the slowest wave's cost; wave v of pass k holds items first + 128 k + 8 v .. + 7
    nb = np.concatenate([np.repeat(np.arange(cnt.shape[1]), cnt[kb]) for kb in range(cnt.shape[0])])
    start = np.concatenate([[0], np.cumsum(cnt.sum(axis=1))])
    row_work = 0.0
    cost = []
    for u in units:
        kb, b, e = u[:3]
        n = nb[start[kb] + b:start[kb] + e]
        pad = (-len(n)) % 128
        full = np.concatenate([n, np.repeat(n[-1:], pad)]).reshape(-1, 16, 8)
        c = a.pass_cost + a.row_cost * (full.max(axis=2) - 1)  # [pass, wave]
        live = (np.arange(full.shape[0] * 128).reshape(-1, 16, 8)[:, :, 0] < len(n))
        wave = (c * live).sum(axis=0)
        cost.append(float(wave.max()))
        row_work += float((a.pass_cost + a.row_cost * (n - 1)).sum()) / 8 / 16
    cost = np.array(cost)
    # the constant: fill_share of the mean full fixed-6144 task
    mean6144 = 48 * (a.pass_cost + a.row_cost * (float((nb * 1.0).mean()) - 1))
    const = a.fill_share * mean6144
    nu = len(units)
    if place == "block":
        xcd = [[] for _ in range(8)]
        for e in range(nu):
            xcd[e % 8].append(e)
    elif place == "snake":
        order = sorted(range(nu), key=lambda i: (-units[i][3], units[i][0], units[i][1]))
        table = [None] * nu
        for r, i in enumerate(order):
            table[snake_slot(r, nu)] = i
        xcd = [[table[e] for e in range(x, nu, 8)] for x in range(8)]
    elif place == "lpt":
        order = sorted(range(nu), key=lambda i: (-cost[i], units[i][0], units[i][1]))
        load, xcd = [0.0] * 8, [[] for _ in range(8)]
        for i in order:
            x = int(np.argmin(load))
            load[x] += cost[i]
            xcd[x].append(i)
    else:
        raise SystemExit(f"unknown placement {place}")
    ends = []
    for x in range(8):
        cus = [0.0] * 32
        heapq.heapify(cus)
        for i in xcd[x]:
            for s in range(slices):
                t = heapq.heappop(cus)
                heapq.heappush(cus, t + (cost[i] + const) * (a.slice0 if s == 0 else 1.0))
        ends.append(max(cus))
    ideal = row_work * (slices + a.slice0 - 1) / 256  # row_work: one task's waves, perfectly divisible
    return {"units": nu, "ratio": max(ends) / ideal, "xcd_spread": min(ends) / max(ends),
            "xcd_end": [e / ideal for e in ends]}


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--positions", type=int, default=1_000_000)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--pass-cost", type=float, default=35.0)
    ap.add_argument("--row-cost", type=float, default=3.0)
    ap.add_argument("--fill-share", type=float, default=0.07)
    ap.add_argument("--slice0", type=float, default=1.3)
    ap.add_argument("--rule", nargs="*", default=["fixed:4096:block", "fixed:5120:block", "fixed:6144:block",
                                                  "fixed:7168:block", "fixed:8192:block", "fixed:6144:lpt",
                                                  "work:605000:block", "work:605000:snake", "work:756000:snake",
                                                  "work:907000:snake", "work:1210000:snake", "work:907000:lpt"])
    ap.add_argument("--hist", help="npy file of a [32, 33] histogram instead of playing positions out")
    ap.add_argument("--out")
    a = ap.parse_args()
    if a.hist:
        cnt = np.load(a.hist)
    else:
        from fishnet_amd import nnue as F
        cnt = histogram(F.random_playouts(a.seed, a.positions, 0, 160, threads=8))
    res = {"items": int(cnt.sum()), "mean_n": float((cnt.sum(axis=0) * np.arange(33)).sum() / cnt.sum()), "rules": {}}
    print(f"{res['items']} items, mean n {res['mean_n']:.2f}")
    print(f"{'rule':24s} {'units':>5s} {'ratio':>7s} {'XCD spread':>10s}")
    for rule in a.rule:
        kind, size, place = rule.split(":")
        units = cut_fixed(cnt, int(size)) if kind == "fixed" else cut_work(cnt, int(size))
        if kind == "fixed":  # key for the snake order: the unit's own item count
            units = [u + (u[2] - u[1],) for u in units]
        r = simulate(cnt, units, place, a)
        res["rules"][rule] = r
        print(f"{rule:24s} {r['units']:5d} {r['ratio']:7.3f} {r['xcd_spread']:10.3f}", flush=True)
    if a.out:
        json.dump(res, open(a.out, "w"), indent=1)


if __name__ == "__main__":
    main()
