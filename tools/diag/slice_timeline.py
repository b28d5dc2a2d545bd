"""Timeline of ft_slices' (unit, slice) tasks from the diagnostic build
(tools/exp/diag_slicetrace.patch -> exp/libfnnue_diag_slicetrace.so): which CU /
XCD ran each task, when it started, when each of its 16 waves finished, and
the unit's item range.  Reports, for config 2's positions: per-XCD last end,
CU occupancy per twentieth of the launch, slice-0 tasks against the others, how
far apart the sixteen waves of a task end (wave_ends: first-to-last end over the
task's duration, mean live waves; mean / p50 / p90, slice 0 / others), and a
least-squares fit of the task duration

    us = fill + passes * a + rows * b        (x slice0 for slice-0 tasks)

passes = 128-item pass steps of the unit, rows = sum over its passes of
(longest n of the pass - 1): a / b is the simulator's --pass-cost / --row-cost
(tools/diag/slice_schedule_sim.py), fill its constant.

usage (GPU box): FNNUE_LIB=$PWD/exp/libfnnue_diag_slicetrace.so python tools/diag/slice_timeline.py [--out file.json]
"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))


def wave_end_spread(start, ends, passes, sl):
    """How the sixteen waves of a task end (all times in ns; ends[task, wave]).
    spread_frac: first-to-last wave end over the task's duration.  live_waves:
    the mean number of waves still running over the task, sum of the waves'
    lifetimes over the task's duration (16 = all waves end together).
    spread_over_pass: the spread in units of the task's own mean pass step
    (duration / 128-item pass steps).  Tasks of fewer than 16 passes leave
    waves idle from the start and are reported apart (short_tasks)."""
    dur = (ends.max(axis=1) - start).astype(np.float64)
    spread = (ends.max(axis=1) - ends.min(axis=1)).astype(np.float64)
    live = (ends - start[:, None]).sum(axis=1) / dur

    def stats(v):
        if len(v) == 0:
            return None
        return {"mean": round(float(v.mean()), 4), "p50": round(float(np.median(v)), 4),
                "p90": round(float(np.percentile(v, 90)), 4)}

    out = {}
    full = passes >= 2  # every wave has at least its two static passes
    for name, m in (("all", full), ("slice0", full & (sl == 0)), ("others", full & (sl != 0))):
        out[name] = {"tasks": int(m.sum()), "spread_frac": stats(spread[m] / dur[m]), "live_waves": stats(live[m]),
                     "spread_us": stats(spread[m] / 1e3),
                     "spread_over_pass": stats(spread[m] / (dur[m] / passes[m]))}
    out["short_tasks"] = int((~full).sum())
    # time-weighted: the share of resident wave slots that hold a running wave
    out["live_waves_time_weighted"] = round(float((ends - start[:, None]).sum() / dur.sum()), 3)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--hd", type=int, default=1024)
    ap.add_argument("--positions", type=int, default=1_000_000)
    ap.add_argument("--out", default="slice_timeline.json")
    args = ap.parse_args()
    import torch
    import fishnet_amd as F
    from fishnet_amd import _native as N
    from slice_schedule_sim import histogram
    lib = N.lib
    lib.fnnue_diag_slice_trace.argtypes = [C.c_void_p, C.c_size_t, C.c_int]
    pos = F.random_playouts(1, args.positions, 0, 160, threads=16)
    cnt = histogram(pos)
    ev = F.Evaluator(F.Net.from_bytes(F.synthesize_net(1, args.hd)), 0)
    ev.set_ft_impl(N.FT_SLICED)
    dev = torch.device("cuda", 0)
    d_pos = torch.from_numpy(pos).to(dev)
    n = len(pos)
    out = torch.zeros((2, n), dtype=torch.int32, device=dev)
    for _ in range(30):  # the clock ramp
        ev.eval_positions_device(d_pos.data_ptr(), n, out[0].data_ptr(), out[1].data_ptr(), None)
    ev.check()
    assert lib.fnnue_diag_slice_trace(None, 0, 1) == 0
    torch.cuda.synchronize()
    ev.eval_positions_device(d_pos.data_ptr(), n, out[0].data_ptr(), out[1].data_ptr(), None)
    ev.check()
    tr = np.zeros(((1 << 15), 20), np.uint64)
    assert lib.fnnue_diag_slice_trace(tr.ctypes.data, tr.nbytes, 0) == 0
    S = args.hd // 64
    live = np.nonzero(tr[:, 0])[0]
    t = tr[live].astype(np.int64)
    t0 = t[:, 0].min()
    start = (t[:, 0] - t0) * 10  # s_memrealtime: 100 MHz -> ns
    ends = (t[:, 2:18] - t0) * 10
    end = ends.max(axis=1)
    hw = t[:, 1] & 0xFFFFFFFF
    xcc = (t[:, 1] >> 32) & 0xF
    cu_key = xcc * 1000 + ((hw >> 13) & 7) * 100 + ((hw >> 12) & 1) * 16 + ((hw >> 8) & 0xF)
    span = end.max()
    dur = end - start
    first, last, kb = t[:, 18] & 0xFFFFFFFF, t[:, 18] >> 32, t[:, 19]
    sl = live % S
    # passes and rows of every unit from the histogram (items of a block are sorted by n)
    nb = np.concatenate([np.repeat(np.arange(33), cnt[b]) for b in range(32)])
    passes, rows = np.zeros(len(live)), np.zeros(len(live))
    cache = {}
    for i, (a, b) in enumerate(zip(first, last)):
        if (a, b) not in cache:
            v = nb[a:b]
            pad = (-len(v)) % 128
            v = np.concatenate([v, np.repeat(v[-1:], pad)]).reshape(-1, 128)
            cache[(a, b)] = (v.shape[0], float((v.max(axis=1) - 1).sum()))
        passes[i], rows[i] = cache[(a, b)]
    ucu = np.unique(cu_key)
    res = {"hd": args.hd, "positions": int(n), "tasks": int(len(live)), "units": int(len(live) // S),
           "cus_seen": int(len(ucu)), "kernel_span_us": round(span / 1e3, 1),
           "task_us": {"mean": round(dur.mean() / 1e3, 2), "p50": round(float(np.median(dur)) / 1e3, 2),
                       "max": round(dur.max() / 1e3, 2)},
           "cu_busy_frac_mean": round(float(dur.sum() / len(ucu) / span), 3),
           "per_xcd_last_end_us": [round(float(end[xcc == x].max()) / 1e3, 1) if np.any(xcc == x) else None
                                   for x in range(8)],
           "per_xcd_busy_us": [round(float(dur[xcc == x].sum()) / 1e3, 1) for x in range(8)],
           "last_task_start_us": round(float(start.max()) / 1e3, 1)}
    edges = np.linspace(0, span, 21)
    res["cu_occupancy_by_twentieth"] = [
        round(float(np.clip(np.minimum(end, b) - np.maximum(start, a), 0, None).sum() / (b - a) / len(ucu)), 3)
        for a, b in zip(edges[:-1], edges[1:])]
    res["task_us_by_slice"] = {"slice0": round(float(dur[sl == 0].mean()) / 1e3, 2),
                               "others": round(float(dur[sl != 0].mean()) / 1e3, 2)}
    res["wave_ends"] = wave_end_spread(start, ends, passes, sl)
    fit = {}
    for name, m in (("others", sl != 0), ("slice0", sl == 0)):
        A = np.stack([np.ones(m.sum()), passes[m], rows[m]], axis=1)
        coef, *_ = np.linalg.lstsq(A, dur[m] / 1e3, rcond=None)
        resid = dur[m] / 1e3 - A @ coef
        fit[name] = {"fill_us": round(float(coef[0]), 3), "us_per_pass": round(float(coef[1]), 4),
                     "us_per_row": round(float(coef[2]), 5), "rms_us": round(float(np.sqrt((resid ** 2).mean())), 3)}
    res["fit"] = fit
    o = fit["others"]
    res["sim_constants"] = {"pass_cost_over_row_cost": round(o["us_per_pass"] / o["us_per_row"], 2),
                            "fill_share_of_mean_task": round(o["fill_us"] / float(dur[sl != 0].mean() / 1e3), 3),
                            "slice0": round(float(dur[sl == 0].mean() / dur[sl != 0].mean()), 3)}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    json.dump(res, open(args.out, "w"), indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
