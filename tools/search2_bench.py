"""Times of the two-ply search (fnnue_search2_device) and of the engine actor
at two plies.  GPU box only.  One JSON line per measurement.

    python tools/search2_bench.py [--games 200] [--plies 60] [--hd 1024] [--runs 3] [--actor] [--lines 3,218] [--draws N] [--quiesce D] [--quiesce-checks]
                                  [--variant crazyhouse|atomic|kingofthehill|racingkings|threecheck]

The shape: N random legal games of L plies each from the start position
(default 200 x 60: ~12k plies, ~400k children, ~13M grandchild records, a few
chunks of the default FNNUE_SEARCH2_RECORDS budget).  Timed with HIP events on
the launch stream, after the workload ran untimed for 0.3 s:
  search1   fnnue_search1_device on the same games (the one-ply search)
  search2   fnnue_search2_device, everything in one call
then one more search2 call with FNNUE_SEARCH2_TRACE=1, whose phases the
library times itself with HIP events between them and prints to stderr
(`FNNUE_SEARCH2_TRACE {...}`): level1 (replay, the plies' children), child
states, the children's counts and the sizing read-back, then over the chunks
the grandchild expansion, their STAR evaluation and the first reduction, and
the second reduction.  records_per_s counts the records each search evaluates
(search1: plies + children; search2: the grandchild records, which hold every
child once more).
`--lines K,...` adds fnnue_[v]search2_lines_device at those k (phases
search2_lines_kK, in the same process on the same games, behind search2), and
the traced call then runs with the first k, so that its line carries the
ranking kernel's own time (topk_ms).
`--actor` adds the engine actor's go_pv() at 1 and 2 plies on 1 and 64
lichess-shaped chess batches; with `--lines` also go_lines_pv() on the same
2-plies channel and the same batches asking for multipv 3.
`--variant NAME` measures fnnue_vsearch1_device / fnnue_vsearch2_device on
random legal games of that variant instead (a synthetic variant net; the atomic
net for kingofthehill, racingkings and threecheck), and with `--actor` the
actor's go_pv() at 1 and 2 variant plies on batches of that variant;
`--draws N` adds N interleaved rounds of search2 with the draw rules
(fnnue_set_search_draws; with `--variant` the variants': fnnue_set_search_vdraws; `--shuffle` makes every game
of the variant a long knight shuffle, whose plies are nearly all on the rules' list) off and on, in this process
on the same games (phases
search2_draws_off / _on: median, min, max), and traced calls with the rules on,
whose line carries history_ms, mark_ms and draw_list (the plies on the list).
`--quiesce D` (chess, or with `--variant` the variants' quiescence: fnnue_set_search_vquiesce) adds interleaved rounds (`--runs` of them, at least 3) of search1 and search2 with the
capture quiescence depth (fnnue_set_search_quiesce) at 0, 1, .. D, in this process on the same games (phases
search1_quiesce_d / search2_quiesce_d: median, min, max of the device time between two events, and the host's
wall time, which holds the level read-backs), and one traced search2 call per depth, whose line carries
quiesce_ms, the per-level record counts and the slice count.  With `--quiesce-checks` every depth above 0 is
measured twice in the same rounds, quiescence checks (fnnue_set_search_quiesce_checks) off and on (phases
search1_quiesce_d / search2_quiesce_d and ..._d_checks), and the traced calls with the setting on carry
quiesce_evasions and quiesce_in_check per level (the evasion records, the nodes in check that had one).
`--piece-plies A,B,...` repeats the 2-plies actor lines with those values of
FNNUE_BACKEND_PIECE_PLIES (a two-plies piece is a 1024th of it).
"""
import argparse
import ctypes as C
import hashlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
START = "rnbqkbnr/pppppppp/8/8/8/8/PPPPPPPP/RNBQKBNR w KQkq - 0 1"
VARIANTS = {"crazyhouse": ("VARIANT_CRAZYHOUSE", START.replace(" w", "[] w"), "crazyhouse"),
            "atomic": ("VARIANT_ATOMIC", START, "atomic"),
            "kingofthehill": ("VARIANT_KINGOFTHEHILL", START, "kingOfTheHill"),
            "racingkings": ("VARIANT_RACINGKINGS", "8/8/8/8/8/8/krbnNBRK/qrbnNBRQ w - - 0 1", "racingKings"),
            "threecheck": ("VARIANT_THREECHECK", START, "threeCheck")}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--games", type=int, default=200)
    ap.add_argument("--plies", type=int, default=60)
    ap.add_argument("--hd", type=int, default=1024)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--seed", type=int, default=4)
    ap.add_argument("--actor", action="store_true")
    ap.add_argument("--variant", choices=sorted(VARIANTS), default=None)
    ap.add_argument("--piece-plies", default="")
    ap.add_argument("--lines", default="")
    ap.add_argument("--draws", type=int, default=0)
    ap.add_argument("--shuffle", action="store_true")
    ap.add_argument("--quiesce", type=int, default=0)
    ap.add_argument("--quiesce-checks", action="store_true")
    a = ap.parse_args()
    import torch
    import fishnet_amd as F
    from fishnet_amd import _native as N

    vid = getattr(N, VARIANTS[a.variant][0]) if a.variant else 0
    if a.variant:
        root = VARIANTS[a.variant][1]
        games = [(root, F.random_vgame(a.seed * 1_000_003 + i, vid, root, a.plies)) for i in range(a.games)]
        if a.shuffle:  # knights going out and back from the start: every ply after the 8th is on the draw rules' list
            back = "e2g3 d2b3 g3e2 b3d2" if a.variant == "racingkings" else "g1f3 g8f6 f3g1 f6g8"
            games = [(root, " ".join(back.split() * (a.plies // 4))) for _ in range(a.games)]
    else:
        games = [(START, F.random_game(a.seed * 1_000_003 + i, START, a.plies)) for i in range(a.games)]
    text, fen_off, mv_off = F.pack_games(games)
    dev = torch.device("cuda", 0)
    d_text = torch.frombuffer(bytearray(text), dtype=torch.uint8).to(dev)
    d_fo = torch.from_numpy(fen_off.view(np.int32)).to(dev)
    d_mo = torch.from_numpy(mv_off.view(np.int32)).to(dev)
    T, FO, MO, ng = d_text.data_ptr(), d_fo.data_ptr(), d_mo.data_ptr(), len(games)
    if a.variant:  # the atomic net also serves kingofthehill, racingkings and threecheck
        made_as = N.VARIANT_CRAZYHOUSE if vid == N.VARIANT_CRAZYHOUSE else N.VARIANT_ATOMIC
        ev = F.Evaluator(F.Net.from_bytes_variant(F.synthesize_variant_net(5, a.hd, made_as), made_as), 0)
    else:
        ev = F.Evaluator(F.Net.from_bytes(F.synthesize_net(1, a.hd, 0)), 0)
    stream = torch.cuda.Stream(dev)
    S = stream.cuda_stream
    plies = sum(len(m.split()) + 1 for _, m in games)
    d_b1 = torch.zeros((plies, N.BEST_BYTES), dtype=torch.uint8, device=dev)
    d_b2 = torch.zeros((plies, N.BEST2_BYTES), dtype=torch.uint8, device=dev)
    d_goff = torch.empty(ng + 1, dtype=torch.int32, device=dev)
    torch.cuda.synchronize(dev)

    def search1():
        if a.variant:
            ev.vsearch1_device(vid, T, FO, MO, ng, d_b1.data_ptr(), plies, d_goff.data_ptr(), ng + 1, S)
        else:
            ev.search1_device(T, FO, MO, ng, d_b1.data_ptr(), plies, d_goff.data_ptr(), ng + 1, S)

    def search2():
        if a.variant:
            ev.vsearch2_device(vid, T, FO, MO, ng, d_b2.data_ptr(), plies, d_goff.data_ptr(), ng + 1, S)
        else:
            ev.search2_device(T, FO, MO, ng, d_b2.data_ptr(), plies, d_goff.data_ptr(), ng + 1, S)

    ks = [int(x) for x in a.lines.split(",") if x]
    d_lines = torch.zeros((plies * max(ks + [0]), N.LINE2_BYTES), dtype=torch.uint8, device=dev)

    def search2_lines(k):
        def run():
            if a.variant:
                ev.vsearch2_lines_device(vid, T, FO, MO, ng, k, d_b2.data_ptr(), plies, d_goff.data_ptr(), ng + 1,
                                         d_lines.data_ptr(), plies * k, S)
            else:
                ev.search2_lines_device(T, FO, MO, ng, k, d_b2.data_ptr(), plies, d_goff.data_ptr(), ng + 1,
                                        d_lines.data_ptr(), plies * k, S)
        return run

    phases = [("search1", search1), ("search2", search2)] + [(f"search2_lines_k{k}", search2_lines(k)) for k in ks]

    def once(timed):
        evs = [torch.cuda.Event(enable_timing=True) for _ in range(len(phases) + 1)] if timed else None
        with torch.cuda.stream(stream):
            for k, (_, fn) in enumerate(phases):
                if timed:
                    evs[k].record(stream)
                fn()
            if timed:
                evs[-1].record(stream)
        stream.synchronize()
        ev.check()
        return [evs[k].elapsed_time(evs[k + 1]) for k in range(len(phases))] if timed else None

    t0 = time.perf_counter()
    once(False)
    while time.perf_counter() - t0 < 0.3:
        once(False)
    runs = [once(True) for _ in range(a.runs)]
    b1 = d_b1.cpu().numpy().view(F.BEST_DTYPE).reshape(-1)
    b2 = d_b2.cpu().numpy().view(F.BEST2_DTYPE).reshape(-1)
    children = int(b1["nodes"].sum())
    grand_records = int(b2["nodes"].sum())  # every child's own record + its children
    assert a.variant or int(b2["nodes"].max()) <= 219 * 219
    base = {"variant": a.variant or "chess", "games": ng, "hd": a.hd, "plies": plies, "children": children, "grandchild_records": grand_records,
            "budget": int(os.environ.get("FNNUE_SEARCH2_RECORDS", 16 << 20))}
    for k, (name, _) in enumerate(phases):
        ms = sorted(r[k] for r in runs)
        rec = plies + children if name == "search1" else grand_records
        print(json.dumps(dict(base, phase=name, ms=[round(x, 4) for x in ms], median_ms=round(ms[len(ms) // 2], 4),
                              records=rec, records_per_s=round(rec / (ms[len(ms) // 2] * 1e-3)))), flush=True)
    kinds = {int(k): int((b2["kind"] == k).sum()) for k in np.unique(b2["kind"])}
    print(json.dumps(dict(base, check="kinds and pv lengths", kinds=kinds,
                          pv_len={int(k): int((b2["pv_len"] == k).sum()) for k in np.unique(b2["pv_len"])},
                          best2_sha256=hashlib.sha256(b2.tobytes()).hexdigest()[:16])), flush=True)
    # the phases, timed by the library itself (its line goes to stderr)
    os.environ["FNNUE_SEARCH2_TRACE"] = "1"
    for _ in range(a.runs):
        with torch.cuda.stream(stream):
            (search2_lines(ks[0]) if ks else search2)()
        stream.synchronize()
    os.environ["FNNUE_SEARCH2_TRACE"] = "0"
    if a.draws:
        draws_rounds(a, ev, stream, search2, base)
    if a.quiesce:
        quiesce_rounds(a, ev, stream, search1, search2, base)
    ev.close()
    if a.actor and a.variant:
        vactor_lines(a, vid)
    elif a.actor:
        actor_lines(a)


def draws_rounds(a, ev, stream, search2, base):
    """search2 with the draw rules off and on, interleaved in this process on the same games; then traced
    calls with the rules on (history_ms, mark_ms and draw_list in the library's line)."""
    import torch

    def timed():
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        with torch.cuda.stream(stream):
            e0.record(stream)
            search2()
            e1.record(stream)
        stream.synchronize()
        ev.check()
        return e0.elapsed_time(e1)

    # a variant net's context has its own switch (fnnue_set_search_vdraws)
    set_draws = ev.set_search_vdraws if a.variant else ev.set_search_draws
    ms = {False: [], True: []}
    for _ in range(a.draws):
        for on in (False, True):
            set_draws(on)
            ms[on].append(timed())
    for on in (False, True):
        v = sorted(ms[on])
        print(json.dumps(dict(base, phase="search2_draws_" + ("on" if on else "off"), rounds=a.draws,
                              ms=[round(x, 4) for x in v], median_ms=round(v[len(v) // 2], 4), min_ms=round(v[0], 4),
                              max_ms=round(v[-1], 4))), flush=True)
    set_draws(True)
    os.environ["FNNUE_SEARCH2_TRACE"] = "1"
    for _ in range(a.runs):
        with torch.cuda.stream(stream):
            search2()
        stream.synchronize()
    os.environ["FNNUE_SEARCH2_TRACE"] = "0"
    set_draws(False)


def quiesce_rounds(a, ev, stream, search1, search2, base):
    """search1 and search2 at quiescence depth 0..D, interleaved in this process on the same games; then one traced
    search2 call per depth (quiesce_ms, quiesce_records per level and quiesce_slices in the library's line)."""
    import torch

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0 = time.perf_counter()
        with torch.cuda.stream(stream):
            e0.record(stream)
            fn()
            e1.record(stream)
        stream.synchronize()
        wall = (time.perf_counter() - t0) * 1e3
        ev.check()
        return e0.elapsed_time(e1), wall

    def setting(d, checks):  # a variant net's context has one setter for both (fnnue_set_search_vquiesce)
        if a.variant:
            ev.set_search_vquiesce(d, checks)
        else:
            ev.set_search_quiesce(d)
            ev.set_search_quiesce_checks(checks)

    depths = [(d, False) for d in range(a.quiesce + 1)]
    if a.quiesce_checks:  # every depth above 0 with the setting off and on, interleaved
        depths = sorted(depths + [(d, True) for d in range(1, a.quiesce + 1)])
    rounds = max(a.runs, 3)
    ms = {(n, d): [] for n in ("search1", "search2") for d in depths}
    for _ in range(rounds):
        for d, checks in depths:
            setting(d, checks)
            ms[("search1", (d, checks))].append(timed(search1))
            ms[("search2", (d, checks))].append(timed(search2))
    for (name, (d, checks)), v in ms.items():
        dev_ms, wall = sorted(x[0] for x in v), sorted(x[1] for x in v)
        print(json.dumps(dict(base, phase=f"{name}_quiesce_{d}" + ("_checks" if checks else ""), rounds=rounds,
                              ms=[round(x, 4) for x in dev_ms],
                              median_ms=round(dev_ms[len(dev_ms) // 2], 4), min_ms=round(dev_ms[0], 4),
                              max_ms=round(dev_ms[-1], 4), wall_median_ms=round(wall[len(wall) // 2], 4))), flush=True)
    os.environ["FNNUE_SEARCH2_TRACE"] = "1"
    for d, checks in depths[1:]:
        setting(d, checks)
        with torch.cuda.stream(stream):
            search2()
        stream.synchronize()
    os.environ["FNNUE_SEARCH2_TRACE"] = "0"
    setting(0, False)


def actor_lines(a):
    """The engine actor at 1 and 2 plies on the same lichess-shaped chess batches."""
    import fishnet_amd as F
    from fishnet_amd import backend as B
    import bench
    net = F.Net.from_bytes(F.synthesize_net(1, a.hd, 0))
    for nb in (1, 64):
        bodies = bench.lichess_batches(F, 11, nb, variants=0.0)
        plies = sum(len(b.moves.split()) + 1 for b in bodies)
        for n in (1, 2):
            stub, actor = B.channel(net, 0, analysis_plies=n)
            t0 = time.perf_counter()
            stub.go_pv(bodies)
            while time.perf_counter() - t0 < 0.3:
                stub.go_pv(bodies)
            calls, stats = [], None
            for _ in range(a.runs):
                stub.go_pv(bodies)
                calls.append(stub.last_call_s * 1e3)
                stats = B.last_stats(actor)
            calls.sort()
            med = calls[len(calls) // 2]
            print(json.dumps({"actor_plies": n, "batches": nb, "plies": plies, "positions": stats["positions"],
                              "ms_per_call": [round(x, 3) for x in calls], "median_ms": round(med, 3),
                              "plies_per_s": round(plies / (med * 1e-3)),
                              "positions_per_s": round(stats["positions"] / (med * 1e-3)),
                              "last_stats": {k: (round(v, 3) if isinstance(v, float) else v) for k, v in stats.items()}}),
                  flush=True)
            if n == 2 and a.lines:  # MultiPV 3 on the same channel and batches: go_lines_pv() beside go_pv()
                asking = [B.AcquireResponseBody(b.batch_id, b.position, b.moves, b.work, b.variant, b.skip_positions, 3)
                          for b in bodies]
                for name, fn, bs in (("go_pv", stub.go_pv, asking), ("go_lines_pv", stub.go_lines_pv, asking)):
                    t0 = time.perf_counter()
                    fn(bs)
                    while time.perf_counter() - t0 < 0.3:
                        fn(bs)
                    calls = []
                    for _ in range(a.runs):
                        res = fn(bs)
                        calls.append(stub.last_call_s * 1e3)
                    calls.sort()
                    nlines = sum(len(r.lines or ()) for rows in res for r in rows)
                    print(json.dumps({"actor_plies": 2, "call": name, "multipv": 3, "batches": nb, "plies": plies,
                                      "lines": nlines, "ms_per_call": [round(x, 3) for x in calls],
                                      "median_ms": round(calls[len(calls) // 2], 3)}), flush=True)
            actor.close()


def vactor_lines(a, vid):
    """The engine actor at 1 and 2 variant plies on lichess-shaped batches of one variant (40-160 plies
    each), the two-plies lines once per piece size asked for."""
    import fishnet_amd as F
    from fishnet_amd import _native as N
    from fishnet_amd import backend as B
    _, root, name = VARIANTS[a.variant]
    made_as = N.VARIANT_CRAZYHOUSE if vid == N.VARIANT_CRAZYHOUSE else N.VARIANT_ATOMIC
    data = F.synthesize_variant_net(5, a.hd, made_as)
    rng = np.random.default_rng(11)
    cuts = [None] + [int(x) for x in a.piece_plies.split(",") if x]
    for nb in (1, 64):
        bodies = [B.AcquireResponseBody(f"b{i}", root, F.random_vgame(11_000_033 + i, vid, root, int(rng.integers(40, 161))),
                                        variant=name) for i in range(nb)]
        plies = sum(len(b.moves.split()) + 1 for b in bodies)
        for n, cut in [(1, None)] + [(2, c) for c in cuts]:
            if cut is None:
                os.environ.pop("FNNUE_BACKEND_PIECE_PLIES", None)
            else:
                os.environ["FNNUE_BACKEND_PIECE_PLIES"] = str(cut)
            stub, actor = B.channel(None, 0, **{a.variant: F.Net.from_bytes_variant(data, vid)},
                                    variant_analysis_plies=n)
            t0 = time.perf_counter()
            stub.go_pv(bodies)
            while time.perf_counter() - t0 < 0.3:
                stub.go_pv(bodies)
            calls, stats = [], None
            for _ in range(a.runs):
                stub.go_pv(bodies)
                calls.append(stub.last_call_s * 1e3)
                stats = B.last_stats(actor)
            calls.sort()
            med = calls[len(calls) // 2]
            print(json.dumps({"variant": a.variant, "actor_plies": n, "piece_plies": cut or 524288, "batches": nb,
                              "plies": plies, "positions": stats["positions"],
                              "ms_per_call": [round(x, 3) for x in calls], "median_ms": round(med, 3),
                              "plies_per_s": round(plies / (med * 1e-3)),
                              "positions_per_s": round(stats["positions"] / (med * 1e-3)),
                              "last_stats": {k: (round(v, 3) if isinstance(v, float) else v) for k, v in stats.items()}}),
                  flush=True)
            actor.close()
    os.environ.pop("FNNUE_BACKEND_PIECE_PLIES", None)


if __name__ == "__main__":
    main()
