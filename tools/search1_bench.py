"""Phase times of the one-ply search (fnnue_search1_device) on config 4's
shape: N random games (L ~ U[0, 160] plies) with every legal child, HD 1024.
GPU box only.  One JSON line per measurement.

    python tools/search1_bench.py [--games 5000] [--hd 1024] [--runs 3] [--lib PATH] [--actor] [--base-only]
                                  [--lines K[,K...]] [--variant NAME[,NAME...]]

The phases are timed with HIP events on the launch stream, after the workload
ran untimed for 0.3 s:
  children  fnnue_build_children_device (records + moves + end flags)
  eval      fnnue_eval_groups_device(STAR)
  reduce    fnnue_best_children_device
  search1   fnnue_search1_device, the three in one call
  build     fnnue_build_batch_device(CHILDREN): the expansion without moves / flags
  topk@K    fnnue_topk_children_device with K slots per group        (--lines)
  lines@K   fnnue_search1_lines_device with k = K, all in one call   (--lines)
`--lib` loads another build of the library (the parent commit's, which has
only `build` and `eval`): the tool binds the few symbols it needs itself, so
the two builds can alternate on one box (`--base-only` runs just those two on
either build: the same work per iteration, for comparing the evaluation
phase).  FNNUE_CHILDREN_IMPL=ply|record in
the environment picks the children kernel (A/B).  `--actor` adds the engine
actor at depth 0 and 1 for 1, 64 and 1024 lichess-shaped batches; with
`--lines` also go_lines() at depth 1 with multipv = K for every K <= 5.
`--variant crazyhouse,atomic,kingOfTheHill,racingKings,threeCheck` (this tree's library
only) times the variant one-ply search instead, per variant on N random legal
games of the variant (L ~ U[0, 160] plies): fnnue_build_vbatch_device(CHILDREN)
(`build`), fnnue_build_vchildren_device (`children`), fnnue_eval_vgroups_device
(STAR), the reduction and fnnue_vsearch1_device, with the records per ply and
the share of plies beyond 256 children; with `--actor` the engine actor's go()
at variant analysis depth 0 and 1 on 1, 64 and 1024 batches of the variant.
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
START = "rnbqkbnr/pppppppp/8/8/8/8/PPPPPPPP/RNBQKBNR w KQkq - 0 1"
HBM_READ_TBPS = 6.8  # whole 1 KiB rows stream at 6.7-6.9 TB/s
vp, sz = C.c_void_p, C.c_size_t


def bind(path):
    import torch  # noqa: F401  (its HIP runtime first, as fishnet_amd._native does)
    lib = C.CDLL(path)
    P = C.POINTER
    sig = {
        "fnnue_last_error": ([], C.c_char_p),
        "fnnue_net_synthesize": ([C.c_uint64, C.c_uint32, C.c_uint32, P(vp), P(sz)], C.c_int),
        "fnnue_net_load_mem": ([vp, sz, P(vp)], C.c_int),
        "fnnue_ctx_create": ([vp, C.c_int, P(vp)], C.c_int),
        "fnnue_ctx_check": ([vp], C.c_int),
        "fnnue_random_game": ([C.c_uint64, C.c_char_p, C.c_uint32, C.c_char_p, sz, P(sz)], C.c_int),
        "fnnue_build_batch_device": ([vp, vp, vp, vp, sz, C.c_int, vp, sz, vp, sz, P(sz), P(sz), vp], C.c_int),
        "fnnue_eval_groups_device": ([vp, vp, vp, sz, sz, C.c_int, vp, vp, vp], C.c_int),
    }
    new = {
        "fnnue_build_children_device": ([vp, vp, vp, vp, sz, vp, sz, vp, sz, vp, vp, P(sz), P(sz), vp], C.c_int),
        "fnnue_best_children_device": ([vp, vp, vp, vp, vp, vp, sz, sz, vp, vp], C.c_int),
        "fnnue_search1_device": ([vp, vp, vp, vp, sz, vp, sz, vp, sz, P(sz), P(sz), vp], C.c_int),
    }
    lines = {
        "fnnue_topk_children_device": ([vp, vp, vp, vp, vp, vp, sz, sz, vp, vp, sz, vp], C.c_int),
        "fnnue_search1_lines_device": ([vp, vp, vp, vp, sz, C.c_uint32, vp, sz, vp, sz, vp, sz, P(sz), P(sz), vp],
                                       C.c_int),
    }
    has_new = all(hasattr(lib, n) for n in new)
    has_lines = has_new and all(hasattr(lib, n) for n in lines)
    for name, (a, r) in {**sig, **(new if has_new else {}), **(lines if has_lines else {})}.items():
        f = getattr(lib, name)
        f.argtypes, f.restype = a, r
    return lib, has_new, has_lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--games", type=int, default=5000)
    ap.add_argument("--hd", type=int, default=1024)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--seed", type=int, default=4)
    ap.add_argument("--lib", default=os.path.join(ROOT, "fishnet_amd", "libfnnue.so"))
    ap.add_argument("--label", default="")
    ap.add_argument("--actor", action="store_true")
    ap.add_argument("--base-only", action="store_true", help="only build + eval, whatever the library has")
    ap.add_argument("--lines", default="", help="slots per group, e.g. 1,3,5,218: also time the top-k kernel and "
                                                "search1_lines (and go_lines with --actor)")
    ap.add_argument("--variant", default="", help="comma-separated variants: the variant one-ply search instead")
    a = ap.parse_args()
    if a.variant:
        return variant_main(a)
    import torch
    lib, has_new, has_lines = bind(a.lib)
    ks = [int(k) for k in a.lines.split(",") if k]
    if ks and not has_lines:
        raise SystemExit("--lines needs a library with fnnue_topk_children_device")
    label = a.label or ("tree" if has_new else "parent")
    impl = os.environ.get("FNNUE_CHILDREN_IMPL", "record")

    def ok(rc, allow=()):
        if rc and rc not in allow:
            raise RuntimeError(f"rc {rc}: {(lib.fnnue_last_error() or b'').decode()}")
        return rc

    # the text: N games, L ~ U[0, 160] random legal plies each
    rng = np.random.default_rng(a.seed)
    buf, n = C.create_string_buffer(8 * 160 + 16), sz()
    parts, fen_off, mv_off, at = [], [], [], 0
    for i in range(a.games):
        ok(lib.fnnue_random_game(a.seed * 1_000_003 + i, START.encode(), int(rng.integers(0, 161)), buf, len(buf),
                                 C.byref(n)))
        f, m = START.encode(), b" " + buf.value
        fen_off.append(at)
        mv_off.append(at + len(f))
        parts += [f, m]
        at += len(f) + len(m)
    fen_off.append(at)
    text = b"".join(parts)
    dev = torch.device("cuda", 0)
    d_text = torch.frombuffer(bytearray(text), dtype=torch.uint8).to(dev)
    d_fo = torch.tensor(fen_off, dtype=torch.int32, device=dev)
    d_mo = torch.tensor(mv_off, dtype=torch.int32, device=dev)
    T, FO, MO = vp(d_text.data_ptr()), vp(d_fo.data_ptr()), vp(d_mo.data_ptr())

    nb, nl, net, ctx = vp(), sz(), vp(), vp()
    ok(lib.fnnue_net_synthesize(1, a.hd, 0, C.byref(nb), C.byref(nl)))
    ok(lib.fnnue_net_load_mem(nb, nl, C.byref(net)))
    ok(lib.fnnue_ctx_create(net, 0, C.byref(ctx)))

    stream = torch.cuda.Stream(dev)
    S = vp(stream.cuda_stream)
    nrec, ngrp = sz(), sz()
    ok(lib.fnnue_build_batch_device(ctx, T, FO, MO, a.games, 2, None, 0, None, 0, C.byref(nrec), C.byref(ngrp), S),
       allow=(-10,))
    R, G = nrec.value, ngrp.value
    d_pos = torch.empty((R, 36), dtype=torch.uint8, device=dev)
    d_off = torch.empty(G + 1, dtype=torch.int32, device=dev)
    d_mv = torch.empty(R, dtype=torch.int16, device=dev)
    d_end = torch.empty(R, dtype=torch.uint8, device=dev)
    d_ps = torch.empty(R, dtype=torch.int32, device=dev)
    d_po = torch.empty(R, dtype=torch.int32, device=dev)
    d_best = torch.zeros((G, 24), dtype=torch.uint8, device=dev)
    d_best2 = torch.zeros((G, 24), dtype=torch.uint8, device=dev)
    d_goff = torch.empty(a.games + 1, dtype=torch.int32, device=dev)
    PO, OF, MV, EN = vp(d_pos.data_ptr()), vp(d_off.data_ptr()), vp(d_mv.data_ptr()), vp(d_end.data_ptr())
    PS, PP = vp(d_ps.data_ptr()), vp(d_po.data_ptr())
    torch.cuda.synchronize(dev)

    def build():
        ok(lib.fnnue_build_batch_device(ctx, T, FO, MO, a.games, 2, PO, R, OF, G + 1, C.byref(nrec), C.byref(ngrp), S))

    def children():
        ok(lib.fnnue_build_children_device(ctx, T, FO, MO, a.games, PO, R, OF, G + 1, MV, EN, C.byref(nrec),
                                           C.byref(ngrp), S))

    def evaluate():
        ok(lib.fnnue_eval_groups_device(ctx, PO, OF, G, R, 1, PS, PP, S))

    def reduce():
        ok(lib.fnnue_best_children_device(ctx, PS, PP, EN, MV, OF, G, R, vp(d_best.data_ptr()), S))

    def search1():
        ok(lib.fnnue_search1_device(ctx, T, FO, MO, a.games, vp(d_best2.data_ptr()), G, vp(d_goff.data_ptr()),
                                    a.games + 1, C.byref(nrec), C.byref(ngrp), S))

    kmax = max(ks, default=0)
    d_lines = torch.zeros((max(G * kmax, 1), 20), dtype=torch.uint8, device=dev)
    d_loff = {k: (torch.arange(G + 1, dtype=torch.int64, device=dev) * k).to(torch.int32) for k in ks}
    torch.cuda.synchronize(dev)

    def topk(k):
        return lambda: ok(lib.fnnue_topk_children_device(ctx, PS, PP, EN, MV, OF, G, R, vp(d_loff[k].data_ptr()),
                                                         vp(d_lines.data_ptr()), G * k, S))

    def search1_lines(k):
        return lambda: ok(lib.fnnue_search1_lines_device(ctx, T, FO, MO, a.games, k, vp(d_best2.data_ptr()), G,
                                                         vp(d_goff.data_ptr()), a.games + 1, vp(d_lines.data_ptr()),
                                                         G * k, C.byref(nrec), C.byref(ngrp), S))

    phases = [("build", build), ("eval", evaluate)]
    if has_new and not a.base_only:
        # eval right behind build, as on a parent build; children rewrites the same records
        phases = [("build", build), ("eval", evaluate), ("children", children), ("reduce", reduce), ("search1", search1)]
        # the top-k kernel right behind the reduction's own arrays; search1 leaves the same d_best2 either way
        phases[4:4] = [(f"topk@{k}", topk(k)) for k in ks]
        phases += [(f"lines@{k}", search1_lines(k)) for k in ks]

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
        ok(lib.fnnue_ctx_check(ctx))
        return [evs[k].elapsed_time(evs[k + 1]) for k in range(len(phases))] if timed else None

    t0 = time.perf_counter()
    once(False)
    while time.perf_counter() - t0 < 0.3:
        once(False)
    runs = [once(True) for _ in range(a.runs)]
    base = {"lib": label, "children_impl": impl if has_new else None, "games": a.games, "hd": a.hd, "plies": G,
            "records": R}
    for k, (name, _) in enumerate(phases):
        ms = sorted(r[k] for r in runs)
        line = dict(base, phase=name, ms=[round(x, 4) for x in ms], median_ms=round(ms[len(ms) // 2], 4),
                    records_per_s=round(R / (ms[len(ms) // 2] * 1e-3)))
        if name == "reduce":
            lo, hi = (9 * R + 24 * G) / (HBM_READ_TBPS * 1e9), (11 * R + 24 * G) / (HBM_READ_TBPS * 1e9)
            line["byte_floor_ms"] = [round(lo, 4), round(hi, 4)]
            line["times_floor"] = round(ms[len(ms) // 2] / hi, 2)
        if name.startswith("topk@"):  # the reduction's reads plus 20 B per written slot
            k = int(name[5:])
            lo, hi = ((9 * R + 8 * G + 20 * G * k) / (HBM_READ_TBPS * 1e9),
                      (11 * R + 8 * G + 20 * G * k) / (HBM_READ_TBPS * 1e9))
            line["byte_floor_ms"] = [round(lo, 4), round(hi, 4)]
            line["times_floor"] = round(ms[len(ms) // 2] / hi, 2)
        print(json.dumps(line), flush=True)
    if has_new and not a.base_only:
        same = bool(torch.equal(d_best, d_best2))
        digest = hashlib.sha256(d_best2.cpu().numpy().tobytes()).hexdigest()[:16]
        print(json.dumps(dict(base, check="search1 == children + eval + reduce", ok=same, best_sha256=digest)),
              flush=True)
        if not same:
            sys.exit(1)
    if a.actor and has_new:
        actor_lines(a, [k for k in ks if k <= 5])


def actor_lines(a, multipvs=()):
    """The engine actor at depth 0 and 1 on the same lichess-shaped chess batches; go_lines() at depth 1 with
    every batch asking for multipv lines, for each of `multipvs`."""
    sys.path.insert(0, ROOT)
    import fishnet_amd as F
    from fishnet_amd import backend as B
    import bench
    net = F.Net.from_bytes(F.synthesize_net(1, a.hd, 0))
    for nb in (1, 64, 1024):
        bodies = bench.lichess_batches(F, 11, nb, variants=0.0)
        plies = sum(len(b.moves.split()) + 1 for b in bodies)
        for depth, mpv in [(0, 0), (1, 0)] + [(1, m) for m in multipvs]:
            stub, actor = B.channel(net, 0, analysis_depth=depth)
            for b in bodies:
                b.multipv = mpv or None
            go = stub.go_lines if mpv else stub.go
            t0 = time.perf_counter()
            go(bodies)
            while time.perf_counter() - t0 < 0.3:
                go(bodies)
            calls, stats = [], None
            for _ in range(a.runs):
                go(bodies)
                calls.append(stub.last_call_s * 1e3)
                stats = B.last_stats(actor)
            calls.sort()
            med = calls[len(calls) // 2]
            print(json.dumps({"actor_depth": depth, "go_lines_multipv": mpv, "batches": nb, "plies": plies,
                              "line_bytes_per_ply": 20 * mpv, "positions": stats["positions"],
                              "ms_per_call": [round(x, 3) for x in calls], "median_ms": round(med, 3),
                              "plies_per_s": round(plies / (med * 1e-3)),
                              "last_stats": {k: (round(v, 3) if isinstance(v, float) else v) for k, v in stats.items()}}),
                  flush=True)
            actor.close()


VSTART = {"crazyhouse": START.replace(" w", "[] w"), "atomic": START, "kingOfTheHill": START,
          "racingKings": "8/8/8/8/8/8/krbnNBRK/qrbnNBRQ w - - 0 1", "threeCheck": START}


def variant_games(F, variant, name, seed, count, lo, hi):
    """`count` seeded random legal games of the variant, lo..hi plies asked of each (generated on 16 threads)."""
    from concurrent.futures import ThreadPoolExecutor
    rng = np.random.default_rng(seed)
    want = [int(x) for x in rng.integers(lo, hi + 1, count)]
    with ThreadPoolExecutor(16) as ex:
        mvs = list(ex.map(lambda i: F.random_vgame(seed * 1_000_003 + i, variant, VSTART[name], want[i]),
                          range(count)))
    return [(VSTART[name], m) for m in mvs]


def variant_main(a):
    sys.path.insert(0, ROOT)
    import torch
    import fishnet_amd as F
    from fishnet_amd import backend as B
    ids = {"crazyhouse": F.VARIANT_CRAZYHOUSE, "atomic": F.VARIANT_ATOMIC, "kingOfTheHill": F.VARIANT_KINGOFTHEHILL,
           "racingKings": F.VARIANT_RACINGKINGS, "threeCheck": F.VARIANT_THREECHECK}
    dev = torch.device("cuda", 0)
    for name in a.variant.split(","):
        v = ids[name]
        # a threeCheck net is atomic-format bytes under its own id
        fmt = F.VARIANT_ATOMIC if v == F.VARIANT_THREECHECK else v
        net = F.Net.from_bytes_variant(F.synthesize_variant_net(5 + v, a.hd, fmt), v)
        ev = F.Evaluator(net, 0)
        games = variant_games(F, v, name, a.seed, a.games, 0, 160)
        text, fen_off, mv_off = F.pack_games(games)
        d_text = torch.frombuffer(bytearray(text), dtype=torch.uint8).to(dev)
        d_fo = torch.from_numpy(fen_off.view(np.int32)).to(dev)
        d_mo = torch.from_numpy(mv_off.view(np.int32)).to(dev)
        T, FO, MO, ng = d_text.data_ptr(), d_fo.data_ptr(), d_mo.data_ptr(), len(games)
        stream = torch.cuda.Stream(dev)
        S = stream.cuda_stream
        rc, R, G = ev.build_vchildren_device(v, T, FO, MO, ng, 0, 0, 0, 0, 0, 0, S)
        assert rc == -10
        d_pos = torch.empty((R, 48), dtype=torch.uint8, device=dev)
        d_off = torch.empty(G + 1, dtype=torch.int32, device=dev)
        d_mv = torch.empty(R, dtype=torch.int16, device=dev)
        d_end = torch.empty(R, dtype=torch.uint8, device=dev)
        d_ps = torch.empty(R, dtype=torch.int32, device=dev)
        d_po = torch.empty(R, dtype=torch.int32, device=dev)
        d_best = torch.zeros((G, 24), dtype=torch.uint8, device=dev)
        d_best2 = torch.zeros((G, 24), dtype=torch.uint8, device=dev)
        d_goff = torch.empty(ng + 1, dtype=torch.int32, device=dev)
        torch.cuda.synchronize(dev)
        n, g = sz(), sz()
        L = F.nnue.N.lib

        def build():
            F.nnue.N.check(L.fnnue_build_vbatch_device(ev._h, v, vp(T), vp(FO), vp(MO), ng, 2, vp(d_pos.data_ptr()), R,
                                                       vp(d_off.data_ptr()), G + 1, C.byref(n), C.byref(g), vp(S)))

        def children():
            ev.build_vchildren_device(v, T, FO, MO, ng, d_pos.data_ptr(), R, d_off.data_ptr(), G + 1, d_mv.data_ptr(),
                                      d_end.data_ptr(), S)

        def evaluate():
            F.nnue.N.check(L.fnnue_eval_vgroups_device(ev._h, vp(d_pos.data_ptr()), vp(d_off.data_ptr()), G, R, 1,
                                                       vp(d_ps.data_ptr()), vp(d_po.data_ptr()), vp(S)))

        def reduce():
            ev.best_children_device(d_ps.data_ptr(), d_po.data_ptr(), d_end.data_ptr(), d_mv.data_ptr(),
                                    d_off.data_ptr(), G, R, d_best.data_ptr(), S)

        def search1():
            ev.vsearch1_device(v, T, FO, MO, ng, d_best2.data_ptr(), G, d_goff.data_ptr(), ng + 1, S)

        phases = [("build", build), ("eval", evaluate), ("children", children), ("reduce", reduce), ("vsearch1", search1)]

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
        kids = np.diff(d_off.cpu().numpy().view(np.uint32).astype(np.int64)) - 1
        base = {"variant": name, "games": a.games, "hd": a.hd, "plies": G, "records": R,
                "records_per_ply": round(R / G, 2), "max_children": int(kids.max()),
                "plies_beyond_256_children": int((kids > 256).sum()),
                "share_beyond_256": round(float((kids > 256).mean()), 6),
                "plies_beyond_218_children": int((kids > 218).sum())}
        for k, (pname, _) in enumerate(phases):
            ms = sorted(r[k] for r in runs)
            print(json.dumps(dict(base, phase=pname, ms=[round(x, 4) for x in ms], median_ms=round(ms[len(ms) // 2], 4),
                                  records_per_s=round(R / (ms[len(ms) // 2] * 1e-3)))), flush=True)
        same = bool(torch.equal(d_best, d_best2))
        print(json.dumps(dict(base, check="vsearch1 == children + eval + reduce", ok=same,
                              best_sha256=hashlib.sha256(d_best2.cpu().numpy().tobytes()).hexdigest()[:16])), flush=True)
        if not same:
            sys.exit(1)
        ev.close()
        if not a.actor:
            continue
        for nb in (1, 64, 1024):
            bodies = [B.AcquireResponseBody(f"b{i}", fen, mv, variant=name)
                      for i, (fen, mv) in enumerate(variant_games(F, v, name, 11, nb, 40, 160))]
            plies = sum(len(b.moves.split()) + 1 for b in bodies)
            for depth in (0, 1):
                stub, actor = B.channel(net, 0, variant_analysis_depth=depth)
                t0 = time.perf_counter()
                stub.go(bodies)
                while time.perf_counter() - t0 < 0.3:
                    stub.go(bodies)
                calls, stats = [], None
                for _ in range(a.runs):
                    stub.go(bodies)
                    calls.append(stub.last_call_s * 1e3)
                    stats = B.last_stats(actor)
                calls.sort()
                med = calls[len(calls) // 2]
                print(json.dumps({"variant": name, "actor_variant_depth": depth, "batches": nb, "plies": plies,
                                  "positions": stats["positions"], "ms_per_call": [round(x, 3) for x in calls],
                                  "median_ms": round(med, 3), "plies_per_s": round(plies / (med * 1e-3)),
                                  "last_stats": {k: (round(x, 3) if isinstance(x, float) else x)
                                                 for k, x in stats.items()}}), flush=True)
                actor.close()


if __name__ == "__main__":
    main()
