"""kingOfTheHill and racingKings on the GPU: evaluation on nets of their ids
against the variant oracle (the feature set and file format are atomic's, so
the oracle is VariantOracleNet(data, VARIANT_ATOMIC) over the same bytes); the
device batch builder (csrc/vbuilder.hip PlainRules: the chess rule set's
lane-parallel chain with the variants' legality and game ends) against the
host replay (csrc/vboard.h), record for record, in both replay kernels and
across the 64-move window; and whole batches through the engine actor.
The rules themselves are pinned on the host by tests/test_plain_variants.py.
[ref] src/queue.rs:530-539, :545; src/logger.rs:194-201."""
import ctypes as C

import numpy as np
import pytest

import fishnet_amd as F
from fishnet_amd import _native as N
from fishnet_amd import backend as B
from fishnet_amd import nnue
from oracle.oracle import OracleNet, VariantOracleNet
from tests.conftest import net_bytes

pytestmark = pytest.mark.gpu

ZH, AT, KOTH, RK = N.VARIANT_CRAZYHOUSE, N.VARIANT_ATOMIC, N.VARIANT_KINGOFTHEHILL, N.VARIANT_RACINGKINGS
NAME = {0: "standard", ZH: "crazyhouse", AT: "atomic", KOTH: "kingOfTheHill", RK: "racingKings"}
CHESS_START = "rnbqkbnr/pppppppp/8/8/8/8/PPPPPPPP/RNBQKBNR w KQkq - 0 1"
ZH_START = "rnbqkbnr/pppppppp/8/8/8/8/PPPPPPPP/RNBQKBNR[] w KQkq - 0 1"
RK_START = "8/8/8/8/8/8/krbnNBRK/qrbnNBRQ w - - 0 1"
START = {KOTH: CHESS_START, RK: RK_START}
# reversible four-ply shuffles that restore the start position
SHUFFLE = {KOTH: "g1f3 g8f6 f3g1 f6g8", RK: "e1f3 d1c3 f3e1 c3d1"}
# games from the start position that end by the variant's rule after 7 / 8 / 9
# (kingOfTheHill: the white, black, white king steps onto the hill) and
# 11 / 12 / 13 / 12 plies (racingKings: white home first and black too far;
# black home first; white home by a detour; both home: a draw)
KOTH_ENDS = ["e2e4 a7a6 e1e2 a6a5 e2d3 a5a4 d3d4",
             "a2a3 e7e5 a3a4 e8e7 a4a5 e7e6 a5a6 e6d5",
             "e2e4 a7a6 e1e2 a6a5 e2e3 a5a4 e3d3 a4a3 d3d4"]
RK_ENDS = ["h2h3 d1c3 h3h4 c3d1 h4h5 d1c3 h5h6 c3d1 h6g7 d1c3 g7h8",
           "e1f3 a2a3 f3e1 a3a4 e1f3 a4a5 f3e1 a5a6 e1f3 a6b7 f3e1 b7a8",
           "h2h3 d1c3 h3h4 c3d1 h4h5 d1c3 h5g5 c3d1 g5h6 d1c3 h6g7 c3d1 g7h8",
           "h2h3 a2a3 h3h4 a3a4 h4h5 a4a5 h5h6 a5a6 h6g7 a6b7 g7h8 b7a8"]
ENDS = {KOTH: KOTH_ENDS, RK: RK_ENDS}
ROOTS = {KOTH: [CHESS_START, "r3k2r/pppq1ppp/2n2n2/3pp3/3PP3/2N2N2/PPPQ1PPP/R3K2R w KQkq - 0 1",
                "8/2k5/8/8/8/8/5K2/8 w - - 0 1", "8/P6k/8/8/8/8/6Kp/8 w - - 0 1"],
         RK: [RK_START, "8/8/8/8/8/2k2K2/1r4R1/q6Q w - - 0 1", "8/8/K6k/8/8/8/8/2R2r2 w - - 0 1"]}


def padded(variant, reps, tail):
    return " ".join([SHUFFLE[variant]] * reps + [tail]).strip()


@pytest.fixture(scope="module")
def nets():
    cache = {}

    def get(variant, hd):
        if (variant, hd) not in cache:
            data = F.synthesize_variant_net(9 + variant, hd, variant)
            cache[(variant, hd)] = (F.Evaluator(F.Net.from_bytes_variant(data, variant), 0),
                                    VariantOracleNet(data, AT))
        return cache[(variant, hd)]

    yield get
    for ev, _ in cache.values():
        ev.close()


@pytest.fixture(scope="module")
def inputs():
    """Per variant: ~200 random legal games of at most 120 plies as CHAIN groups
    and ~20 games with their children as STAR groups (computed once)."""
    out = {}
    for v in (KOTH, RK):
        chain = F.random_vgames(31 + v, v, 200, 120, threads=8)
        parts, offs, base = [], [np.zeros(1, np.int64)], 0
        for i in range(20):
            fen = ROOTS[v][i % len(ROOTS[v])]
            p, o = nnue.game_vchildren(v, fen, nnue.random_vgame(70 + i, v, fen, 24))
            parts.append(p)
            offs.append(o[1:].astype(np.int64) + base)
            base += len(p)
        out[v] = (chain, (np.concatenate(parts), np.concatenate(offs).astype(np.uint32)))
    return out


def oracle(on, pos):
    ps, po, rc = on.eval_packed(pos, threads=8)
    assert rc == 0
    return ps, po


@pytest.mark.parametrize("variant", [KOTH, RK])
@pytest.mark.parametrize("hd", [256, 1024])
def test_evaluation_matches_the_oracle(nets, inputs, variant, hd):
    """eval_vpositions (the from-scratch plan and ft_slices) and eval_vgroups
    CHAIN / STAR (the segment plans, the chunk form and the small one-workgroup
    form, and ft_segments) on nets of ids 3 and 4."""
    ev, on = nets(variant, hd)
    (cpos, coff), (spos, soff) = inputs[variant]
    walks = F.random_vpositions(5 + hd, variant, 3001, 120)
    for pos in (cpos, walks):
        ps, po = ev.eval_vpositions(pos)
        ops, opo = oracle(on, pos)
        assert np.array_equal(ps, ops) and np.array_equal(po, opo)
    ops, opo = oracle(on, cpos)
    gs, go = ev.eval_vgroups(cpos, coff, N.GROUP_CHAIN)
    assert np.array_equal(gs, ops) and np.array_equal(go, opo)
    few = int(coff[3])  # three games: the small plan
    gs, go = ev.eval_vgroups(cpos[:few], coff[:4], N.GROUP_CHAIN)
    assert np.array_equal(gs, ops[:few]) and np.array_equal(go, opo[:few])
    ops, opo = oracle(on, spos)
    gs, go = ev.eval_vgroups(spos, soff, N.GROUP_STAR)
    assert np.array_equal(gs, ops) and np.array_equal(go, opo)


@pytest.mark.parametrize("variant", [KOTH, RK])
def test_one_king_position_is_invalid(nets, inputs, variant):
    """The (0, 0) game-over record is atomic's alone."""
    ev, _ = nets(variant, 256)
    (cpos, coff), _ = inputs[variant]
    few = int(coff[3])
    for n, ngroups in ((few, 3), (len(cpos), len(coff) - 1)):  # the small plan, the chunk plan
        bad = cpos[:n].copy()
        k = n // 2
        bad[k, :32] &= np.where((bad[k, :32] & 15) == 14, 0xF0, 0xFF).astype(np.uint8)  # drop the black king
        bad[k, :32] &= np.where((bad[k, :32] >> 4) == 14, 0x0F, 0xFF).astype(np.uint8)
        with pytest.raises(F.FnnueError) as e:
            ev.eval_vpositions(bad)
        assert e.value.name == "FNNUE_E_POSITION" and f"index {k}" in str(e.value)
        with pytest.raises(F.FnnueError) as e:
            ev.eval_vgroups(bad, coff[:ngroups + 1], N.GROUP_CHAIN)
        assert e.value.name == "FNNUE_E_POSITION"


def test_multi_evaluator_with_a_racingkings_net(inputs):
    """fnnue_multi_* on a net of id 4 (the image broadcast and the sharded call)."""
    data = F.synthesize_variant_net(3, 256, RK)
    m = F.MultiEvaluator(F.Net.from_bytes_variant(data, RK), [0])
    try:
        pos = inputs[RK][0][0][:4000]
        ps, po = m.eval_vpositions(pos)
        ops, opo = oracle(VariantOracleNet(data, AT), pos)
        assert np.array_equal(ps, ops) and np.array_equal(po, opo)
    finally:
        m.close()


# ---- device builder against host builder ----

@pytest.fixture(scope="module")
def ctx():
    e = F.Evaluator(F.Net.from_bytes(net_bytes(7, 128, 0)), 0)  # the builder needs a ctx (device, stream) only
    yield e
    e.close()


def host_outcome(variant, fen, moves):
    """(positions, None) for a legal game, (None, first failing ply) else."""
    mv = moves.split()
    try:
        return nnue.game_vpositions(variant, fen, moves), None
    except F.FnnueError as e:
        assert e.name == "FNNUE_E_MOVE"
        k = 0
        while True:
            try:
                nnue.game_vpositions(variant, fen, " ".join(mv[:k + 1]))
                k += 1
            except F.FnnueError:
                return None, k + 1


def builder_games(variant):
    """Random games from several roots, and games from the start whose end
    lands at plies 63, 64, 65 (and early, and in the second window); the same
    with a token after the end, and (racingKings) a checking move in the middle
    of the first and of the second window."""
    games = []
    for i in range(40):
        fen = ROOTS[variant][i % len(ROOTS[variant])]
        games.append((fen, nnue.random_vgame(500 + i, variant, fen, 30 + (i * 37) % 150)))
    ends = ENDS[variant]
    for tail in ends:
        n = len(tail.split())
        for target in (n, 63, 64, 65, 64 + n + 4):
            if (target - n) % 4 == 0:
                games.append((START[variant], padded(variant, (target - n) // 4, tail)))
    finished = [g for g in games[40:]]
    assert {len(m.split()) for _, m in finished} >= {63, 64, 65}
    games += [(f, m + " " + SHUFFLE[variant].split()[len(m.split()) % 2]) for f, m in finished]
    if variant == RK:
        games += [(RK_START, padded(RK, r, "e2c3 d1c3")) for r in (5, 15, 16, 20)]  # Nc3+ is no move
        games += [(RK_START, padded(RK, r, "e2g3 d2b3 g3f5")) for r in (5, 15)]    # the same knight, no check
    return games


@pytest.mark.parametrize("variant", [KOTH, RK])
def test_device_builder_plies_match_host_replay(ctx, variant):
    legal, illegal = [], []
    for fen, moves in builder_games(variant):
        pos, ply = host_outcome(variant, fen, moves)
        (legal if ply is None else illegal).append((fen, moves, pos, ply))
    assert len(legal) >= 45 and len(illegal) >= 9
    ends = [nnue.game_end(f, m, variant) for f, m, _, _ in legal[40:]]
    assert all(e & F.END_NO_MOVES for e in ends[:10]) and any(e & F.END_VARIANT for e in ends)
    assert variant == KOTH or F.END_NO_MOVES in ends  # the racingKings draw
    hpos = np.concatenate([p for _, _, p, _ in legal])
    hoff = np.concatenate([[0], np.cumsum([len(p) for _, _, p, _ in legal])])
    for reps in (1, 1100 // len(legal) + 1):  # the two-wave replay; past 1024 games: one wave per game
        pos, off = ctx.build_vbatch(variant, [(f, m) for f, m, _, _ in legal] * reps, N.PLAYOUT_PLIES)
        assert np.array_equal(off[:len(hoff)], hoff) and len(off) == reps * len(legal) + 1
        assert np.array_equal(pos, np.concatenate([hpos] * reps)), reps
    for fen, moves, _, ply in illegal:
        with pytest.raises(F.FnnueError) as e:
            ctx.build_vbatch(variant, [(fen, moves)])
        assert e.value.name == "FNNUE_E_MOVE" and f"ply {ply} of game 0" in str(e.value), (moves, str(e.value))
    # a failing game inside a batch past 1024 games (the one-wave kernel) is named
    fen, moves, _, ply = illegal[-1]
    batch = [(f, m) for f, m, _, _ in legal[:30]] * 35
    with pytest.raises(F.FnnueError) as e:
        ctx.build_vbatch(variant, batch[:1029] + [(fen, moves)] + batch[1029:])
    assert e.value.name == "FNNUE_E_MOVE" and f"ply {ply} of game 1029" in str(e.value)


@pytest.mark.parametrize("variant", [KOTH, RK])
def test_device_builder_children_match_host(ctx, variant):
    games = [(f, m) for f, m in builder_games(variant)[:24]]
    games += [(START[variant], padded(variant, 0, t)) for t in ENDS[variant]]  # finished positions have no children
    games += [(START[variant], padded(variant, 15, ENDS[variant][0]))]
    hp, ho, base = [], [np.zeros(1, np.int64)], 0
    for fen, mv in games:
        p, o = nnue.game_vchildren(variant, fen, mv)
        assert o[-1] - o[-2] == 1 or (fen, mv) in games[:24]
        hp.append(p)
        ho.append(o[1:].astype(np.int64) + base)
        base += len(p)
    for reps in (1, 1100 // len(games) + 1):
        pos, off = ctx.build_vbatch(variant, games * reps, N.PLAYOUT_CHILDREN)
        n = len(np.concatenate(ho))
        assert np.array_equal(off[:n].astype(np.int64), np.concatenate(ho))
        assert np.array_equal(pos[:base], np.concatenate(hp)) and len(pos) == reps * base


def test_device_builder_fen_errors(ctx):
    with pytest.raises(F.FnnueError) as e:  # a pawn in racingKings
        ctx.build_vbatch(RK, [(RK_START, "h2h3"), ("8/8/8/8/8/8/krbnNBRK/qrbnNBPQ w - - 0 1", "")])
    assert e.value.name == "FNNUE_E_FEN" and "game 1" in str(e.value)
    with pytest.raises(F.FnnueError) as e:  # castling rights in racingKings
        ctx.build_vbatch(RK, [("r3k3/8/8/8/8/8/8/4K3 w q - 0 1", "")])
    assert e.value.name == "FNNUE_E_FEN"
    with pytest.raises(F.FnnueError) as e:  # holdings are crazyhouse's
        ctx.build_vbatch(KOTH, [(ZH_START, "e2e4")])
    assert e.value.name == "FNNUE_E_FEN"


# ---- the actor ----

@pytest.fixture(scope="module")
def chan():
    data = {0: net_bytes(1, 256, 0), ZH: F.synthesize_variant_net(5, 256, ZH), AT: F.synthesize_variant_net(6, 256, AT),
            KOTH: F.synthesize_variant_net(7, 256, KOTH), RK: F.synthesize_variant_net(8, 512, RK)}
    stub, actor = B.channel(F.Net.from_bytes(data[0]), 0, crazyhouse=F.Net.from_bytes_variant(data[ZH], ZH),
                            atomic=F.Net.from_bytes_variant(data[AT], AT),
                            kingofthehill=F.Net.from_bytes_variant(data[KOTH], KOTH),
                            racingkings=F.Net.from_bytes_variant(data[RK], RK))
    on = {0: OracleNet(data[0]), ZH: VariantOracleNet(data[ZH], ZH)}
    on.update({v: VariantOracleNet(data[v], AT) for v in (AT, KOTH, RK)})
    yield stub, on
    actor.close()


def body(variant, tag, fen, moves, **kw):
    return B.AcquireResponseBody(tag, fen, moves, variant=NAME[variant], **kw)


def cp(ps, po, norm=361):
    v = int((int(ps) + int(po)) / 16)  # C truncation
    return int(v * 100 / norm)


def check_rows(on, variant, b, rows):
    """Every ply against the oracle; the last ply of a finished game as the
    engine answers it (mate 0 / cp 0, depth 0, nodes 0, no best move)."""
    pos = F.game_positions(b.position, b.moves) if variant == 0 else F.game_vpositions(variant, b.position, b.moves)
    ps, po, rc = on[variant].eval_packed(pos, threads=8)
    assert rc == 0
    assert [r.position_id for r in rows] == list(range(len(ps)))
    assert [r.psqt for r in rows] == ps.tolist() and [r.positional for r in rows] == po.tolist()
    end = F.game_end(b.position, b.moves, variant)
    for k, r in enumerate(rows):
        if k == len(rows) - 1 and end & F.END_NO_MOVES:
            mated = bool(end & (F.END_CHECK | F.END_EXTINCT | F.END_VARIANT))
            assert (r.score.kind, r.score.value, r.depth, r.nodes) == ("mate" if mated else "cp", 0, 0, 0)
            assert r.best_move is None
        else:
            assert (r.score.kind, r.score.value, r.depth, r.nodes) == ("cp", cp(ps[k], po[k]), 0, 1)
    return end


def analysis_bodies():
    bodies, kinds = [], []
    for i in range(8):
        for v, fen in ((0, CHESS_START), (ZH, ZH_START), (AT, CHESS_START), (KOTH, CHESS_START), (RK, RK_START)):
            moves = F.random_game(900 + i, fen, 20 + 9 * i) if v == 0 else F.random_vgame(900 + i, v, fen, 20 + 9 * i)
            bodies.append(body(v, f"{NAME[v]}{i}", fen, moves))
            kinds.append(v)
    for v in (KOTH, RK):
        for k, tail in enumerate(ENDS[v]):
            bodies.append(body(v, f"end{v}.{k}", START[v], padded(v, (k * 7) % 16, tail)))
            kinds.append(v)
    bodies.append(body(KOTH, "after-end", CHESS_START, KOTH_ENDS[0] + " a4a3"))
    kinds.append(KOTH)
    bodies.append(body(RK, "check", RK_START, "e2c3"))
    kinds.append(RK)
    return bodies, kinds


def test_analysis_batches_on_five_nets(chan):
    stub, on = chan
    bodies, kinds = analysis_bodies()
    res = stub.go(bodies)
    ends = {}
    for b, rows, v in zip(bodies, res, kinds):
        if b.batch_id in ("after-end", "check"):
            assert isinstance(rows, B.PositionFailed) and rows.code == -8, b.batch_id
            continue
        assert not isinstance(rows, B.PositionFailed), (b.batch_id, rows)
        ends[b.batch_id] = (check_rows(on, v, b, rows), rows[-1])
    for k in range(3):  # a king on the hill
        end, last = ends[f"end{KOTH}.{k}"]
        assert end == F.END_NO_MOVES | F.END_VARIANT
        assert last.score == B.Score("mate", 0) and (last.depth, last.nodes) == (0, 0)
    for k in range(3):  # racingKings wins
        end, last = ends[f"end{RK}.{k}"]
        assert end == F.END_NO_MOVES | F.END_VARIANT and last.score == B.Score("mate", 0)
    end, last = ends[f"end{RK}.3"]  # both kings home
    assert end == F.END_NO_MOVES and last.score == B.Score("cp", 0) and (last.depth, last.nodes) == (0, 0)


def test_move_work(chan):
    stub, on = chan
    bodies = [body(KOTH, "hill", "8/8/3k4/8/8/3K4/8/8 w - - 0 1", "", work="move"),
              body(RK, "home", "8/K7/8/7k/8/8/8/8 w - - 0 1", "", work="move"),
              body(RK, "catch-up", "8/K6k/8/8/8/8/8/8 w - - 0 1", "a7a8", work="move"),
              body(KOTH, "over", CHESS_START, KOTH_ENDS[0], work="move"),
              body(RK, "drawn", RK_START, RK_ENDS[3], work="move"),
              body(KOTH, "plain", CHESS_START, "e2e4 e7e5", work="move")]
    res = [r[0] for r in stub.go(bodies)]
    assert res[0].best_move in ("d3d4", "d3e4") and res[0].score == B.Score("mate", 1) and res[0].depth == 1
    assert F.game_end(bodies[0].position, res[0].best_move, KOTH) == F.END_NO_MOVES | F.END_VARIANT
    assert res[1].best_move in ("a7a8", "a7b8") and res[1].score == B.Score("mate", 1)
    # black must catch up (a draw, 0); every other move loses at once and is never chosen
    assert res[2].best_move in ("h7g8", "h7h8") and res[2].score == B.Score("cp", 0) and res[2].nodes == 5
    assert res[3].best_move is None and res[3].score == B.Score("mate", 0) and (res[3].depth, res[3].nodes) == (0, 0)
    assert res[4].best_move is None and res[4].score == B.Score("cp", 0)
    pos, off = F.game_vchildren(KOTH, CHESS_START, "e2e4 e7e5")
    kids = pos[off[-2] + 1: off[-1]]
    ps, po, rc = on[KOTH].eval_packed(kids, threads=8)
    vals = [-int((int(a) + int(b)) / 16) for a, b in zip(ps, po)]
    assert res[5].nodes == len(kids) and res[5].score == B.Score("cp", int(max(vals) * 100 / 361))
    after = F.game_vpositions(KOTH, CHESS_START, "e2e4 e7e5 " + res[5].best_move)[-1]
    assert np.array_equal(after, kids[int(np.argmax(vals))])


def test_routing():
    chess = F.Net.from_bytes(net_bytes(1, 256, 0))
    stub, actor = B.channel(chess, 0)
    try:
        res = stub.go([body(KOTH, "koth", CHESS_START, "e2e4"), body(RK, "rk", RK_START, "h2h3"),
                       B.AcquireResponseBody("anti", CHESS_START, "e2e4", variant="antichess"),
                       B.AcquireResponseBody("std", CHESS_START, "e2e4")])
        assert [getattr(r, "code", 0) for r in res] == [-4, -4, -4, 0]
    finally:
        actor.close()
    # one net through fnnue_backend_channel goes to its own variant's slot
    koth = F.Net.from_bytes_variant(F.synthesize_variant_net(7, 256, KOTH), KOTH)
    stub, actor = B.channel(koth, 0)
    try:
        res = stub.go([body(KOTH, "koth", CHESS_START, "e2e4"), body(AT, "at", CHESS_START, "e2e4"),
                       B.AcquireResponseBody("anti", CHESS_START, "e2e4", variant="antichess")])
        assert [getattr(r, "code", 0) for r in res] == [0, -4, -4]
    finally:
        actor.close()
    # two nets of one variant
    other = F.Net.from_bytes_variant(F.synthesize_variant_net(8, 256, KOTH), KOTH)
    arr = (C.c_void_p * 3)(chess._h.value, koth._h.value, other._h.value)
    h = C.c_void_p()
    rc = N.lib.fnnue_backend_channel_netv(arr, 3, 0, None, C.byref(h))
    assert rc == -1 and not h.value and "two kingofthehill nets" in N.lib.fnnue_last_error().decode()
    with pytest.raises(F.FnnueError) as e:
        B.channel(chess, 0, kingofthehill=chess)
    assert e.value.name == "FNNUE_E_ARG"


def test_compact_form_equals_full_records(chan):
    stub, _ = chan
    bodies, _ = analysis_bodies()
    bodies += [body(KOTH, "hill", "8/8/3k4/8/8/3K4/8/8 w - - 0 1", "", work="move"),
               body(RK, "catch-up", "8/K6k/8/8/8/8/8/8 w - - 0 1", "a7a8", work="move"),
               body(KOTH, "over", CHESS_START, KOTH_ENDS[0], work="move"),
               body(RK, "skip", RK_START, RK_ENDS[3], skip_positions=[0, 2])]
    full = stub.go(bodies)
    comp = stub.go_compact(bodies)
    key = lambda r: (r.position_id, r.score, r.psqt, r.positional, r.depth, r.nodes, r.best_move, r.skipped, r.matrix)
    for b, f, c in zip(bodies, full, comp):
        if isinstance(f, B.PositionFailed):
            assert isinstance(c, B.PositionFailed) and c.code == f.code, b.batch_id
            continue
        assert [key(r) for r in f] == [key(r) for r in c], b.batch_id
