"""threeCheck on the GPU: evaluation on a net of id 5 against the variant oracle
(the feature set and file format are atomic's: VariantOracleNet(data,
VARIANT_ATOMIC) over the same bytes); the device batch builder
(csrc/vbuilder.hip PlainRules<kVariantThreeCheck>: the chess chain with the
check counters counted lane-parallel, one ballot per 64-move window) against
the host replay (csrc/vboard.h) record for record, in both replay kernels,
with the three checks before, across and after the window boundary and from
roots whose carried-in counters differ; the children expansion and the one-ply
search; and whole batches through the engine actor.  The rules themselves are
pinned on the host by tests/test_three_check.py."""
import numpy as np
import pytest

import fishnet_amd as F
from fishnet_amd import _native as N
from fishnet_amd import backend as B
from fishnet_amd import nnue
from oracle.oracle import OracleNet, VariantOracleNet
from tests.conftest import net_bytes

pytestmark = pytest.mark.gpu

TC, AT, KOTH = N.VARIANT_THREECHECK, N.VARIANT_ATOMIC, N.VARIANT_KINGOFTHEHILL
START = "rnbqkbnr/pppppppp/8/8/8/8/PPPPPPPP/RNBQKBNR w KQkq - 0 1"
LOST = F.END_NO_MOVES | F.END_VARIANT | F.END_CHECK
SHUFFLE = "g1f3 g8f6 f3g1 f6g8"  # four plies that restore the position and give no check
WHITE_THIRD = "e2e4 e7e5 d1h5 b8c6 h5f7 e8f7 f1c4 f7e8 c4f7"         # checks on plies 5, 7, 9
BLACK_THIRD = "a2a3 e7e5 a3a4 d8h4 b1c3 h4f2 e1f2 f8c5 f2e1 c5f2"    # checks on plies 6, 8, 10
NAMED = (WHITE_THIRD, BLACK_THIRD)
ROOTS = [START, "r1bqk2r/pppp1ppp/2n2n2/2b1p3/2B1P3/2N2N2/PPPP1PPP/R1BQK2R w KQkq - 2+2 4 5",
         "4k3/8/8/8/8/8/r2R4/4K3 w - - 1+3 0 1", "8/P6k/8/8/8/8/6Kp/8 w - - 0 1 +1+2"]


def with_counters(w, b):
    return START[:-3] + f"{w}+{b} 0 1"


def padded(reps, tail):
    return " ".join([SHUFFLE] * reps + [tail]).strip()


def cut_at_end(fen, moves):
    """The game's moves up to the first position without a legal move (the host's flags)."""
    ms = moves.split()
    for q in range(len(ms) + 1):
        if nnue.game_end(fen, ms[:q], TC) & F.END_NO_MOVES:
            return " ".join(ms[:q])
    return moves


@pytest.fixture(scope="module")
def nets():
    cache = {}

    def get(hd):
        if hd not in cache:
            data = F.synthesize_variant_net(9 + TC, hd, AT)
            net = F.Net.from_bytes_variant(data, TC)
            assert net.variant == TC
            cache[hd] = (F.Evaluator(net, 0), VariantOracleNet(data, AT))
        return cache[hd]

    yield get
    for ev, _ in cache.values():
        ev.close()


@pytest.fixture(scope="module")
def inputs():
    """200 random legal games of at most 120 plies as CHAIN groups and 20 games with their children as STAR
    groups (computed once)."""
    chain = F.random_vgames(36, TC, 200, 120, threads=8)
    parts, offs, base = [], [np.zeros(1, np.int64)], 0
    for i in range(20):
        fen = ROOTS[i % len(ROOTS)]
        p, o = nnue.game_vchildren(TC, fen, nnue.random_vgame(70 + i, TC, fen, 24))
        parts.append(p)
        offs.append(o[1:].astype(np.int64) + base)
        base += len(p)
    return chain, (np.concatenate(parts), np.concatenate(offs).astype(np.uint32))


def oracle(on, pos):
    ps, po, rc = on.eval_packed(pos, threads=8)
    assert rc == 0
    return ps, po


@pytest.mark.parametrize("hd", [256, 1024])
def test_evaluation_matches_the_oracle(nets, inputs, hd):
    """eval_vpositions and eval_vgroups CHAIN / STAR / the small plan on a net of id 5, bit-exact."""
    ev, on = nets(hd)
    (cpos, coff), (spos, soff) = inputs
    ops, opo = oracle(on, cpos)
    ps, po = ev.eval_vpositions(cpos)
    assert np.array_equal(ps, ops) and np.array_equal(po, opo)
    gs, go = ev.eval_vgroups(cpos, coff, N.GROUP_CHAIN)
    assert np.array_equal(gs, ops) and np.array_equal(go, opo)
    few = int(coff[3])  # three games: the small plan
    gs, go = ev.eval_vgroups(cpos[:few], coff[:4], N.GROUP_CHAIN)
    assert np.array_equal(gs, ops[:few]) and np.array_equal(go, opo[:few])
    ops, opo = oracle(on, spos)
    gs, go = ev.eval_vgroups(spos, soff, N.GROUP_STAR)
    assert np.array_equal(gs, ops) and np.array_equal(go, opo)


# ---- device builder against host builder ----

@pytest.fixture(scope="module")
def ctx():
    e = F.Evaluator(F.Net.from_bytes(net_bytes(7, 128, 0)), 0)  # the builder needs a ctx (device, stream) only
    yield e
    e.close()


def random_games():
    """200 random legal games from the start position, 20 to 120 plies asked for.  The seed was chosen on the
    CPU: 56 of them end by the third check."""
    return [(START, nnue.random_vgame(4000 + i, TC, START, 20 + (i * 37) % 101)) for i in range(200)]


def placed_games():
    """The two named games behind 0 and 13 to 16 shuffles (the checks on plies 57-62, 61-66, 65-70, 69-74: before,
    across and after the 64-move window), and the same from roots whose counters differ, cut where the host
    ends them."""
    games = []
    for tail in NAMED:
        for reps in (0, 13, 14, 15, 16):
            games.append((START, padded(reps, tail)))
            for w, b in ((1, 3), (2, 3), (3, 1), (3, 2), (1, 1)):
                fen = with_counters(w, b)
                games.append((fen, cut_at_end(fen, padded(reps, tail))))
    games.append((START + " +1+0", cut_at_end(START + " +1+0", padded(15, WHITE_THIRD))))
    games.append((with_counters(0, 2), ""))  # over at the root: the side to move has won
    return games


def host_fail_ply(fen, moves):
    mv = moves.split()
    for k in range(len(mv) + 1):
        try:
            nnue.game_vpositions(TC, fen, " ".join(mv[:k]))
        except F.FnnueError as e:
            assert e.name == "FNNUE_E_MOVE"
            return k
    return None


def test_games_are_what_they_should_be():
    rnd = random_games()
    ends = [nnue.game_end(f, m, TC) for f, m in rnd]
    assert sum(bool(e & F.END_VARIANT) for e in ends) >= 10
    assert all(e == LOST for e in ends if e & F.END_VARIANT)
    assert max(len(m.split()) for _, m in rnd) > 100
    placed = placed_games()
    assert all(nnue.game_end(f, m, TC) == LOST for f, m in placed[:-1])
    assert nnue.game_end(*placed[-1], TC) == F.END_NO_MOVES | F.END_VARIANT
    lens = sorted({len(m.split()) for f, m in placed if f == START})
    assert lens == [9, 10, 61, 62, 65, 66, 69, 70, 73, 74]
    # from a 2+3 root the first game ends on ply 7, from 1+3 on ply 5; black's counters move the second
    assert len(placed[2][1].split()) == 7 and len(placed[1][1].split()) == 5 and len(placed[3][1].split()) == 9
    assert len(cut_at_end(with_counters(3, 1), BLACK_THIRD).split()) == 6


def test_device_builder_plies_match_host_replay(ctx):
    legal = random_games() + placed_games()
    hpos = [nnue.game_vpositions(TC, f, m) for f, m in legal]
    hoff = np.concatenate([[0], np.cumsum([len(p) for p in hpos])])
    hpos = np.concatenate(hpos)
    for reps in (1, 1100 // len(legal) + 1):  # the two-wave replay; past 1024 games: one wave per game
        pos, off = ctx.build_vbatch(TC, legal * reps, N.PLAYOUT_PLIES)
        assert np.array_equal(off[:len(hoff)], hoff) and len(off) == reps * len(legal) + 1
        assert np.array_equal(pos, np.concatenate([hpos] * reps)), reps
    # one token after the end: the device fails at the host's ply
    over = [(f, m) for f, m in legal if nnue.game_end(f, m, TC) & F.END_VARIANT]
    assert len(over) >= 10 + 60
    illegal = [(f, (m + " " + SHUFFLE.split()[len(m.split()) % 2]).strip()) for f, m in over[:12] + over[-62:]]
    illegal.append((START, padded(16, "e2e4 e7e5 e1e3") + " " + WHITE_THIRD))  # an illegal move before any end
    for fen, moves in illegal:
        ply = host_fail_ply(fen, moves)
        assert ply is not None and (ply == len(moves.split()) or "e1e3" in moves)
        with pytest.raises(F.FnnueError) as e:
            ctx.build_vbatch(TC, [(fen, moves)])
        assert e.value.name == "FNNUE_E_MOVE" and f"ply {ply} of game 0" in str(e.value), (fen, moves, str(e.value))
    # a failing game inside a batch past 1024 games (the one-wave kernel) is named
    fen, moves = illegal[20]
    batch = legal[:40] * 27
    with pytest.raises(F.FnnueError) as e:
        ctx.build_vbatch(TC, batch[:1029] + [(fen, moves)] + batch[1029:])
    assert e.value.name == "FNNUE_E_MOVE" and f"ply {host_fail_ply(fen, moves)} of game 1029" in str(e.value)


def test_device_builder_fen_errors(ctx):
    for tail in ("2+3 0 1 +1+0", "4+3 0 1", "0 1 +0+4", "3+ 0 1", "0+0 0 1"):
        with pytest.raises(F.FnnueError) as e:
            ctx.build_vbatch(TC, [(START, "e2e4"), (START[:-3] + tail, "")])
        assert e.value.name == "FNNUE_E_FEN" and "game 1" in str(e.value), tail
    pos, off = ctx.build_vbatch(TC, [(START[:-3] + "3+3 0 1", "e2e4"), (START + " +0+0", "e2e4")])
    assert np.array_equal(pos[:2], pos[2:]) and np.array_equal(pos[:2], nnue.game_vpositions(TC, START, "e2e4"))


# ---- children and the one-ply search ----

CHILD_GAMES = [(START, nnue.random_vgame(4000 + i, TC, START, 20 + (i * 37) % 101)) for i in (0, 1, 2, 3)] + \
    [(START, WHITE_THIRD), (START, BLACK_THIRD), (START, padded(15, WHITE_THIRD)),
     (with_counters(2, 3), cut_at_end(with_counters(2, 3), padded(15, WHITE_THIRD))),
     (ROOTS[1], nnue.random_vgame(5, TC, ROOTS[1], 30)), (ROOTS[2], nnue.random_vgame(6, TC, ROOTS[2], 30)),
     (with_counters(0, 2), ""), (with_counters(2, 0), "")]


@pytest.fixture(scope="module")
def kids(nets):
    ev, _ = nets(256)
    pos, off, moves, end = ev.build_vchildren(TC, CHILD_GAMES)
    for a in (pos, off, moves, end):
        a.setflags(write=False)
    first, g0 = [], 0
    for _, m in CHILD_GAMES:
        first.append(g0)
        g0 += len(m.split()) + 1
    assert g0 == len(off) - 1
    return pos, off, moves, end, first


def test_children_records_offsets_moves_and_flags_equal_the_host(nets, ctx, kids):
    pos, off, moves, end, first = kids
    for e in (nets(256)[0], ctx):  # the plain children builder writes the same records
        p2, o2 = e.build_vbatch(TC, CHILD_GAMES, F.PLAYOUT_CHILDREN)
        assert np.array_equal(pos, p2) and np.array_equal(off, o2)
    replays, last_checks, finished = 0, 0, 0
    for (fen, mv), g0 in zip(CHILD_GAMES, first):
        hp, ho = F.game_vchildren(TC, fen, mv)
        n = len(ho) - 1
        assert np.array_equal(off[g0:g0 + n + 1] - off[g0], ho)
        assert np.array_equal(pos[off[g0]:off[g0 + n]], hp)
        ms = mv.split()
        for q in range(len(ms) + 1):
            o, e = int(off[g0 + q]), int(off[g0 + q + 1])
            prefix = ms[:q]
            assert moves[o] == 0 and end[o] == F.game_end(fen, prefix, TC), (fen, prefix)
            assert bool(end[o] & F.END_NO_MOVES) == (e - o == 1)
            if end[o] & F.END_VARIANT:  # a finished ply has no children
                assert e - o == 1 and q == len(ms)
                finished += 1
            texts = [F.vmove_uci(int(m)) for m in moves[o + 1:e]]
            assert len(set(texts)) == len(texts) and "" not in texts
            for x, t in zip(range(o + 1, e), texts):
                assert int(end[x]) == F.game_end(fen, prefix + [t], TC), (fen, prefix, t)  # never END_WON
                last_checks += int(end[x]) == LOST
                replays += 1
            if q < len(ms):
                assert ms[q] in texts
    assert replays > 1500 and last_checks >= 6 and finished >= 8  # each ended game's ply before has such a child


def test_search1_picks_the_last_check(nets, kids):
    ev, _ = nets(256)
    games = [(START, m.rsplit(" ", 1)[0]) for m in NAMED] + \
        [(START, padded(15, m).rsplit(" ", 1)[0]) for m in NAMED] + [(START, WHITE_THIRD), (with_counters(0, 2), "")]
    best, goff = ev.vsearch1(TC, games)
    _, goff2, lines = ev.vsearch1_lines(TC, games, 3)
    assert np.array_equal(goff, goff2)
    for g, m in enumerate(NAMED + NAMED):
        r = best[goff[g + 1] - 1]
        assert int(r["kind"]) == F.BEST_MATE and F.vmove_uci(int(r["move"])) == m.split()[-1] and int(r["end"]) == 0
        top = lines[goff[g + 1] - 1][0]
        assert int(top["kind"]) == F.BEST_MATE and F.vmove_uci(int(top["move"])) == m.split()[-1]
        assert int(top["child"]) == int(r["best"])
    for g in (4, 5):  # a finished ply: no children, its own flags
        r = best[goff[g + 1] - 1]
        assert int(r["kind"]) == F.BEST_NONE and int(r["nodes"]) == 0
        assert int(r["end"]) == (LOST if g == 4 else F.END_NO_MOVES | F.END_VARIANT)
    # the search is its three steps: the children of the fixture, the STAR evaluation, the reduction
    pos, off, moves, end, first = kids
    ps, po = ev.eval_vgroups(pos, off, N.GROUP_STAR)
    want = ev.best_children(ps, po, end, moves, off)
    got, _ = ev.vsearch1(TC, CHILD_GAMES)
    assert np.array_equal(got, want)
    assert (got["kind"] == F.BEST_MATE).sum() >= 4 and not (got["kind"] == F.BEST_LOST).any()


# ---- the actor ----

def body(tag, fen, moves, **kw):
    return B.AcquireResponseBody(tag, fen, moves, variant="threeCheck", **kw)


@pytest.fixture(scope="module")
def chans():
    """(depth 0, variant depth 1) channels over a chess net and a threeCheck net, and the net's oracle."""
    data = F.synthesize_variant_net(7, 256, AT)
    made = [B.channel(F.Net.from_bytes(net_bytes(1, 256, 0)), 0, threecheck=F.Net.from_bytes_variant(data, TC), **kw)
            for kw in ({}, {"variant_analysis_depth": 1})]
    yield made[0][0], made[1][0], VariantOracleNet(data, AT)
    for _, actor in made:
        actor.close()


def cp(ps, po, norm=361):
    v = int((int(ps) + int(po)) / 16)  # C truncation
    return int(v * 100 / norm)


def actor_bodies():
    bodies = [body(f"r{i}", START, nnue.random_vgame(4000 + i, TC, START, 20 + (i * 37) % 101)) for i in range(12)]
    bodies += [body("white", START, WHITE_THIRD), body("black", START, BLACK_THIRD),
               body("across", START, padded(14, WHITE_THIRD)), body("after", START, padded(16, BLACK_THIRD)),
               body("carry", with_counters(2, 3), cut_at_end(with_counters(2, 3), padded(15, WHITE_THIRD))),
               body("won", with_counters(0, 2), "")]
    return bodies


def test_actor_depth0_terms_and_ends(chans):
    d0, _, on = chans
    bodies = actor_bodies()
    res = d0.go(bodies + [body("after-end", START, WHITE_THIRD + " a7a6"), body("bad-fen", with_counters(0, 0), "")])
    assert isinstance(res[-2], B.PositionFailed) and res[-2].code == -8
    assert isinstance(res[-1], B.PositionFailed) and res[-1].code == -9
    ended = 0
    for b, rows in zip(bodies, res):
        assert not isinstance(rows, B.PositionFailed), (b.batch_id, rows)
        pos = F.game_vpositions(TC, b.position, b.moves)
        ps, po = oracle(on, pos)
        assert [r.position_id for r in rows] == list(range(len(ps)))
        assert [r.psqt for r in rows] == ps.tolist() and [r.positional for r in rows] == po.tolist()
        end = F.game_end(b.position, b.moves, TC)
        for k, r in enumerate(rows):
            if k == len(rows) - 1 and end & F.END_NO_MOVES:
                mated = bool(end & (F.END_CHECK | F.END_VARIANT))
                assert (r.score.kind, r.score.value, r.depth, r.nodes) == ("mate" if mated else "cp", 0, 0, 0)
                assert r.best_move is None
                ended += bool(end & F.END_VARIANT)
            else:
                assert (r.score.kind, r.score.value, r.depth, r.nodes) == ("cp", cp(ps[k], po[k]), 0, 1)
    assert ended >= 8
    comp = d0.go_compact(bodies)
    for f, c in zip(res, comp):
        assert [(r.position_id, r.score, r.psqt, r.positional, r.depth, r.nodes) for r in f] == \
            [(r.position_id, r.score, r.psqt, r.positional, r.depth, r.nodes) for r in c]


def test_actor_depth1_mates_with_the_last_check(chans):
    d0, d1, _ = chans
    bodies = actor_bodies()
    res, zero = d1.go(bodies), d0.go(bodies)
    mates = 0
    for b, rows, z in zip(bodies, res, zero):
        assert not isinstance(rows, B.PositionFailed), b.batch_id
        ms = b.moves.split()
        if F.game_end(b.position, b.moves, TC) & F.END_VARIANT and ms:
            last, before = rows[-1], rows[-2]
            assert (last.score, last.depth, last.nodes, last.best_move) == (B.Score("mate", 0), 0, 0, None)
            assert (last.psqt, last.positional) == (z[-1].psqt, z[-1].positional)
            assert before.score == B.Score("mate", 1) and before.depth == 1
            # the last check: the game's own move, or an earlier child that gives one too
            assert F.game_end(b.position, ms[:-1] + [before.best_move], TC) == LOST
            if b.batch_id in ("white", "black", "across", "after", "carry"):
                assert before.best_move == ms[-1]
            mates += 1
    assert mates >= 8
    won = res[-1]
    assert len(won) == 1 and (won[0].score, won[0].depth, won[0].best_move) == (B.Score("mate", 0), 0, None)
    # move work on the position before the last check, at either depth
    roots = [body("mv", START, WHITE_THIRD.rsplit(" ", 1)[0], work="move"), body("over", START, WHITE_THIRD, work="move")]
    for ch in (d0, d1):
        mv = [r[0] for r in ch.go(roots)]
        assert (mv[0].best_move, mv[0].score, mv[0].depth) == ("c4f7", B.Score("mate", 1), 1)
        assert (mv[1].best_move, mv[1].score, mv[1].depth, mv[1].nodes) == (None, B.Score("mate", 0), 0, 0)
    # MultiPV lines: the last check first
    lb = [body("l0", START, WHITE_THIRD, multipv=3), body("l1", START, padded(14, BLACK_THIRD), multipv=3)]
    for b, rows, plain in zip(lb, d1.go_lines(lb), d1.go(lb)):
        assert rows[-1].lines is None and len(rows[-2].lines) == 3
        top = rows[-2].lines[0]
        assert (top.score, top.move) == (B.Score("mate", 1), b.moves.split()[-1])
        assert [(r.score, r.best_move, r.psqt, r.positional) for r in rows] == \
            [(r.score, r.best_move, r.psqt, r.positional) for r in plain]
    assert all(r.lines is None for rows in d0.go_lines(lb) for r in rows)
    comp = d1.go_compact(bodies)
    for f, c in zip(res, comp):
        assert [(r.score, r.depth, r.psqt, r.positional) for r in f] == [(r.score, r.depth, r.psqt, r.positional) for r in c]


def test_routing():
    chess = F.Net.from_bytes(net_bytes(1, 256, 0))
    koth = F.Net.from_bytes_variant(F.synthesize_variant_net(7, 256, KOTH), KOTH)
    stub, actor = B.channel(chess, 0, kingofthehill=koth)  # no threeCheck net
    try:
        res = stub.go([body("tc", START, WHITE_THIRD),
                       B.AcquireResponseBody("anti", START, "e2e4", variant="antichess"),
                       B.AcquireResponseBody("horde", START, "e2e4", variant="horde"),
                       B.AcquireResponseBody("std", START, "e2e4")])
        assert [getattr(r, "code", 0) for r in res] == [-4, -4, -4, 0]
    finally:
        actor.close()
    # one net through fnnue_backend_channel goes to its own variant's slot
    tc = F.Net.from_bytes_variant(F.synthesize_variant_net(7, 256, AT), TC)
    stub, actor = B.channel(tc, 0)
    try:
        res = stub.go([body("tc", START, WHITE_THIRD), B.AcquireResponseBody("at", START, "e2e4", variant="atomic"),
                       B.AcquireResponseBody("anti", START, "e2e4", variant="antichess")])
        assert [getattr(r, "code", 0) for r in res] == [0, -4, -4]
        assert res[0][-1].score == B.Score("mate", 0)
    finally:
        actor.close()
    with pytest.raises(F.FnnueError) as e:
        B.channel(chess, 0, threecheck=chess)
    assert e.value.name == "FNNUE_E_ARG"
