"""The whole position domain on the GPU (tests/corpus.py): every reachable FT
row, every (perspective, king block, piece count) bin, every layer-stack
bucket, bare kings, and every delta shape of the grouped paths, bit-exact
against the CPU oracle over the whole corpus (no sampling); then about twenty
short legal endgames end to end (builder, CHAIN / STAR evaluation, the engine
actor at depth 0 and 1, fnnue_search1).  Run on an MI355X with -m gpu.

The host entry points apply the device's validity rule (one king per colour,
<= 32 pieces, valid codes, stm <= 1), so pawns on ranks 1 and 8 and 30 queens
of a colour pass through them as well as through the device entry points."""
import numpy as np
import pytest

import fishnet_amd as F
from fishnet_amd import _native as N
from fishnet_amd import backend as B
from oracle.oracle import OracleNet, VariantOracleNet
from tests import corpus as Cp
from tests.conftest import net_bytes
from tests.test_gpu_backend import check_rows
from tests.test_gpu_search1 import as_tuples, bodies_of, check_depth1, reduce_groups

pytestmark = pytest.mark.gpu

ZH, AT = N.VARIANT_CRAZYHOUSE, N.VARIANT_ATOMIC
HEAVY = (5, 512, N.SYNTH_HEAVY)  # slices 1 mod 3 run packed rows, the others SWAR: mixed kernels
NETS = [(1, 1024, 0), (7, 128, 0), (3, 1024, N.SYNTH_WRAP), (9, 2560, 0), (6, 2048, 0), HEAVY]
GROUP_NETS = [(1, 1024, 0), (7, 128, 0), (3, 1024, N.SYNTH_WRAP)]
MODES = (N.GROUP_CHAIN, N.GROUP_STAR)


@pytest.fixture(scope="module")
def corpus():
    pos = Cp.chess_corpus()
    pos.setflags(write=False)
    return pos


@pytest.fixture(scope="module")
def batches(corpus):
    """name -> (records, offsets): the grouped inputs, built once and never changed."""
    out = {"strip": Cp.strip_chains(), "fill": Cp.fill_chains(), "chains<=2048": Cp.chess_chains(2048),
           "chains>2048": Cp.chess_chains(2600), "sweep": Cp.sweep_groups(corpus)}
    assert len(out["chains<=2048"][0]) <= 2048 < len(out["chains>2048"][0])
    for pos, off in out.values():
        pos.setflags(write=False)
        off.setflags(write=False)
    return out


@pytest.fixture(scope="module")
def nets():
    """(seed, hd, flags) -> (evaluator, oracle net, oracle results by input name)."""
    cache = {}

    def get(seed, hd, flags):
        key = (seed, hd, flags)
        if key not in cache:
            data = net_bytes(seed, hd, flags)
            cache[key] = (F.Evaluator(F.Net.from_bytes(data), 0), OracleNet(data), {})
        return cache[key]

    yield get
    for ev, _, _ in cache.values():
        ev.close()


def oracle_on(entry, name, pos):
    """The oracle's results on a named input, computed once per net."""
    _, on, memo = entry
    if name not in memo:
        ps, po, rc = on.eval_packed(pos, threads=8)
        assert rc == 0
        ps.setflags(write=False)
        po.setflags(write=False)
        memo[name] = (ps, po)
    return memo[name]


def assert_equal(got, want, what):
    bad = np.nonzero((got[0] != want[0]) | (got[1] != want[1]))[0]
    assert len(bad) == 0, f"{what}: {len(bad)} of {len(want[0])} differ, first at {bad[:8].tolist()}: " \
                          f"gpu {got[0][bad[:3]]},{got[1][bad[:3]]} oracle {want[0][bad[:3]]},{want[1][bad[:3]]}"


def groups_device(ev, pos, off, mode, variant=False):
    import torch
    dev = torch.device("cuda", 0)
    d_pos = torch.from_numpy(np.array(pos)).to(dev)
    d_off = torch.from_numpy(np.array(off).view(np.int32)).to(dev)
    out = torch.full((2, len(pos)), 77, dtype=torch.int32, device=dev)
    torch.cuda.synchronize(dev)
    call = ev.eval_vgroups_device if variant else ev.eval_groups_device
    call(d_pos.data_ptr(), d_off.data_ptr(), len(off) - 1, len(pos), mode, out[0].data_ptr(), out[1].data_ptr(), None)
    ev.check()
    o = out.cpu().numpy()
    return o[0], o[1]


# ---- from scratch --------------------------------------------------------------------------------

@pytest.mark.parametrize("impl", [N.FT_SLICED, N.FT_GATHER, N.FT_AUTO])
@pytest.mark.parametrize("seed,hd,flags", NETS)
def test_corpus_from_scratch(nets, corpus, seed, hd, flags, impl):
    """eval_positions over the whole corpus == the oracle, for each feature-transformer choice,
    SWAR row sums on and off (a WRAP net has none to turn on), and the bucket-0 / bare-king
    answers are real evaluations."""
    entry = nets(seed, hd, flags)
    ev = entry[0]
    want = oracle_on(entry, "corpus", corpus)
    swar = ev.swar()[0]
    assert swar == (flags != N.SYNTH_WRAP)
    if (seed, hd, flags) == HEAVY:
        eligible, enabled, ns = ev.swar_slices()
        assert enabled == eligible and 0 < bin(enabled).count("1") < ns  # mixed SWAR / packed slices
    ev.set_ft_impl(impl)
    try:
        assert_equal(ev.eval_positions(corpus), want, "swar as created")
        if swar:
            ev.set_swar(False)
            try:
                assert_equal(ev.eval_positions(corpus), want, "swar off")
            finally:
                ev.set_swar(True)
    finally:
        ev.set_ft_impl(N.FT_AUTO)
    bucket0, bare = Cp.buckets(corpus) == 0, Cp.piece_counts(corpus) == 2
    assert bucket0.sum() >= 500 and bare.sum() >= 170
    assert np.unique(want[1][bucket0]).size > 100 and np.unique(want[1][bare]).size > 20
    assert np.count_nonzero(want[0][bucket0]) > 100  # PSQT of one to two extra pieces


def test_corpus_device_entry_point(nets, corpus):
    """The device-pointer entry point takes the same records (pawns on ranks 1 and 8, 30 queens)."""
    import torch
    entry = nets(1, 1024, 0)
    ev = entry[0]
    d = torch.from_numpy(np.array(corpus)).cuda()
    out = torch.full((2, len(corpus)), 77, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    ev.eval_positions_device(d.data_ptr(), len(corpus), out[0].data_ptr(), out[1].data_ptr(), None)
    ev.check()
    o = out.cpu().numpy()
    assert_equal((o[0], o[1]), oracle_on(entry, "corpus", corpus), "device entry")


def test_a_wrong_row_is_noticed(corpus):
    """What the corpus is for: three FT rows that 20000 random playouts never read are changed
    in the evaluator's net (the oracle keeps the original).  On the playouts nothing shows; on
    the corpus results differ, and only at positions that hold one of those rows, through every FT path."""
    seed, hd = 7, 128
    data = net_bytes(seed, hd, 0)
    playouts = F.random_playouts(1, 20000, threads=8)
    unread = np.nonzero(Cp.chess_coverage(corpus)["rows"] & ~Cp.chess_coverage(playouts)["rows"])[0]
    assert len(unread) > 5000
    rows = unread[[0, len(unread) // 2, -1]]
    bad = bytearray(data)
    o = 12 + int(np.frombuffer(data, np.uint32, 1, 8)[0]) + 4 + 2 * hd
    for r in rows:
        w = np.frombuffer(data, "<i2", hd, o + 2 * hd * int(r)).astype(np.int32)
        bad[o + 2 * hd * int(r):o + 2 * hd * (int(r) + 1)] = (w + 57).astype("<i2").tobytes()
    ev, on = F.Evaluator(F.Net.from_bytes(bytes(bad)), 0), OracleNet(data)
    try:
        ops, opo, rc = on.eval_packed(playouts, threads=8)
        assert rc == 0
        assert_equal(ev.eval_positions(playouts), (ops, opo), "playouts")  # the old inputs see nothing
        want = on.eval_packed(corpus, threads=8)
        holds = _holding(corpus, rows)
        assert holds.sum() >= 3
        for impl in (N.FT_SLICED, N.FT_GATHER):
            ev.set_ft_impl(impl)
            ps, po = ev.eval_positions(corpus)
            differ = (ps != want[0]) | (po != want[1])
            assert differ.any() and not differ[~holds].any(), impl
    finally:
        ev.close()


def _holding(records, rows):
    """Mask of the records with one of `rows` among either perspective's features (refpy)."""
    table = Cp._chess_index_table()
    boards, _ = Cp.unpack_boards(records)
    n, sq = np.nonzero(boards)
    pc = boards[n, sq]
    out = np.zeros(len(boards), dtype=bool)
    for persp, king in ((0, Cp.WK), (1, Cp.BK)):
        ksq = np.argmax(boards == king, axis=1)
        hit = np.isin(table[persp, ksq[n], pc, sq], rows)
        np.logical_or.at(out, n[hit], True)
    return out


def test_full_boards_near_the_swar_limit(corpus, batches):
    """The corpus's 32-piece boards (30 identical pieces) through a net whose accumulators come
    close to the doubled-column SWAR limit: SWAR == packed == oracle, from scratch and along
    the chains."""
    data = Cp.edge_net(21, 256, (400, 500))
    net = F.Net.from_bytes(data)
    assert 31 * 400 * 2 < net.accumulator_bound() < 32768
    ev, on = F.Evaluator(net, 0), OracleNet(data)
    try:
        assert ev.swar()[0]
        full = corpus[Cp.piece_counts(corpus) == 32]
        assert len(full) > 1000
        gpos, goff = batches["chains>2048"]
        ps, po, rc = on.eval_packed(full, threads=8)
        gps, gpo, grc = on.eval_packed(gpos, threads=8)
        assert rc == 0 and grc == 0
        for swar in (True, False):
            ev.set_swar(swar)
            assert_equal(ev.eval_positions(full), (ps, po), f"swar {swar}")
            for mode in MODES:
                assert_equal(ev.eval_groups(gpos, goff, mode), (gps, gpo), f"swar {swar} mode {mode}")
    finally:
        ev.close()


# ---- grouped -------------------------------------------------------------------------------------

@pytest.mark.parametrize("impl", [N.FT_SLICED, N.FT_GATHER])
@pytest.mark.parametrize("seed,hd,flags", GROUP_NETS)
def test_chains_and_sweep_groups(nets, batches, seed, hd, flags, impl):
    """Strip / fill / mixed chains (both plan sizes) and the sweep groups, CHAIN and STAR,
    through the host and the device entry point == from scratch == the oracle."""
    entry = nets(seed, hd, flags)
    ev = entry[0]
    for name, (pos, off) in batches.items():
        want = oracle_on(entry, name, pos)
        assert_equal(ev.eval_positions(pos), want, f"{name} from scratch")
        ev.set_ft_impl(impl)
        try:
            for mode in MODES:
                assert_equal(ev.eval_groups(pos, off, mode), want, f"{name} mode {mode} host")
                assert_equal(groups_device(ev, pos, off, mode), want, f"{name} mode {mode} device")
        finally:
            ev.set_ft_impl(N.FT_AUTO)


@pytest.mark.parametrize("seed,hd,flags", [(1, 1024, 0), (7, 128, 0)])
def test_chains_of_one_length(nets, seed, hd, flags):
    """Every chain of a call the same length: a pass's longest segment is that length, so the
    last batch of 8 deltas holds each count 1..8 in turn."""
    entry = nets(seed, hd, flags)
    ev = entry[0]
    for length in Cp.CHAIN_LENGTHS[1:]:
        pos, off = Cp.uniform_chains(length, 600)
        want = oracle_on(entry, f"uniform{length}", pos)
        for mode in MODES:
            assert_equal(ev.eval_groups(pos, off, mode), want, f"length {length} mode {mode}")


def test_chains_dual_net(nets, batches):
    """fnnue_eval_groups_dual_device with (1024, 128) on the chains: bucket 0, bare kings and
    the non-move delta shapes through the shared plan."""
    big, small = nets(1, 1024, 0), nets(7, 128, 0)
    for name in ("chains<=2048", "chains>2048", "strip", "fill"):
        pos, off = batches[name]
        wb, ws = oracle_on(big, name, pos), oracle_on(small, name, pos)
        for mode in MODES:
            ps, po, ps2, po2 = big[0].eval_groups_dual(small[0], np.array(pos), np.array(off), mode)
            assert_equal((ps, po), wb, f"{name} mode {mode} big")
            assert_equal((ps2, po2), ws, f"{name} mode {mode} small")


# ---- variants ------------------------------------------------------------------------------------

@pytest.mark.parametrize("hd", [256, 1024])
@pytest.mark.parametrize("variant", [ZH, AT])
def test_variant_corpus_and_chains(variant, hd):
    """eval_vpositions and eval_vgroups (CHAIN, STAR; host and device entry) over the variant
    corpus (every board row, every hand row and pocket count, 30 pieces in hand) and the
    chains (pockets changing with the board; exploded kings inside groups, answered (0, 0)),
    SWAR on and off, against the variant oracle."""
    data = F.synthesize_variant_net(5, hd, variant)
    ev, on = F.Evaluator(F.Net.from_bytes_variant(data, variant), 0), VariantOracleNet(data, variant)
    try:
        pos = Cp.variant_corpus(variant)
        inputs = [("corpus", pos, Cp.sweep_groups(pos)[1])]
        inputs += [(f"chains {cap}",) + Cp.variant_chains(variant, cap) for cap in (2048, 2600)]
        assert ev.swar()[0]
        for name, p, off in inputs:
            ps, po, rc = on.eval_packed(p, threads=8)
            assert rc == 0
            gone = Cp.one_king(p)
            assert gone.any() == (variant == AT and name != "corpus")
            assert not ps[gone].any() and not po[gone].any()
            for swar in (True, False):
                ev.set_swar(swar)
                assert_equal(ev.eval_vpositions(p), (ps, po), f"{name} swar {swar} from scratch")
                for mode in MODES:
                    assert_equal(ev.eval_vgroups(p, off, mode), (ps, po), f"{name} swar {swar} mode {mode}")
            ev.set_swar(True)
            for mode in MODES:
                assert_equal(groups_device(ev, p, off, mode, variant=True), (ps, po), f"{name} mode {mode} device")
    finally:
        ev.close()


# ---- end to end on sparse endgames ---------------------------------------------------------------

@pytest.fixture(scope="module")
def endgames():
    """The host builder's records of the written-out games (it checks their legality)."""
    plies = [F.game_positions(fen, mv) for fen, mv in Cp.ENDGAMES]
    kids = [F.game_children(fen, mv) for fen, mv in Cp.ENDGAMES]
    pos = np.concatenate(plies)
    cpos = np.concatenate([k[0] for k in kids])
    coff = Cp.offsets(np.concatenate([np.diff(k[1].astype(np.int64)) for k in kids]))
    for a in (pos, cpos, coff):
        a.setflags(write=False)
    assert (Cp.buckets(pos) == 0).all() and (Cp.buckets(cpos) == 0).all()
    assert (Cp.piece_counts(cpos) == 2).sum() >= 40  # children that are bare kings
    return pos, Cp.offsets([len(p) for p in plies]), cpos, coff


@pytest.mark.parametrize("seed,hd,flags", [(1, 1024, 0), (1, 256, 0)])
def test_endgames_builder_and_groups(nets, endgames, seed, hd, flags):
    pos, off, cpos, coff = endgames
    entry = nets(seed, hd, flags)
    ev = entry[0]
    bp, bo = ev.build_batch(Cp.ENDGAMES, F.PLAYOUT_PLIES)
    assert np.array_equal(bp, pos) and np.array_equal(bo, off)
    bp, bo = ev.build_batch(Cp.ENDGAMES, F.PLAYOUT_CHILDREN)
    assert np.array_equal(bp, cpos) and np.array_equal(bo, coff)
    assert_equal(ev.eval_groups(pos, off, N.GROUP_CHAIN), oracle_on(entry, "endgame plies", pos), "CHAIN")
    assert_equal(ev.eval_groups(cpos, coff, N.GROUP_STAR), oracle_on(entry, "endgame children", cpos), "STAR")
    assert_equal(ev.eval_positions(cpos), oracle_on(entry, "endgame children", cpos), "from scratch")


def test_endgames_search1_and_actor(nets, endgames):
    """fnnue_search1 on the endgames == the oracle's evaluation of the host builder's children
    reduced by test_gpu_search1's restatement; the actor at depth 0 (test_gpu_backend's
    check_rows) and at depth 1 (check_depth1 against search1).  Children here are bucket-0
    records, bare kings among them."""
    pos, off, cpos, coff = endgames
    entry = nets(1, 256, 0)
    ev = entry[0]
    kp, koff, moves, end = ev.build_children(Cp.ENDGAMES)
    assert np.array_equal(kp, cpos) and np.array_equal(koff, coff)
    hend = np.zeros(len(cpos), dtype=np.uint8)  # the host's end flags of every record
    g = 0
    for fen, mv in Cp.ENDGAMES:
        ms = mv.split()
        for q in range(len(ms) + 1):
            o, e = int(coff[g]), int(coff[g + 1])
            hend[o] = F.game_end(fen, ms[:q])
            for x in range(o + 1, e):
                hend[x] = F.game_end(fen, ms[:q] + [F.move_uci(int(moves[x]))])
            g += 1
    assert np.array_equal(end, hend)
    ops, opo = oracle_on(entry, "endgame children", cpos)
    want = reduce_groups(ops, opo, hend, moves, coff)
    best, goff = ev.search1(Cp.ENDGAMES)
    assert goff.tolist() == off.tolist()
    assert as_tuples(best) == want
    kinds = set(best["kind"].tolist())
    assert {F.BEST_NONE, F.BEST_CP, F.BEST_MATE} <= kinds  # ended games, evaluations, mates in one
    data = net_bytes(1, 256, 0)
    on = {0: entry[1]}
    made = [B.channel(F.Net.from_bytes(data), 0, **kw) for kw in ({"analysis_depth": 1}, {})]
    try:
        d1, d0 = made[0][0], made[1][0]
        bodies = bodies_of(Cp.ENDGAMES)
        res, zero = d1.go(bodies), d0.go(bodies)
        for i, (body, rows, zrows) in enumerate(zip(bodies, res, zero)):
            assert not isinstance(rows, B.PositionFailed) and not isinstance(zrows, B.PositionFailed), body.batch_id
            check_rows(on, body, zrows)
            check_depth1(rows, zrows, best[goff[i]:goff[i + 1]])
    finally:
        for _, actor in made:
            actor.close()
