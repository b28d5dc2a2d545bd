// vbuilder.hip — device batch builder for Fairy-Stockfish variants
// (crazyhouse, atomic, kingofthehill, racingkings, threecheck): the variant half of
// IncomingBatch::from_acquired
// ([ref] src/queue.rs:524-552 with body.variant != Standard, routed to the
// MultiVariant engine at :530-539; variants from src/assets.rs:384-391).
//
// As builder.hip for chess: one wave per game (replay_wave.h) parses the FEN
// (holdings, promoted marks) and replays the UCI moves (drops "P@e4",
// pockets, explosions) with the rules of vboard.h — the same source the host replay
// (fnnue_game_vpositions) runs, which the tests hold it to record for record —
// writing one fnnue_vpos per ply; CHILDREN adds one thread per ply for its
// legal children (drops included), and the one-ply search's form of it
// (fnnue_build_vchildren) one thread per record for the children with their
// move codes and game-end flags.
//
// kingofthehill, racingkings and threecheck play chess moves (no drops, no
// explosions), so they replay on the chess rule set's lane-parallel chain
// (chess_rules.h ChessRules::lane_chain) with their own legality and end of
// the game (PlainRules below), on DBoard boards; the host runs the same rules
// from vboard.h, and the tests hold the two to each other record for record.
// threecheck's counters ride on that chain too: lane j sees on its own
// snapshot whether move j gave check, and every ply's counters follow from one
// ballot (PlainRules::lane_chain).
#include <hip/hip_runtime.h>

#include <vector>

#include "builder.h"
#include "chess_rules.h"
#include "replay_wave.h"
#include "vboard.h"

namespace fnnue {

namespace {

__global__ void vcount_plies_kernel(const char* __restrict__ text, const uint32_t* __restrict__ fen_off,
                                    const uint32_t* __restrict__ mv_off, uint32_t ngames,
                                    uint32_t* __restrict__ plies) {
  const uint32_t g = blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= ngames) return;
  uint32_t p = mv_off[g], st, n = 1;
  const uint32_t end = fen_off[g + 1];
  while (vb::next_token(text, p, end, st) > 0) ++n;
  plies[g] = n;
}

// Variant rules of the wave replay (replay_wave.h), vboard.h's.
struct VariantRules {
  using Board = vb::VBoard;
  using Move = vb::VMove;
  using Pos = fnnue_vpos;
  // the board's non-square state: pockets, castling rooks (VBoard::cr bytes),
  // en passant, side to move, variant | c960 << 8
  struct Scalars {
    uint64_t pocket[2];
    uint32_t cr;
    int32_t ep;
    uint32_t stm;
    uint32_t vc;
  };
  // Along the chain the pockets, cr and ep change; stm alternates and the
  // variant word is fixed (the checking lanes derive those two).
  static constexpr int kVary = 6;
  static constexpr bool kLaneChain = false;  // drops and explosions: the sequential chain (replay::chain)
  struct Win {};
  __device__ static Win window(const Scalars&, uint32_t, uint32_t, int) { return Win{}; }
  __device__ static void advance(Scalars&, const Win&, uint32_t) {}
  __device__ static void fix(Scalars& s, const Scalars& s0, const Win&, uint32_t j, bool after) {
    s.stm = s0.stm ^ ((j + (after ? 1u : 0u)) & 1u);
    s.vc = s0.vc;
  }
  __device__ static Scalars scalars(const vb::VBoard& b) {
    Scalars s;
    s.pocket[0] = b.pocket[0];
    s.pocket[1] = b.pocket[1];
    uint32_t cr;
    __builtin_memcpy(&cr, b.cr, 4);
    s.cr = cr;
    s.ep = b.ep;
    s.stm = b.stm;
    s.vc = (uint32_t)b.variant | ((uint32_t)b.c960 << 8);
    return s;
  }
  __device__ static int sc_cr(uint32_t cr, int c, int side) {
    return (int)(int8_t)((cr >> (8 * (2 * c + side))) & 0xFFu);
  }
  __device__ static void sc_cr_set(uint32_t& cr, int c, int side, int v) {
    const int sh = 8 * (2 * c + side);
    cr = (cr & ~(0xFFu << sh)) | (((uint32_t)v & 0xFFu) << sh);
  }
  __device__ static int sc_hand(const Scalars& s, int c, int t) {
    return (int)(((c ? s.pocket[1] : s.pocket[0]) >> (8 * (t - 1))) & 255u);
  }
  __device__ static void sc_hand_add(Scalars& s, int c, int t, int d) {
    const uint64_t delta = (uint64_t)(int64_t)d << (8 * (t - 1));
    if (c) s.pocket[1] += delta;
    else s.pocket[0] += delta;
  }
  __device__ static bool parse_fen(const char* t, uint32_t p, uint32_t e, int variant, vb::VBoard& b) {
    return vb::parse_fen(t, p, e, variant, b);
  }
  __device__ static const char* start_fen(int variant) {
    return variant == vb::kCrazyhouse ? "rnbqkbnr/pppppppp/8/8/8/8/PPPPPPPP/RNBQKBNR[] w KQkq - 0 1"
                                      : "rnbqkbnr/pppppppp/8/8/8/8/PPPPPPPP/RNBQKBNR w KQkq - 0 1";
  }
  __device__ static uint32_t start_fen_len(int variant) { return variant == vb::kCrazyhouse ? 58 : 56; }
  __device__ static vb::VBoard start_board(int variant) {
    vb::VBoard b;
    b.bc[0] = 0x000000000000FFFFull;
    b.bc[1] = 0xFFFF000000000000ull;
    b.bt[0] = 0;
    b.bt[vb::PAWN] = 0x00FF00000000FF00ull;
    b.bt[vb::KNIGHT] = 0x4200000000000042ull;
    b.bt[vb::BISHOP] = 0x2400000000000024ull;
    b.bt[vb::ROOK] = 0x8100000000000081ull;
    b.bt[vb::QUEEN] = 0x0800000000000008ull;
    b.bt[vb::KING] = 0x1000000000000010ull;
    b.promoted = 0;
    b.pocket[0] = b.pocket[1] = 0;
    b.cr[0][0] = 7;
    b.cr[0][1] = 0;
    b.cr[1][0] = 63;
    b.cr[1][1] = 56;
    b.ep = -1;
    b.stm = 0;
    b.variant = (uint8_t)variant;
    b.c960 = 0;
    return b;
  }
  // vb::match_uci's token rules: drops "P@e4" (piece letter either case, no
  // king), moves "e2e4" / "e7e8q" (promotion letter either case, N B R Q)
  __device__ static uint32_t encode(const char* c, int len) {
    if (len == 4 && c[1] == '@') {
      const int pt = vb::piece_type_of(c[0]), to = replay::tok_sq(c[2], c[3]);
      if (!pt || pt == vb::KING || to < 0) return replay::kTokBad;
      return ((uint32_t)to << 6) | ((uint32_t)pt << 12) | replay::kTokDrop;
    }
    const int from = replay::tok_sq(c[0], c[1]), to = replay::tok_sq(c[2], c[3]);
    if (from < 0 || to < 0) return replay::kTokBad;
    int promo = 0;
    if (len == 5) {
      promo = vb::piece_type_of(c[4]);
      if (!promo || promo == vb::PAWN || promo == vb::KING) return replay::kTokBad;
    }
    return (uint32_t)from | ((uint32_t)to << 6) | ((uint32_t)promo << 12);
  }
  __device__ static bool interpret(const Scalars& b, uint32_t code, vb::VMove& m, uint32_t sqv) {
    const int to = (int)replay::tok_to(code), pc = (int)replay::tok_piece(code);
    if (code & replay::kTokDrop) {
      m = vb::VMove{-1, (int8_t)to, (int8_t)pc, 2};
      return true;
    }
    const int from = (int)replay::tok_from(code);
    const uint32_t own = replay::lane_value(sqv, from) & 15u;
    if (!own || (int)(own >> 3) != (int)b.stm) return false;
    m = vb::VMove{(int8_t)from, (int8_t)to, (int8_t)pc, 0};
    if ((own & 7u) == (uint32_t)vb::KING && !pc) {
      const int back = b.stm == 0 ? 0 : 56;
      const bool c960 = (b.vc >> 8) & 1;
#pragma unroll
      for (int side = 0; side < 2; ++side) {
        const int rsq = sc_cr(b.cr, b.stm, side);
        if (rsq >= 0 && (to == rsq || (!c960 && to == back + (side == 0 ? 6 : 2)))) {
          m = vb::VMove{(int8_t)from, (int8_t)rsq, 0, 1};
          return true;
        }
      }
    }
    return true;
  }
  // lane byte: piece code, bit 4 = promoted (crazyhouse)
  __device__ static uint32_t lane_square(const vb::VBoard& b, int sq) {
    return (uint32_t)vb::piece_at(b, sq) | ((uint32_t)((b.promoted >> sq) & 1) << 4);
  }
  // vb::do_move with lane l holding square l (see ChessRules::play): drops,
  // castling (the rook keeps its promoted mark), captures to the pocket (a
  // promoted piece as a pawn), atomic explosions as one select per lane.
  __device__ static void play(Scalars& b, const vb::VMove& m, uint32_t& sqv, int lane) {
    using vb::mkpc;
    constexpr int PAWN = vb::PAWN, ROOK = vb::ROOK, KING = vb::KING;
    const int us = b.stm;
    const int variant = (int)(b.vc & 255u);
    uint32_t v = sqv;
    int new_ep = -1;
    if (m.kind == 2) {
      v = lane == m.to ? (uint32_t)mkpc(us, m.piece) : v;
      sc_hand_add(b, us, m.piece, -1);
    } else if (m.kind == 1) {
      const int back = us == 0 ? 0 : 56;
      const bool king_side = m.to > m.from;
      const int kto = back + (king_side ? 6 : 2), rto = back + (king_side ? 5 : 3);
      const uint32_t rook_flag = replay::lane_value(v, m.to) & 16u;
      v = (lane == m.from || lane == m.to) ? 0u : v;
      v = lane == kto ? (uint32_t)mkpc(us, KING) : v;
      v = lane == rto ? ((uint32_t)mkpc(us, ROOK) | rook_flag) : v;
      sc_cr_set(b.cr, us, 0, -1);
      sc_cr_set(b.cr, us, 1, -1);
    } else {
      const uint32_t moved = replay::lane_value(v, m.from);
      const int pc = (int)(moved & 15u);
      int cap_sq = m.to;
      if ((pc & 7) == PAWN && m.to == b.ep && ((m.from ^ m.to) & 7) && !(replay::lane_value(v, m.to) & 15u))
        cap_sq = m.to + (us == 0 ? -8 : 8);
      const uint32_t capv = replay::lane_value(v, cap_sq);
      const int cap = (int)(capv & 15u);
      const bool zh = variant == vb::kCrazyhouse;
      if (cap && zh) {
        const int t = (capv & 16u) ? PAWN : (cap & 7);
        if (sc_hand(b, us, t) < 255) sc_hand_add(b, us, t, 1);
      }
      const uint32_t flag = (zh && (m.piece || (moved & 16u))) ? 16u : 0u;
      v = (lane == m.from || (cap && lane == cap_sq)) ? 0u : v;
      v = lane == m.to ? ((uint32_t)(m.piece ? mkpc(us, m.piece) : pc) | flag) : v;
      if (cap && variant == vb::kAtomic) {
        // the capturer explodes with its victim, and every non-pawn around
        const bool near = (vb::king_att(m.to) >> lane) & 1;
        v = (lane == m.to || (near && v != 0 && (v & 7u) != (uint32_t)PAWN)) ? 0u : v;
      }
      if ((pc & 7) == PAWN && (m.from ^ m.to) == 16) new_ep = (m.from + m.to) / 2;
      if ((pc & 7) == KING) {
        sc_cr_set(b.cr, us, 0, -1);
        sc_cr_set(b.cr, us, 1, -1);
      }
    }
    sqv = v;
    // castling rights end with the rook (moved, captured, exploded) or the king
    const uint64_t kings = __ballot((v & 7u) == (uint32_t)KING);
    const uint64_t black = __ballot((v & 15u) >= 8);
    for (int c = 0; c < 2; ++c) {
      if (!(kings & (c ? black : ~black))) {
        sc_cr_set(b.cr, c, 0, -1);
        sc_cr_set(b.cr, c, 1, -1);
      }
      for (int side = 0; side < 2; ++side) {
        const int r = sc_cr(b.cr, c, side);
        if (r >= 0 && (replay::lane_value(v, r) & 15u) != (uint32_t)mkpc(c, ROOK)) sc_cr_set(b.cr, c, side, -1);
      }
    }
    b.ep = new_ep;
    b.stm = (uint32_t)(us ^ 1);
  }
  // One chain step: interpret the code on the current board and play it;
  // false: it names no move of the side to move (the game's replay ends).
  __device__ __forceinline__ static bool step(Scalars& b, const Win&, uint32_t, uint32_t code, uint32_t& sqv, int lane,
                                              uint32_t& mv) {
    vb::VMove m;
    if (!interpret(b, code, m, sqv)) return false;
    play(b, m, sqv, lane);
    mv = pack_move(m);
    return true;
  }
  __device__ static uint32_t pack_move(const vb::VMove& m) {
    uint32_t w;
    __builtin_memcpy(&w, &m, 4);
    return w;
  }
  __device__ static vb::VMove unpack_move(uint32_t w) {
    vb::VMove m;
    __builtin_memcpy(&m, &w, 4);
    return m;
  }
  // A snapshot's bytes as bitboards (bit k of a code = plane k; bit 4 promoted).
  __device__ static vb::VBoard board_from(const uint32_t (&w)[16], const Scalars& sc) {
    const uint64_t p0 = replay::byte_plane(w, 0), p1 = replay::byte_plane(w, 1), p2 = replay::byte_plane(w, 2);
    const uint64_t p3 = replay::byte_plane(w, 3), p4 = replay::byte_plane(w, 4);
    const uint64_t occ = p0 | p1 | p2;
    vb::VBoard b;
    b.bc[0] = occ & ~p3;
    b.bc[1] = occ & p3;
    b.bt[0] = 0;
    b.bt[vb::PAWN] = p0 & ~p1 & ~p2;
    b.bt[vb::KNIGHT] = ~p0 & p1 & ~p2;
    b.bt[vb::BISHOP] = p0 & p1 & ~p2;
    b.bt[vb::ROOK] = ~p0 & ~p1 & p2;
    b.bt[vb::QUEEN] = p0 & ~p1 & p2;
    b.bt[vb::KING] = ~p0 & p1 & p2;
    b.promoted = p4;
    b.pocket[0] = sc.pocket[0];
    b.pocket[1] = sc.pocket[1];
    __builtin_memcpy(b.cr, &sc.cr, 4);
    b.ep = (int8_t)sc.ep;
    b.stm = (uint8_t)sc.stm;
    b.variant = (uint8_t)(sc.vc & 255u);
    b.c960 = (uint8_t)((sc.vc >> 8) & 255u);
    return b;
  }
  __device__ static fnnue_vpos pack_from(const uint32_t (&w)[16], const Scalars& sc) {
    uint32_t q[12];
    uint32_t nib[8];
    replay::pack_nibbles(w, nib);
#pragma unroll
    for (int i = 0; i < 8; ++i) q[i] = nib[i];
    // byte 32 stm, bytes 33..42 the pockets (white P N B R Q, black P N B R Q)
    const uint64_t wp = sc.pocket[0], bp = sc.pocket[1];
    q[8] = sc.stm | ((uint32_t)(wp & 0xFFFFFFu) << 8);
    q[9] = (uint32_t)((wp >> 24) & 0xFFFFu) | ((uint32_t)(bp & 0xFFFFu) << 16);
    q[10] = (uint32_t)((bp >> 16) & 0xFFFFFFu);
    q[11] = 0;
    fnnue_vpos p;
    memcpy(&p, q, sizeof(p));
    return p;
  }
  // As for chess (builder.hip ChessRules::verify): the token is accepted iff
  // the move interpret() built from it is legal.
  __device__ static bool verify(const vb::VBoard& b, const vb::VMove& m) {
    if (!vb::pseudo_member(b, m)) return false;
    vb::VBoard c = b;
    vb::do_move(c, m);
    return vb::legal_after(b, c);
  }
  __device__ static fnnue_vpos pack(const vb::VBoard& b) { return vb::pack(b); }
  __device__ static bool any_legal_from(const vb::VBoard& b, int sq, bool drops) {
    const bool own = (vb::colour(b, b.stm) >> sq) & 1;
    if (!own && !drops) return false;
    bool any = false;
    const vb::VBoard c = b;  // a copy for the by-reference generator: the chain's board stays in registers
    vb::for_each_legal(c, [&](const vb::VMove&) -> bool {
      any = true;
      return false;
    }, own ? 1ull << sq : 0ull, own, drops);
    return any;
  }
  __device__ static uint8_t end_flags(const vb::VBoard& b, bool any) { return vb::end_flags(b, any); }
};

// kingofthehill / racingkings / threecheck (V): the chess rule set with
//  * fnnue_vpos records (the chess record, empty pockets),
//  * vboard.h's FEN acceptance for them (racingkings: no pawns, no castling
//    rights; threecheck: the check counters) and match_uci's token rules
//    (promotion letters in either case),
//  * the variant's legality: nothing is legal in a finished position, and no
//    racingkings move gives check,
//  * the variant's game-end flags.
// Scalars, Win, window, advance and (but for threecheck) lane_chain, fix and
// board_from are ChessRules'.
//
// threecheck's counters (DBoard::bt[0], vboard.h checks_word) travel along the
// replay in the scalars' c960 word, above its bit 0: c960 | counters << 8.
// That word becomes the third the chain collects per lane (kVary = 3), so
// check() hands every lane the counters before and after its move like the
// en-passant square; board_from splits it into DBoard::c960 and bt[0].
//
// The counters of a window's 64 plies need no serial pass.  After the chess
// chain has written the window's snapshots, lane j turns its own (the board
// after move j) into bitboards and asks whether the mover attacks the other
// king: one ballot.  Colours alternate, so colour c's moves are the lanes of
// one parity, and its counter after move j is the value carried into the
// window minus the popcount of the ballot over that parity's lanes up to j,
// never below 0 (vb::checks_spend).  The chain is exact up to the window's
// first illegal move (ChessRules::lane_chain), and lane j's count reads
// lanes <= j only: every ply up to the first failing one has the host's
// counters, so the first ply that finds a counter at 0 before it (verify:
// plain_over) is the host's, and nothing after a failing ply is used.
template <int V>
struct PlainRules : ChessRules {
  using Pos = fnnue_vpos;
  static constexpr bool kCounts = V == kVariantThreeCheck;
  static constexpr int kVary = kCounts ? 3 : ChessRules::kVary;
  __device__ static Scalars scalars(const DBoard& b) {
    Scalars s = ChessRules::scalars(b);
    if constexpr (kCounts) s.c960 |= (uint32_t)b.bt[0] << 8;
    return s;
  }
  __device__ static DBoard board_from(const uint32_t (&w)[16], const Scalars& sc) {
    DBoard b = ChessRules::board_from(w, sc);
    if constexpr (kCounts) {
      b.c960 = sc.c960 & 1u;
      b.bt[0] = sc.c960 >> 8;
    }
    return b;
  }
  __device__ static void fix(Scalars& s, const Scalars& s0, const Win& w, uint32_t j, bool after) {
    const uint32_t word = s.c960;  // threecheck: this ply's own, collected along the chain
    ChessRules::fix(s, s0, w, j, after);
    if constexpr (kCounts) s.c960 = word;
  }
  __device__ static uint32_t lane_chain(Scalars& sc, uint32_t& sqv, uint32_t myc, uint32_t k, const Win& w,
                                        uint32_t (*SNAP)[16], int lane, uint32_t& mvw, uint32_t (&scw)[kVary]) {
    if constexpr (!kCounts) {
      return ChessRules::lane_chain(sc, sqv, myc, k, w, SNAP, lane, mvw, scw);
    } else {
      const uint32_t word = sc.c960, stm0 = sc.stm;
      sc.c960 = word & 1u;
      uint32_t epw[ChessRules::kVary];
      const uint32_t kplay = ChessRules::lane_chain(sc, sqv, myc, k, w, SNAP, lane, mvw, epw);
      // did move j give check?  the board after it, from lane j's own snapshot
      bool gives = false;
      if ((uint32_t)lane < kplay) {
        uint32_t wa[16];
#pragma unroll
        for (int i = 0; i < 16; ++i) wa[i] = SNAP[lane + 1][i];
        const DBoard a = ChessRules::board_from(wa, sc);  // the squares; the scalars are not read
        const int mover = (int)(stm0 ^ ((uint32_t)lane & 1u)), kt = king_sq(a, mover ^ 1);
        gives = kt >= 0 && attacked(a, kt, mover, a.bc[0] | a.bc[1]);
      }
      const uint64_t g = __ballot(gives);
      const uint64_t upto = lane == 63 ? ~0ull : (2ull << lane) - 1;  // moves 0..j
      const uint64_t white = stm0 == WHITE ? 0x5555555555555555ull : 0xAAAAAAAAAAAAAAAAull;  // white's moves
      const int w0 = (int)((word >> 8) & 0xFFu), b0 = (int)((word >> 16) & 0xFFu);
      const int wl = max(w0 - __popcll(g & white & upto), 0), bl = max(b0 - __popcll(g & ~white & upto), 0);
      const uint32_t mine = (word & 1u) | (uint32_t)wl << 8 | (uint32_t)bl << 16;
      scw[0] = epw[0];
      scw[1] = 0;  // the side to move: fix() derives it
      scw[2] = mine;
      sc.c960 = kplay ? replay::lane_value(mine, (int)kplay - 1) : word;
      return kplay;
    }
  }
  __device__ static fnnue_vpos widen(const fnnue_pos& p) {
    uint32_t q[12];
    memcpy(q, &p, sizeof(p));
    q[9] = q[10] = q[11] = 0;
    fnnue_vpos v;
    memcpy(&v, q, sizeof(v));
    return v;
  }
  __device__ static fnnue_vpos pack(const DBoard& b) { return widen(fnnue::pack(b)); }
  __device__ static fnnue_vpos pack_from(const uint32_t (&w)[16], const Scalars& sc) {
    return widen(ChessRules::pack_from(w, sc));
  }
  __device__ static const char* start_fen(int) {
    return V == kVariantRacingKings ? "8/8/8/8/8/8/krbnNBRK/qrbnNBRQ w - - 0 1" : ChessRules::start_fen(0);
  }
  __device__ static uint32_t start_fen_len(int) { return V == kVariantRacingKings ? 39 : 56; }
  __device__ static DBoard start_board(int) {
    if constexpr (V == kVariantThreeCheck) {
      DBoard b = ChessRules::start_board(0);
      b.bt[0] = vb::checks_word(3, 3);
      return b;
    }
    if constexpr (V != kVariantRacingKings) return ChessRules::start_board(0);
    DBoard b;
    b.bc[WHITE] = 0xF0F0ull;
    b.bc[BLACK] = 0x0F0Full;
    b.bt[0] = b.bt[PAWN] = 0;
    b.bt[KNIGHT] = 0x1818ull;
    b.bt[BISHOP] = 0x2424ull;
    b.bt[ROOK] = 0x4242ull;
    b.bt[QUEEN] = 0x0081ull;
    b.bt[KING] = 0x8100ull;
    b.cr = 0xFFFFFFFFu;
    b.ep = -1;
    b.stm = WHITE;
    b.c960 = 0;
    return b;
  }
  __device__ static bool parse_fen(const char* t, uint32_t p, uint32_t e, int, DBoard& b) {
    if (!fnnue::parse_fen(t, p, e, b)) return false;
    if (V == kVariantRacingKings && (b.bt[PAWN] || b.cr != 0xFFFFFFFFu)) return false;
    // vboard.h takes an en-passant square only while it is empty
    if (b.ep >= 0 && (((b.bc[0] | b.bc[1]) >> b.ep) & 1)) b.ep = -1;
    if constexpr (kCounts) {  // the fields after the en-passant square
      uint32_t st;
      for (int i = 0; i < 4; ++i) vb::next_token(t, p, e, st);
      if (!vb::parse_checks(t, p, e, b.bt[0])) return false;
    }
    return true;
  }
  __device__ static uint32_t encode(const char* c, int len) {
    const int from = replay::tok_sq(c[0], c[1]), to = replay::tok_sq(c[2], c[3]);
    if (from < 0 || to < 0) return replay::kTokBad;
    int promo = 0;
    if (len == 5) {
      promo = vb::piece_type_of(c[4]);
      if (!promo || promo == vb::PAWN || promo == vb::KING) return replay::kTokBad;
    }
    return (uint32_t)from | ((uint32_t)to << 6) | ((uint32_t)promo << 12);
  }
  __device__ static bool verify(const DBoard& b, const DMove& m) {
    return !plain_over<V>(b) && pseudo_member(b, m) && legal<V>(b, m);
  }
  __device__ static bool any_legal_from(const DBoard& b, int sq, bool) {
    if (!((colour(b, b.stm) >> sq) & 1)) return false;
    bool any = false;
    const DBoard c = b;  // a copy for the by-reference generator: the chain's board stays in registers
    for_each_legal<V>(c, [&](const DMove&) -> bool {
      any = true;
      return false;
    }, 1ull << sq);
    return any;
  }
  // vb::end_flags: decided by the variant's rule unless both racingkings kings are home (a draw)
  __device__ static uint8_t end_flags(const DBoard& b, bool any) {
    const uint64_t home = b.bt[KING] & 0xFF00000000000000ull;
    const bool draw = V == kVariantRacingKings && (home & b.bc[0]) && (home & b.bc[1]);
    return (uint8_t)(ChessRules::end_flags(b, any) | (plain_over<V>(b) && !draw ? kFinalVariant : 0));
  }
};

// CHILDREN of the plain variants, one thread per ply, in vb::for_each_legal's
// order (own pieces by square; a pawn's push, double push, captures, en
// passant; castling king side, queen side: chess_rules.h for_each_legal).
template <int V>
__global__ void pcount_children_kernel(const DBoard* __restrict__ states, uint32_t n, uint32_t* __restrict__ cnt) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const DBoard b = states[i];
  uint32_t c = 0;
  for_each_legal<V>(b, [&](const DMove&) -> bool {
    ++c;
    return true;
  });
  cnt[i] = 1u + c;
}

template <int V>
__global__ void pwrite_children_kernel(const DBoard* __restrict__ states, uint32_t n, const uint32_t* __restrict__ off,
                                       fnnue_vpos* __restrict__ out) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const DBoard b = states[i];
  uint32_t o = off[i];
  out[o++] = PlainRules<V>::pack(b);
  for_each_legal<V>(b, [&](const DMove& m) -> bool {
    DBoard c = b;
    do_move(c, m);
    out[o++] = PlainRules<V>::pack(c);
    return true;
  });
}

__global__ void vcount_children_kernel(const vb::VBoard* __restrict__ states, uint32_t n, uint32_t* __restrict__ cnt) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const vb::VBoard b = states[i];
  uint32_t c = 0;
  vb::for_each_legal(b, [&](const vb::VMove&) -> bool {
    ++c;
    return true;
  });
  cnt[i] = 1u + c;
}

__global__ void vwrite_children_kernel(const vb::VBoard* __restrict__ states, uint32_t n,
                                       const uint32_t* __restrict__ off, fnnue_vpos* __restrict__ out) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const vb::VBoard b = states[i];
  uint32_t o = off[i];
  out[o++] = vb::pack(b);
  vb::for_each_legal(b, [&](const vb::VMove& m) -> bool {
    vb::VBoard c = b;
    vb::do_move(c, m);
    out[o++] = vb::pack(c);
    return true;
  });
}

// ---- the one-ply search's children: records, moves, end flags ----
// As builder.hip's write_children_record_kernel: one thread per record, each
// regenerating its ply's moves up to its own (a crazyhouse ply with full
// pockets has several hundred children: one thread per ply would leave a piece
// of a few thousand plies on a handful of waves).

// fnnue_vmove_uci's codes: vb::move_code for the VBoard variants; the plain
// variants' castling carries the king's two-square step unless the game needs
// Chess960 notation.
__device__ __forceinline__ uint16_t pmove_code(const DBoard& b, const DMove& m) {
  int to = m.to;
  if (m.castle && !b.c960) to = (m.from & 56) + (m.to > m.from ? 6 : 2);
  return (uint16_t)((uint32_t)m.from | (uint32_t)to << 6 | (uint32_t)m.promo << 12);
}

// Record r's ply: off[lo] <= r < off[lo + 1] (off[0] = 0, off[n] = total > r).
__device__ __forceinline__ uint32_t ply_of_record(const uint32_t* __restrict__ off, uint32_t n, uint32_t r) {
  uint32_t lo = 0, hi = n;
  while (hi - lo > 1) {
    const uint32_t mid = (lo + hi) >> 1;
    if (off[mid] <= r) lo = mid;
    else hi = mid;
  }
  return lo;
}

__global__ __launch_bounds__(64) void vwrite_children_record_kernel(
    const vb::VBoard* __restrict__ states, uint32_t n, const uint32_t* __restrict__ off, uint32_t total,
    fnnue_vpos* __restrict__ out, uint16_t* __restrict__ moves, uint8_t* __restrict__ end) {
  const uint32_t r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= total) return;
  const uint32_t lo = ply_of_record(off, n, r);
  const uint32_t o0 = off[lo], j = r - o0;
  const vb::VBoard b = states[lo];
  vb::VBoard c = b;
  uint16_t mv = 0;
  if (j) {
    uint32_t k = 0;
    vb::for_each_legal(b, [&](const vb::VMove& m) -> bool {
      if (++k < j) return true;
      vb::do_move(c, m);
      mv = vb::move_code(b, m);
      return false;
    });
  }
  out[r] = vb::pack(c);
  moves[r] = mv;
  uint8_t f;
  if (j) {
    // the child's own flags: a second ply of generation that stops at the first
    // legal move; a child its side to move has already won loses for the mover
    const vb::VBoard d = c;  // a copy for the by-reference generator
    f = vb::final_state(d);
    if (vb::variant_over(d) && vb::variant_won(d)) f |= kFinalWon;
  } else {
    f = vb::end_flags(b, off[lo + 1] - o0 > 1);
  }
  end[r] = f;
}

template <int V>
__global__ __launch_bounds__(64) void pwrite_children_record_kernel(
    const DBoard* __restrict__ states, uint32_t n, const uint32_t* __restrict__ off, uint32_t total,
    fnnue_vpos* __restrict__ out, uint16_t* __restrict__ moves, uint8_t* __restrict__ end) {
  const uint32_t r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= total) return;
  const uint32_t lo = ply_of_record(off, n, r);
  const uint32_t o0 = off[lo], j = r - o0;
  const DBoard b = states[lo];
  DBoard c = b;
  uint16_t mv = 0;
  if (j) {
    uint32_t k = 0;
    for_each_legal<V>(b, [&](const DMove& m) -> bool {
      if (++k < j) return true;
      do_move_v<V>(c, m);  // threecheck: with the counters, which the child's flags read
      mv = pmove_code(b, m);
      return false;
    });
  }
  out[r] = PlainRules<V>::pack(c);
  moves[r] = mv;
  uint8_t f;
  if (j) {
    bool any = false;
    const DBoard d = c;  // a copy for the generator's reference
    for_each_legal<V>(d, [&](const DMove&) -> bool {
      any = true;
      return false;
    });
    f = PlainRules<V>::end_flags(c, any);
    if constexpr (V == kVariantRacingKings) {  // vb::variant_won
      const uint64_t goal = c.bt[KING] & 0xFF00000000000000ull;
      if (plain_over<V>(c) && (goal & colour(c, c.stm)) && !(goal & colour(c, c.stm ^ 1))) f |= kFinalWon;
    }
  } else {
    f = PlainRules<V>::end_flags(b, off[lo + 1] - o0 > 1);
  }
  end[r] = f;
}

// ---- the variant two-ply search's child states ----
// As builder.hip's child_states_kernel: one thread per record of the plies' STAR
// groups finds its ply and its move; the child's board is stored as it is (not
// packed), the ply's own record is skipped, so child j of ply i is entry
// off[i] - i + j - 1 of a dense array that vchildren_count_device and
// vchildren_write_device expand like any array of boards.  A threecheck child
// carries its counters (do_move_v), which its own children's flags read.
// map (optional): entry d -> (ply, 1-based child index).
__global__ __launch_bounds__(64) void vchild_states_kernel(const vb::VBoard* __restrict__ states, uint32_t n,
                                                           const uint32_t* __restrict__ off, uint32_t total,
                                                           vb::VBoard* __restrict__ out, uint2* __restrict__ map) {
  const uint32_t r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= total) return;
  const uint32_t lo = ply_of_record(off, n, r);
  const uint32_t j = r - off[lo];
  if (j == 0) return;
  const vb::VBoard b = states[lo];
  vb::VBoard c = b;
  uint32_t k = 0;
  vb::for_each_legal(b, [&](const vb::VMove& m) -> bool {
    if (++k < j) return true;
    vb::do_move(c, m);
    return false;
  });
  const uint32_t d = r - lo - 1;
  out[d] = c;
  if (map) map[d] = make_uint2(lo, j);
}

template <int V>
__global__ __launch_bounds__(64) void pchild_states_kernel(const DBoard* __restrict__ states, uint32_t n,
                                                           const uint32_t* __restrict__ off, uint32_t total,
                                                           DBoard* __restrict__ out, uint2* __restrict__ map) {
  const uint32_t r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= total) return;
  const uint32_t lo = ply_of_record(off, n, r);
  const uint32_t j = r - off[lo];
  if (j == 0) return;
  const DBoard b = states[lo];
  DBoard c = b;
  uint32_t k = 0;
  for_each_legal<V>(b, [&](const DMove& m) -> bool {
    if (++k < j) return true;
    do_move_v<V>(c, m);
    return false;
  });
  const uint32_t d = r - lo - 1;
  out[d] = c;
  if (map) map[d] = make_uint2(lo, j);
}

}  // namespace

hipError_t vchild_states_device(int variant, const void* d_states, uint32_t n, const uint32_t* d_off, uint32_t total,
                                void* d_out, uint2* d_map, hipStream_t s) {
  if (n == 0 || total == 0) return hipSuccess;
  const uint32_t bs = 64;
  const dim3 grid((total + bs - 1) / bs);
  if (variant == kVariantKingOfTheHill)
    hipLaunchKernelGGL(pchild_states_kernel<kVariantKingOfTheHill>, grid, dim3(bs), 0, s,
                       static_cast<const DBoard*>(d_states), n, d_off, total, static_cast<DBoard*>(d_out), d_map);
  else if (variant == kVariantRacingKings)
    hipLaunchKernelGGL(pchild_states_kernel<kVariantRacingKings>, grid, dim3(bs), 0, s,
                       static_cast<const DBoard*>(d_states), n, d_off, total, static_cast<DBoard*>(d_out), d_map);
  else if (variant == kVariantThreeCheck)
    hipLaunchKernelGGL(pchild_states_kernel<kVariantThreeCheck>, grid, dim3(bs), 0, s,
                       static_cast<const DBoard*>(d_states), n, d_off, total, static_cast<DBoard*>(d_out), d_map);
  else
    hipLaunchKernelGGL(vchild_states_kernel, grid, dim3(bs), 0, s, static_cast<const vb::VBoard*>(d_states), n, d_off,
                       total, static_cast<vb::VBoard*>(d_out), d_map);
  return hipGetLastError();
}

hipError_t vchildren_count_device(int variant, const void* d_states, uint32_t n, uint32_t* d_cnt, uint32_t* d_off,
                                  hipStream_t s, BuilderScratch& ws) {
  hipError_t e;
  if ((e = hipMemsetAsync(d_cnt + n, 0, 4, s)) != hipSuccess) return e;
  if (n) {
    const uint32_t bs = 64;
    const dim3 grid((n + bs - 1) / bs);
    if (variant == kVariantKingOfTheHill)
      hipLaunchKernelGGL(pcount_children_kernel<kVariantKingOfTheHill>, grid, dim3(bs), 0, s,
                         static_cast<const DBoard*>(d_states), n, d_cnt);
    else if (variant == kVariantRacingKings)
      hipLaunchKernelGGL(pcount_children_kernel<kVariantRacingKings>, grid, dim3(bs), 0, s,
                         static_cast<const DBoard*>(d_states), n, d_cnt);
    else if (variant == kVariantThreeCheck)
      hipLaunchKernelGGL(pcount_children_kernel<kVariantThreeCheck>, grid, dim3(bs), 0, s,
                         static_cast<const DBoard*>(d_states), n, d_cnt);
    else
      hipLaunchKernelGGL(vcount_children_kernel, grid, dim3(bs), 0, s, static_cast<const vb::VBoard*>(d_states), n,
                         d_cnt);
    if ((e = hipGetLastError()) != hipSuccess) return e;
  }
  return builder_exclusive_scan(d_cnt, d_off, n, s, ws);
}

hipError_t vchildren_write_device(int variant, const void* d_states, uint32_t n, const uint32_t* d_off, uint32_t total,
                                  fnnue_vpos* d_out, uint16_t* d_moves, uint8_t* d_end, hipStream_t s) {
  if (n == 0 || total == 0) return hipSuccess;
  const uint32_t bs = 64;
  const dim3 grid((total + bs - 1) / bs);
  if (variant == kVariantKingOfTheHill)
    hipLaunchKernelGGL(pwrite_children_record_kernel<kVariantKingOfTheHill>, grid, dim3(bs), 0, s,
                       static_cast<const DBoard*>(d_states), n, d_off, total, d_out, d_moves, d_end);
  else if (variant == kVariantRacingKings)
    hipLaunchKernelGGL(pwrite_children_record_kernel<kVariantRacingKings>, grid, dim3(bs), 0, s,
                       static_cast<const DBoard*>(d_states), n, d_off, total, d_out, d_moves, d_end);
  else if (variant == kVariantThreeCheck)
    hipLaunchKernelGGL(pwrite_children_record_kernel<kVariantThreeCheck>, grid, dim3(bs), 0, s,
                       static_cast<const DBoard*>(d_states), n, d_off, total, d_out, d_moves, d_end);
  else
    hipLaunchKernelGGL(vwrite_children_record_kernel, grid, dim3(bs), 0, s, static_cast<const vb::VBoard*>(d_states),
                       n, d_off, total, d_out, d_moves, d_end);
  return hipGetLastError();
}

// The variants that replay on DBoard boards (PlainRules).
static bool plain_variant(int variant) {
  return variant == kVariantKingOfTheHill || variant == kVariantRacingKings || variant == kVariantThreeCheck;
}

size_t vstate_bytes(int variant) { return plain_variant(variant) ? sizeof(DBoard) : sizeof(vb::VBoard); }

hipError_t replay_vgames_device(int variant, const char* d_text, const uint32_t* d_fen_off, const uint32_t* d_mv_off,
                                const uint32_t* d_ply_off, uint32_t ngames, fnnue_vpos* d_out, void* d_states,
                                uint8_t* d_final, uint32_t* d_err, hipStream_t s) {
  // d_states: DBoard for kingofthehill / racingkings / threecheck, vb::VBoard otherwise
  if (variant == kVariantKingOfTheHill)
    return replay::launch_replay<PlainRules<kVariantKingOfTheHill>>(variant, d_text, d_fen_off, d_mv_off, ngames,
                                                                    d_ply_off, d_out, static_cast<DBoard*>(d_states),
                                                                    d_err, d_final, s);
  if (variant == kVariantRacingKings)
    return replay::launch_replay<PlainRules<kVariantRacingKings>>(variant, d_text, d_fen_off, d_mv_off, ngames,
                                                                  d_ply_off, d_out, static_cast<DBoard*>(d_states),
                                                                  d_err, d_final, s);
  if (variant == kVariantThreeCheck)
    return replay::launch_replay<PlainRules<kVariantThreeCheck>>(variant, d_text, d_fen_off, d_mv_off, ngames,
                                                                 d_ply_off, d_out, static_cast<DBoard*>(d_states),
                                                                 d_err, d_final, s);
  return replay::launch_replay<VariantRules>(variant, d_text, d_fen_off, d_mv_off, ngames, d_ply_off, d_out,
                                             static_cast<vb::VBoard*>(d_states), d_err, d_final, s);
}

BuildResult build_vbatch_device(int variant, const char* d_text, const uint32_t* d_fen_off, const uint32_t* d_mv_off,
                                uint32_t ngames, bool children, fnnue_vpos* d_out, size_t cap, uint32_t* d_group_off,
                                size_t off_cap, hipStream_t s, BuilderScratch& ws, uint8_t* d_final, uint16_t* d_moves,
                                uint8_t* d_end, VChildrenBufs* own) {
  BuildResult R;
  auto fail = [&](hipError_t e) {
    R.hip = e;
    return R;
  };
  hipError_t e;
  uint32_t *plies = nullptr, *ply_off = nullptr, *err = nullptr, *cnt = nullptr, *coff = nullptr;
  void* states = nullptr;
  const size_t state_bytes = vstate_bytes(variant);
  using W = BuilderScratch;
  if ((e = ws.get(W::kPlies, (size_t)(ngames + 1) * 4, (void**)&plies)) != hipSuccess) return fail(e);
  if ((e = ws.get(W::kPlyOff, (size_t)(ngames + 1) * 4, (void**)&ply_off)) != hipSuccess) return fail(e);
  if ((e = ws.get(W::kErr, 16, (void**)&err)) != hipSuccess) return fail(e);
  if ((e = hipMemsetAsync(err, 0, 16, s)) != hipSuccess) return fail(e);
  if ((e = hipMemsetAsync(plies + ngames, 0, 4, s)) != hipSuccess) return fail(e);
  const uint32_t bs = 64;
  hipLaunchKernelGGL(vcount_plies_kernel, dim3((ngames + bs - 1) / bs), dim3(bs), 0, s, d_text, d_fen_off, d_mv_off,
                     ngames, plies);
  if ((e = hipGetLastError()) != hipSuccess) return fail(e);
  if ((e = builder_exclusive_scan(plies, ply_off, ngames, s, ws)) != hipSuccess) return fail(e);
  uint32_t total_plies = 0;
  if ((e = hipMemcpyAsync(&total_plies, ply_off + ngames, 4, hipMemcpyDeviceToHost, s)) != hipSuccess) return fail(e);
  if ((e = hipStreamSynchronize(s)) != hipSuccess) return fail(e);
  if (!children) {
    R.n_out = total_plies;
    R.n_groups = ngames;
    if (cap < total_plies || off_cap < (size_t)ngames + 1 || !d_out || !d_group_off) {
      R.capacity = true;
      return R;
    }
    if ((e = replay_vgames_device(variant, d_text, d_fen_off, d_mv_off, ply_off, ngames, d_out, nullptr, d_final, err,
                                  s)) != hipSuccess)
      return fail(e);
    if ((e = hipMemcpyAsync(d_group_off, ply_off, (size_t)(ngames + 1) * 4, hipMemcpyDeviceToDevice, s)) !=
        hipSuccess)
      return fail(e);
  } else {
    if (own && total_plies > own->max_groups) {  // the search's capacity: one record per ply
      R.n_groups = total_plies;
      R.capacity = true;
      return R;
    }
    if ((e = ws.get(W::kStates, (size_t)total_plies * state_bytes, &states)) != hipSuccess)
      return fail(e);
    if ((e = ws.get(W::kCnt, (size_t)(total_plies + 1) * 4, (void**)&cnt)) != hipSuccess) return fail(e);
    if ((e = ws.get(W::kCoff, (size_t)(total_plies + 1) * 4, (void**)&coff)) != hipSuccess) return fail(e);
    if ((e = replay_vgames_device(variant, d_text, d_fen_off, d_mv_off, ply_off, ngames, nullptr, states, d_final,
                                  err, s)) != hipSuccess)
      return fail(e);
    uint32_t herr[4];
    if ((e = hipMemcpyAsync(herr, err, 16, hipMemcpyDeviceToHost, s)) != hipSuccess) return fail(e);
    if ((e = hipStreamSynchronize(s)) != hipSuccess) return fail(e);
    if (herr[0]) {
      R.err_code = herr[0];
      R.err_game = herr[1];
      R.err_ply = herr[2];
      return R;
    }
    if ((e = vchildren_count_device(variant, states, total_plies, cnt, coff, s, ws)) != hipSuccess) return fail(e);
    uint32_t total = 0;
    if ((e = hipMemcpyAsync(&total, coff + total_plies, 4, hipMemcpyDeviceToHost, s)) != hipSuccess) return fail(e);
    if ((e = hipStreamSynchronize(s)) != hipSuccess) return fail(e);
    R.n_out = total;
    R.n_groups = total_plies;
    if (own) {
      if ((e = ws.get(W::kKids, (size_t)total * sizeof(fnnue_vpos), (void**)&own->pos)) != hipSuccess) return fail(e);
      if ((e = ws.get(W::kKidMoves, (size_t)total * 2, (void**)&own->moves)) != hipSuccess) return fail(e);
      if ((e = ws.get(W::kKidEnd, (size_t)total, (void**)&own->end)) != hipSuccess) return fail(e);
      own->off = coff;
      own->ply_off = ply_off;
      if ((e = vchildren_write_device(variant, states, total_plies, coff, total, own->pos, own->moves, own->end,
                                      s)) != hipSuccess)
        return fail(e);
    } else {
      if (cap < total || off_cap < (size_t)total_plies + 1 || !d_out || !d_group_off) {
        R.capacity = true;
        return R;
      }
      const dim3 cgrid((total_plies + bs - 1) / bs);
      if (d_moves && d_end) {
        if ((e = vchildren_write_device(variant, states, total_plies, coff, total, d_out, d_moves, d_end, s)) !=
            hipSuccess)
          return fail(e);
      } else {
        if (variant == kVariantKingOfTheHill)
          hipLaunchKernelGGL(pwrite_children_kernel<kVariantKingOfTheHill>, cgrid, dim3(bs), 0, s,
                             static_cast<const DBoard*>(states), total_plies, coff, d_out);
        else if (variant == kVariantRacingKings)
          hipLaunchKernelGGL(pwrite_children_kernel<kVariantRacingKings>, cgrid, dim3(bs), 0, s,
                             static_cast<const DBoard*>(states), total_plies, coff, d_out);
        else if (variant == kVariantThreeCheck)
          hipLaunchKernelGGL(pwrite_children_kernel<kVariantThreeCheck>, cgrid, dim3(bs), 0, s,
                             static_cast<const DBoard*>(states), total_plies, coff, d_out);
        else
          hipLaunchKernelGGL(vwrite_children_kernel, cgrid, dim3(bs), 0, s, static_cast<const vb::VBoard*>(states),
                             total_plies, coff, d_out);
        if ((e = hipGetLastError()) != hipSuccess) return fail(e);
      }
      if ((e = hipMemcpyAsync(d_group_off, coff, (size_t)(total_plies + 1) * 4, hipMemcpyDeviceToDevice, s)) !=
          hipSuccess)
        return fail(e);
    }
  }
  uint32_t herr[4];
  if ((e = hipMemcpyAsync(herr, err, 16, hipMemcpyDeviceToHost, s)) != hipSuccess) return fail(e);
  if ((e = hipStreamSynchronize(s)) != hipSuccess) return fail(e);
  R.err_code = herr[0];
  R.err_game = herr[1];
  R.err_ply = herr[2];
  return R;
}

}  // namespace fnnue
