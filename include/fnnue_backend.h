/* fnnue_backend.h — a batched static-evaluation backend with the shape of
 * fishnet's engine actor, above the evaluator ABI (fnnue.h).
 *
 * The reference sends every position of an acquired batch to a Stockfish
 * child over UCI, one position per round trip:
 *   stockfish::channel(exe, StockfishInit{nnue}, logger)
 *       -> (StockfishStub, StockfishActor)          [ref] src/stockfish.rs:23-38
 *   StockfishStub::go(Position)
 *       -> Result<PositionResponse, PositionFailed> [ref] src/stockfish.rs:44-54
 * with Position / PositionResponse / PositionFailed from src/ipc.rs:16-41,
 * 100-103, and the batch expanded by IncomingBatch::from_acquired
 * (src/queue.rs:518-627) from an AcquireResponseBody (src/api.rs:293-309).
 *
 * Here the same pair is a channel to one evaluator per net on one GPU: the
 * actor owns an fnnue_ctx per net (chess, and optionally the crazyhouse and
 * atomic Fairy-Stockfish variant nets); a go() hands it whole acquired
 * batches, which it answers on the calling thread, one call at a time (a
 * second caller waits, as on the reference's mpsc::channel(1)), returning
 * one response per position.
 * Each batch goes to the net of its variant (the reference picks the engine
 * by EngineFlavor, src/queue.rs:530-539, and the variant, src/assets.rs:
 * 384-391).  The expansion (FEN parse, UCI replay, every ply) runs on the
 * device (fnnue_build_batch_device / fnnue_build_vbatch_device), the plies are
 * evaluated incrementally along each game (CHAIN groups), and the two raw NNUE
 * terms become a Score::Cp.  A batch that fails (unparsable FEN, illegal move,
 * a variant this backend has no net for) gets its own nonzero code in
 * batch_rc — PositionFailed{batch_id} (queue.rs:207-213 drops that batch) —
 * while the other batches of the call complete.  A nonzero return of go()
 * itself (device failure) fails them all.
 *
 * Score (static evaluation; search is outside this path):
 *   v  = (psqt + positional) / 16            Stockfish's NNUE value (internal
 *                                             units, side to move, C division;
 *                                             upstream evaluate_nnue.cpp with
 *                                             adjusted = false — the "NNUE
 *                                             evaluation" the `eval` command
 *                                             prints)
 *   cp = v * 100 / normalize_to_pawn         UCI::value's normalisation (upstream
 *                                             uci.cpp; 361 in SF 15.1 as recalled,
 *                                             a parameter because it is unpinned)
 * Analysis work: one response per ply, depth 0, nodes 1, no pv / best move
 * (the default; fnnue_backend_set_analysis_depth(b, 1) answers chess batches
 * with a one-ply search per ply instead, and
 * fnnue_backend_set_variant_analysis_depth(b, 1) the variant batches, see there).
 * A position with no legal move (it can only be a game's last ply) is
 * answered as the engine answers it — `info depth 0 score mate 0` when the
 * side to move is checkmated (atomic: its king exploded), `score cp 0` when
 * stalemated, `bestmove (none)` (src/stockfish.rs:359-376, 418-425): score
 * Mate(0) / Cp(0), depth 0, nodes 0, no best move; psqt / positional still
 * carry the NNUE terms ((0, 0) for an exploded king).
 * Move work: the root after all moves; a one-ply search over its legal
 * children: a child that mates (checkmate, atomic explosion of the other
 * king) is chosen first (score Mate(1)), a stalemating child is worth 0, every
 * other child -v(child) from its NNUE evaluation; the first maximum is the
 * best move (depth 1, nodes = children).  A root with no legal move: no best
 * move, Mate(0) / Cp(0), depth 0, nodes 0.
 */
#ifndef FNNUE_BACKEND_H
#define FNNUE_BACKEND_H

#include "fnnue.h"

#ifdef __cplusplus
extern "C" {
#endif

#define FNNUE_WORK_ANALYSIS 0 /* Work::Analysis (api.rs:130-143) */
#define FNNUE_WORK_MOVE 1     /* Work::Move (api.rs:144-151) */

#define FNNUE_SCORE_CP 0      /* Score::Cp (api.rs:383-388) */
#define FNNUE_SCORE_MATE 1    /* Score::Mate */

typedef struct fnnue_backend fnnue_backend;

/* StockfishInit (stockfish.rs): what the engine is configured with. */
typedef struct {
  int32_t normalize_to_pawn; /* cp = v * 100 / normalize_to_pawn; 0 -> 361 */
  uint32_t timeout_ms;       /* budget of one go(): 0 -> 60000, the worker's cap min(60 s, budget)
                                ([ref] src/main.rs:316); see fnnue_backend_go_timeout */
} fnnue_backend_init;

/* AcquireResponseBody (api.rs:293-309) of one batch. */
typedef struct {
  const char *batch_id;            /* Work::id (BatchId), copied into logs / errors */
  int work;                        /* FNNUE_WORK_* */
  int multipv;                     /* Work::Analysis multipv: 0 = None; >= 1 = Some(k): the response is the
                                      matrix form (AnalysisPart::Matrix, Work::matrix_wanted, api.rs:179-187).
                                      go() answers its one line (at depth 0 a static eval has no second PV);
                                      on a depth-1 channel fnnue_backend_go_lines answers min(k, legal moves)
                                      lines per ply */
  const char *position;            /* root FEN (X-FEN / Shredder castling accepted) */
  const char *variant;             /* "standard", "chess960", "fromPosition", NULL / "" = standard;
                                      "crazyhouse", "atomic" (variant nets); anything else: FNNUE_E_ARCH */
  const char *moves;               /* space-separated UCI (Chess960 king-takes-rook accepted) */
  const uint32_t *skip_positions;  /* skipPositions: position ids answered as Skipped */
  size_t nskip;
} fnnue_acquired;

/* PositionResponse (ipc.rs:28-39) of one position (Skip::Skip when skipped). */
typedef struct {
  uint32_t position_id;  /* PositionId: 0 = root, k = after k moves */
  uint8_t skipped;       /* 1: Skip::Skip (AnalysisPart::Skipped) */
  uint8_t score_kind;    /* FNNUE_SCORE_* */
  uint8_t depth;
  uint8_t matrix;        /* 1: serialise as AnalysisPart::Matrix (multipv requested) */
  int64_t score;         /* centipawns (side to move) */
  int32_t psqt;          /* the raw NNUE terms the score came from */
  int32_t positional;
  uint64_t nodes;
  uint64_t time_ms;      /* wall time of the go() call until this position's piece was back on the host */
  uint32_t nps;          /* positions evaluated by then, per second */
  char best_move[8];     /* UCI, NUL-terminated; "" for analysis at depth 0 */
} fnnue_position_response;

/* The nets of one backend, by the batches they evaluate.  Any may be NULL
 * (not all); a batch whose variant has no net fails with FNNUE_E_ARCH. */
typedef struct {
  const fnnue_net *chess;      /* standard / chess960 / fromPosition: a HalfKAv2_hm net */
  const fnnue_net *crazyhouse; /* a FNNUE_VARIANT_CRAZYHOUSE net (fnnue_net_load_variant) */
  const fnnue_net *atomic;     /* a FNNUE_VARIANT_ATOMIC net */
} fnnue_backend_nets;

/* stockfish::channel: starts the actor (one evaluator per net on `device`, a
 * few host threads for the per-batch loops of large calls).  A net in the
 * wrong slot: FNNUE_E_ARCH.  init may be NULL (defaults).  The nets may be
 * freed after the call. */
int fnnue_backend_channel_nets(const fnnue_backend_nets *nets, int device, const fnnue_backend_init *init,
                               fnnue_backend **out);
/* Any set of nets, each going to the slot of its own variant
 * (fnnue_net_variant: chess, crazyhouse, atomic, kingofthehill, racingkings,
 * threecheck; fnnue_backend_nets keeps its three members, its size being ABI).  n >= 1;
 * two nets of one variant: FNNUE_E_ARG. */
int fnnue_backend_channel_netv(const fnnue_net *const *nets, size_t n, int device, const fnnue_backend_init *init,
                               fnnue_backend **out);
/* The one-net form: the net goes to the slot of its variant. */
int fnnue_backend_channel(const fnnue_net *net, int device, const fnnue_backend_init *init, fnnue_backend **out);
/* Stops the actor (after the call in flight) and frees it.  Never waits for
 * the device: when a timed-out call's work is still running on the channel's
 * streams, its buffers are released later (by a later channel() or free()),
 * once the streams have drained. */
void fnnue_backend_free(fnnue_backend *b);

/* Analysis depth of the channel: 0 (the default: a static evaluation per ply)
 * or 1; anything else is FNNUE_E_ARG.  A setter because the size of
 * fnnue_backend_init is ABI.  Takes effect with the next go().
 * At depth 1 every non-skipped ply of a chess analysis batch (standard,
 * chess960, fromPosition) is answered by a one-ply search over its legal
 * children on the device (fnnue_search1_device's three steps per piece: the
 * children with their moves and end flags, their STAR evaluation, the
 * reduction to a fnnue_best), by the rule of move work: an evaluated best child
 * gives Score::Cp(value * 100 / normalize_to_pawn), a mating child
 * Score::Mate(1); depth 1, nodes = the children, best_move = the pv's one move
 * ([ref] AnalysisPart::Best::pv, src/api.rs:359-369), psqt / positional the best
 * child's, negated.  A ply without a legal move is answered exactly as at
 * depth 0 (mate 0 / cp 0, depth 0, nodes 0, no move); skipped ids stay
 * skipped; move work is unchanged.  Variant batches (crazyhouse, atomic,
 * kingOfTheHill, racingKings, threeCheck) are not affected by this setter: they are
 * answered at depth 0 exactly as on a depth-0 channel unless
 * fnnue_backend_set_variant_analysis_depth (below) says otherwise.
 * Pieces are cut at a 32nd of FNNUE_BACKEND_PIECE_PLIES, so that a piece's
 * children (about 35 per ply) take the room a depth-0 piece's plies do; each
 * piece reads its children count back once (a bounded wait inside the call's
 * budget).  fnnue_backend_stats.positions counts plies plus children.
 * fnnue_backend_go_compact on a depth-1 channel gives the depth-1 score and
 * depth = 1 but no move and no node count: the 16-byte record has no room for
 * them (nodes reads as 1, as at depth 0).
 * MultiPV: every child of every ply is evaluated at depth 1, so a chess
 * analysis batch with multipv = k >= 1 can be answered with its k best lines
 * per ply.  go(), go_timeout() and go_compact() keep answering the best line
 * alone (and launch nothing more than before); fnnue_backend_go_lines runs one
 * more kernel per piece (fnnue_topk_children_device's) and returns the lines
 * beside the responses. */
int fnnue_backend_set_analysis_depth(fnnue_backend *b, int depth);
/* The same for the variant nets (ABI 3.6), independent of the chess setting:
 * 0 (the default) or 1, anything else FNNUE_E_ARG.  At 1 every non-skipped ply
 * of a crazyhouse, atomic, kingOfTheHill, racingKings or threeCheck analysis batch is
 * answered with a one-ply search on the device under the variant's rules
 * (fnnue_vsearch1's steps), by the rule of move work: a child that ends the
 * game for the opponent (checkmate, an exploded king, the variant's rule: threeCheck's last check) is
 * Mate(1); a child the mover has lost by playing (racingKings: black fails to
 * catch up) is chosen only when there is nothing else, Mate(-1); otherwise
 * Cp(value * 100 / normalize_to_pawn).  depth 1, nodes = the children,
 * best_move spelled by fnnue_vmove_uci (drops as "N@f3").  A ply without a
 * legal move is answered as at depth 0; move work is unchanged; go_compact
 * gives the score without a move; fnnue_backend_go_lines gives such plies their
 * min(multipv, nodes, 218) lines.  Pieces are cut at an 8th of
 * FNNUE_BACKEND_PIECE_PLIES, and a piece's children buffers are sized from the
 * count that is read back (a crazyhouse ply with full pockets has several
 * hundred children). */
int fnnue_backend_set_variant_analysis_depth(fnnue_backend *b, int depth);

/* Number of responses batch `a` expands to (IncomingBatch::from_acquired):
 * analysis = moves + 1, move = 1.  Host only; FNNUE_E_ARG on a bad work type. */
int fnnue_backend_batch_size(const fnnue_acquired *a, size_t *n);

/* StockfishStub::go for whole batches.  Batch i's responses land in
 * out[off[i] .. off[i + 1]) (off: nbatches + 1 entries, filled here; cap =
 * capacity of out, FNNUE_E_CAPACITY when too small); batch_rc[i] = 0 or the
 * FNNUE_E_* code of its PositionFailed (its responses then are unspecified).
 * Thread-safe: concurrent callers queue on the capacity-1 channel. */
int fnnue_backend_go(fnnue_backend *b, const fnnue_acquired *batches, size_t nbatches, fnnue_position_response *out,
                     size_t cap, uint32_t *off, int32_t *batch_rc);

/* go() with its own budget (timeout_ms; 0 = the channel's init.timeout_ms).
 * The reference worker races each go against `min(60 s, budget) +
 * work.timeout()` and, when it runs out, drops the engine (the child is
 * killed) and fails the batch ([ref] src/main.rs:316, 343-351;
 * src/stockfish.rs:138).  Here every wait of the call is bounded by that
 * deadline; on expiry the call returns FNNUE_E_TIMEOUT at once, without
 * waiting for the device: batch_rc[i] = 0 for the batches whose responses were
 * written before the deadline (valid), FNNUE_E_TIMEOUT for the others.  The
 * channel is then broken — the device may still be working in its buffers —
 * and every later go() on it fails fast with FNNUE_E_TIMEOUT; free it and open
 * a new channel (the worker's drop-and-restart). */
int fnnue_backend_go_timeout(fnnue_backend *b, const fnnue_acquired *batches, size_t nbatches,
                             fnnue_position_response *out, size_t cap, uint32_t *off, int32_t *batch_rc,
                             uint32_t timeout_ms);

/* The compact form of a go()'s answer (16 B per position instead of 56, and
 * what is the same for all of a batch's positions once per batch): what a
 * caller that builds its own response objects needs — fishnet's actor builds
 * PositionResponse (ipc.rs:28-39) in Rust memory anyway, so the 56-byte C
 * record is an intermediate it need not pay for.  Same semantics as
 * fnnue_position_response field by field:
 *   nodes     = 0 when flags has FNNUE_COMPACT_SKIPPED or FNNUE_COMPACT_NO_MOVES,
 *               else 1 for an analysis position, fnnue_batch_compact.nodes for
 *               the answer of a move batch;
 *   best_move = fnnue_batch_compact.best_move (move work), else none;
 *   time_ms / nps = the batch's (every position of a batch gets its piece's).
 * score is 32-bit: exact for normalize_to_pawn >= 13 (|psqt + positional| <
 * 2^32), which the compact call requires. */
#define FNNUE_COMPACT_SKIPPED 1   /* Skip::Skip: nothing else set */
#define FNNUE_COMPACT_MATRIX 2    /* serialise as AnalysisPart::Matrix */
#define FNNUE_COMPACT_NO_MOVES 4  /* a position without a legal move: mate 0 / cp 0, nodes 0, depth 0 */
typedef struct {
  int32_t psqt;
  int32_t positional;
  int32_t score;         /* centipawns or mate (score_kind), side to move */
  uint8_t score_kind;    /* FNNUE_SCORE_* */
  uint8_t depth;
  uint8_t flags;         /* FNNUE_COMPACT_* */
  uint8_t reserved;
} fnnue_position_compact;

typedef struct {
  uint64_t time_ms;      /* wall time of the go() call until the batch's piece was back on the host */
  uint32_t nps;          /* positions evaluated by then, per second */
  uint32_t nodes;        /* move work: the legal children searched (0 for a root without one); analysis: 0 */
  char best_move[8];     /* move work: UCI, NUL-terminated; "" otherwise */
} fnnue_batch_compact;

/* go() answering in the compact form: batch i's positions in out[off[i] ..
 * off[i + 1]) (cap = capacity of out), its per-batch part in bout[i]; budget
 * and errors as fnnue_backend_go_timeout.  FNNUE_E_ARG when the channel's
 * normalize_to_pawn is below 13. */
int fnnue_backend_go_compact(fnnue_backend *b, const fnnue_acquired *batches, size_t nbatches,
                             fnnue_position_compact *out, size_t cap, fnnue_batch_compact *bout, uint32_t *off,
                             int32_t *batch_rc, uint32_t timeout_ms);

/* Where the last go() spent its time (diagnostics; the reference's engine
 * reports only time / nps per position).  Each net's games are cut into pieces
 * of about FNNUE_BACKEND_PIECE_PLIES plies (default 524288); a piece is one
 * host-to-device copy, the replay, the evaluation kernels and one device-to-
 * host copy of its results (plus the evaluator's error word), in order on the
 * net's stream; the host stages the next pieces and writes a piece's
 * responses while the device works on the later ones, in the order the
 * pieces come back (another net's may be written first), blocking only when
 * a single net is left. */
typedef struct {
  double prep_ms;         /* host: sizes, move-work roots, text staging, copies and kernels enqueued */
  double device_ms;       /* host waiting for the device (blocked, or polling the nets' pieces) */
  double fill_ms;         /* responses written (overlaps the device's later pieces) */
  double total_ms;
  uint64_t positions;     /* positions evaluated (analysis plies + move-work children; + searched children, grandchildren) */
  uint32_t stream_syncs;  /* host blocking waits on an event, a stream or a copy */
  uint32_t rebuilds;      /* extra passes after a batch failed (per failed batch, its piece only) */
  uint32_t host_threads;  /* threads for the staging / fill loops (FNNUE_BACKEND_THREADS; default: the usable CPUs, at most 8) */
  uint32_t pieces;        /* pieces over all nets */
} fnnue_backend_stats;

int fnnue_backend_last_stats(fnnue_backend *b, fnnue_backend_stats *out);

/* The `analysis` array fishnet submits for one analysis batch
 * (CompletedBatch::into_analysis, queue.rs:715-727; AnalysisPart / Score
 * serialisation, api.rs:355-388): {"skipped":true} or {"score":{"cp":..},
 * "depth":..,"nodes":..,"time":..,"nps":..} per position, or for a MultiPV
 * batch the matrix form {"pv":[[[]]],"score":[[{"cp":..}]],"depth":0,...}
 * (Matrix::set(multipv 1, depth 0): one row, one column), as JSON.  A
 * response with a best move (analysis at depth 1) carries it as its pv:
 * {"pv":"e2e4","score":{..},..} (AnalysisPart::Best: space-separated, omitted
 * when empty), and the matrix form puts its one line at column `depth`
 * (Matrix::set, [ref] src/ipc.rs:77-86): {"pv":[[null,["e2e4"]]],
 * "score":[[null,{"cp":..}]],"depth":1,...}.  Writes
 * at most cap bytes including the NUL; *len = the full length (without NUL);
 * FNNUE_E_CAPACITY when it did not fit. */
int fnnue_backend_analysis_json(const fnnue_position_response *r, size_t n, char *buf, size_t cap, size_t *len);

/* ---- MultiPV at analysis depth 1 (ABI 3.5) ----
 * One line of a response: the reference collects one score and one pv per
 * MultiPV line into Matrix<Score> / Matrix<Vec<Uci>>, indexed [multipv - 1]
 * [depth] ([ref] src/ipc.rs:68-93, src/stockfish.rs:350-445).  The sizes of
 * fnnue_position_response and fnnue_best being ABI, the lines travel beside
 * the responses. */
typedef struct {
  int64_t score;        /* centipawns or mate, as fnnue_position_response.score */
  int32_t psqt;         /* this child's raw NNUE terms, negated */
  int32_t positional;
  char move[7];         /* UCI, NUL-terminated: the line's pv, one move */
  uint8_t score_kind;   /* FNNUE_SCORE_* */
} fnnue_pv_line;

/* Lines a go_lines() over these batches may write: the sum over analysis
 * batches with multipv >= 1 of (moves + 1) * min(multipv, FNNUE_MAX_CHILDREN)
 * (skipped positions are not subtracted).  Host only; FNNUE_E_ARG on NULL. */
int fnnue_backend_lines_bound(const fnnue_acquired *batches, size_t nbatches, size_t *n);

/* fnnue_backend_go_timeout plus the lines: out, off and batch_rc are filled
 * exactly as there (every response equals go()'s field by field but for
 * time_ms / nps); response r's lines are lines[line_off[r] .. line_off[r + 1])
 * (line_off: cap + 1 entries, off[nbatches] + 1 of them written).
 * A response has lines iff the channel is at depth 1, it belongs to a chess
 * analysis batch with multipv >= 1, it is not skipped and its ply has a legal
 * move; it then has min(multipv, nodes) of them (as Stockfish answers a
 * MultiPV beyond the legal moves), best first in fnnue_topk_children's order,
 * line 0 being the response's own score, score_kind, best_move, psqt and
 * positional.  Line j's score follows the depth-1 rule: Cp(value * 100 /
 * normalize_to_pawn), Mate(1) for a mating child.  Every other response has
 * none: a depth-0 channel, variant batches, move work, batches without
 * multipv, skipped ids, plies without a legal move, failed batches.
 * lines_cap < fnnue_backend_lines_bound(...) is FNNUE_E_CAPACITY before any
 * work.  Budget and errors as fnnue_backend_go_timeout. */
int fnnue_backend_go_lines(fnnue_backend *b, const fnnue_acquired *batches, size_t nbatches,
                           fnnue_position_response *out, size_t cap, uint32_t *off, int32_t *batch_rc,
                           fnnue_pv_line *lines, size_t lines_cap, uint32_t *line_off, uint32_t timeout_ms);

/* fnnue_backend_analysis_json with the lines of a go_lines() (line_off: n + 1
 * entries, relative to r[0]: response i's lines are lines[line_off[i] -
 * line_off[0] ..)).  A response with L >= 1 lines at depth d is the matrix as
 * Matrix::set builds it ([ref] src/ipc.rs:77-86), L rows of d nulls and the
 * entry: {"pv":[[null,["e2e4"]],[null,["d2d4"]]],"score":[[null,{"cp":31}],
 * [null,{"cp":28}]],"depth":1,...}.  A response without lines (or without
 * `matrix`: lines are rows of the matrix form only) is serialised as
 * fnnue_backend_analysis_json does it, so whenever every response has at most
 * one line the two functions give the same bytes. */
int fnnue_backend_analysis_json_lines(const fnnue_position_response *r, size_t n, const fnnue_pv_line *lines,
                                      const uint32_t *line_off, char *buf, size_t cap, size_t *len);

/* ---- analysis at two plies (ABI 3.7) ----
 * fnnue_backend_set_analysis_plies(b, plies): 0, 1 or 2, anything else
 * FNNUE_E_ARG.  0 and 1 are fnnue_backend_set_analysis_depth(b, 0 / 1), on the
 * same field (that setter keeps refusing 2).  At 2 every non-skipped ply of a
 * chess analysis batch is answered with fnnue_search2's full-width two-ply
 * search on the device (fnnue.h, fnnue_best2): Score::Cp(value * 100 /
 * normalize_to_pawn), Mate(1) (a mate in one) or Mate(-1) (every move allows a
 * mate in one); depth = the pv's length, 2, or 1 when the best move ends the
 * game; nodes = children + grandchildren; best_move = the pv's first move;
 * psqt / positional = the record's (the pv's last position, from the ply's
 * side to move).  A ply without a legal move is answered as at depth 0;
 * skipped ids, move work and variant batches are unchanged; go_compact gives
 * score and depth only.  fnnue_backend_go_lines on a 2-plies channel behaves
 * as on a 1-ply channel: depth-1 responses and lines; MultiPV at two plies is
 * fnnue_backend_go_lines_pv (below).  Pieces are cut at a 1024th of FNNUE_BACKEND_PIECE_PLIES (at
 * least 16 plies), so that a piece's grandchildren (about 1000 per ply) take
 * the room a depth-0 piece's plies do; each piece has two bounded sizing waits
 * (children, grandchildren) inside the call's budget; a piece with a rejected
 * game skips the search.  fnnue_backend_stats.positions counts plies +
 * children + grandchildren. */
int fnnue_backend_set_analysis_plies(fnnue_backend *b, int plies);
/* fnnue_backend_go_timeout plus the pv's second move: reply[i] is parallel to
 * out[i] (cap entries), the reply's fnnue_move code (fnnue_move_uci prints it)
 * or 0 for none: a channel below 2 plies, a one-move pv, a ply without a legal
 * move, skipped ids, move work, variant batches (below 2 variant plies, see
 * fnnue_backend_set_variant_analysis_plies), failed batches.  The
 * responses are those of go() / go_timeout() on the same channel. */
int fnnue_backend_go_pv(fnnue_backend *b, const fnnue_acquired *batches, size_t nbatches,
                        fnnue_position_response *out, size_t cap, uint32_t *off, int32_t *batch_rc, fnnue_move *reply,
                        uint32_t timeout_ms);
/* fnnue_backend_analysis_json with the replies of a go_pv() (reply: n entries
 * parallel to r, or NULL): a response with a best move and a reply carries
 * both as its pv, "pv":"e2e4 e7e5" (space-separated, as Vec<Uci> is
 * serialised; the matrix form: ["e2e4","e7e5"]).  Without a reply the bytes
 * are fnnue_backend_analysis_json's. */
int fnnue_backend_analysis_json_pv(const fnnue_position_response *r, size_t n, const fnnue_move *reply, char *buf,
                                   size_t cap, size_t *len);

/* ---- variant analysis at two plies (ABI 3.10) ----
 * fnnue_backend_set_variant_analysis_plies(b, plies): 0, 1 or 2, anything else
 * FNNUE_E_ARG.  0 and 1 are fnnue_backend_set_variant_analysis_depth(b, 0 / 1),
 * on the same field (that setter keeps refusing 2); the chess setting is
 * another field and neither setter moves the other's.  At 2 every non-skipped
 * ply of a crazyhouse, atomic, kingOfTheHill, racingKings or threeCheck
 * analysis batch is answered with fnnue_vsearch2's two-ply search under the
 * variant's rules and ranks: Cp(value * 100 / normalize_to_pawn); Mate(1) for
 * FNNUE_BEST_MATE, at a one-move pv (the move ends the game) or a two-move pv
 * (every reply loses at once); Mate(-1) for FNNUE_BEST_MATED (every move
 * allows a reply that wins at once) and FNNUE_BEST_LOST (every move loses at
 * once); depth = the pv's length; nodes = children + grandchildren; best_move
 * spelled by fnnue_vmove_uci.  fnnue_backend_go_pv's reply is then a variant
 * move code (fnnue_vmove_uci prints it; fnnue_backend_analysis_json_pv does:
 * "pv":"N@f3 e7e5").  Staging is the chess channel's at two plies: pieces cut at
 * a 256th of FNNUE_BACKEND_PIECE_PLIES (at least 16 plies; four times the
 * chess cut measured fastest on crazyhouse), two bounded sizing waits per piece, a
 * piece with a rejected game skips the search and is recovered as at depth 1,
 * positions counts plies + children + grandchildren.  fnnue_backend_go_lines on
 * such a channel is a one-ply search with lines, as on a one-ply channel;
 * fnnue_backend_go_lines_pv gives the k best two-move lines.  Move work is
 * unchanged. */
int fnnue_backend_set_variant_analysis_plies(fnnue_backend *b, int plies);

/* ---- repetition and fifty-move draws (ABI 3.12) ----
 * fnnue_backend_set_draw_rules(b, on) (default off): on, every chess analysis
 * batch searched at 1 or 2 plies (go, go_timeout, go_pv, go_lines, go_lines_pv,
 * go_compact) marks the searched positions that are drawn by repetition or the
 * fifty-move rule, the game before the ply counted (fnnue.h: FNNUE_END_DRAW,
 * fnnue_set_search_draws): such a move is worth 0 and ends the pv, so a drawn
 * best move answers as a stalemating one does: Score::Cp(0), depth = the pv's
 * length, "pv":"f6g8".  A piece holds whole games, so the history is complete.
 * The ply itself is never tested; nodes do not change.  Depth 0, move work and
 * variant batches are unchanged (variant batches: ABI 3.16, below). */
int fnnue_backend_set_draw_rules(fnnue_backend *b, int on);
int fnnue_backend_draw_rules(fnnue_backend *b, int *on);

/* ---- capture quiescence below the searches' leaves (ABI 3.13) ----
 * fnnue_backend_set_quiesce(b, depth) (default 0, at most FNNUE_QUIESCE_MAX:
 * FNNUE_E_ARG): every chess analysis batch searched at 1 or 2 plies (go,
 * go_timeout, go_pv, go_lines, go_lines_pv, go_compact) replaces its leaves'
 * terms by those of their capture line's end (fnnue.h: the rule and what
 * stays), before the piece's reductions: the same device function at both
 * reduction sites.  Depth-0 analysis, move work, variant batches, `nodes` /
 * `positions` and the JSON shapes are unchanged, and the setting composes with
 * the draw rules.  With quiescence on, a piece reads each level's size back
 * (one more blocking wait per level and slice, counted in stream_syncs, and not
 * bounded by the call's deadline as the sizing waits are): what is said above
 * about a piece's one or two sizing waits holds with quiescence off only. */
int fnnue_backend_set_quiesce(fnnue_backend *b, int depth);
int fnnue_backend_quiesce(fnnue_backend *b, int *depth);

/* ---- check evasions and mates inside the quiescence (ABI 3.14) ----
 * fnnue_backend_set_quiesce_checks(b, on) (off by default): the quiescence of
 * the chess analysis batches follows Q' (fnnue.h), and a FNNUE_BEST_CP result
 * or line whose |value| > FNNUE_VALUE_MATE - 64 is answered as
 * FNNUE_SCORE_MATE: plies = FNNUE_VALUE_MATE - |value|, a win is +(plies + 1)
 * / 2, a loss -plies / 2, at every fill site (best, best2, lines, lines2, the
 * compact form; the JSON prints "mate").  Reported psqt / positional are the
 * coded terms.  With the setting off no value is ever remapped.  Move work,
 * variant batches, depth-0 analysis and batches with quiescence depth 0 are
 * unchanged. */
int fnnue_backend_set_quiesce_checks(fnnue_backend *b, int on);
int fnnue_backend_quiesce_checks(fnnue_backend *b, int *on);

/* ---- capture quiescence for variant batches (ABI 3.15) ----
 * fnnue_backend_set_variant_quiesce(b, depth, checks) (default 0 / off, depth at
 * most FNNUE_QUIESCE_MAX: FNNUE_E_ARG): variant analysis batches at one and two
 * plies, through every go* call, put the variants' quiescence (fnnue.h, ABI
 * 3.15) below their searches' leaves, at both reduction sites.  With depth > 0
 * a coded mate (|value| > FNNUE_VALUE_MATE - 64) is answered as Score::Mate by
 * the conversion of ABI 3.14 at every fill site; the variants' rule decides
 * finished positions with checks off too, so the condition is the depth alone.
 * Move work, depth-0 analysis, chess batches and a backend without the setting
 * are unchanged; fnnue_backend_set_quiesce[_checks] keep applying to chess
 * batches only. */
int fnnue_backend_set_variant_quiesce(fnnue_backend *b, int depth, int checks);
int fnnue_backend_variant_quiesce(fnnue_backend *b, int *depth, int *checks);

/* ---- repetition and fifty-move draws for variant batches (ABI 3.16) ----
 * fnnue_backend_set_variant_draw_rules(b, on) (default off): on, every variant
 * analysis batch searched at 1 or 2 plies, through every go* call, marks the
 * searched positions that are drawn under its variant's rule (fnnue.h, ABI
 * 3.16: crazyhouse has repetition only, with pockets and promoted marks in the
 * identity; threecheck's identity has the check counters), at the place
 * fnnue_backend_set_draw_rules acts for chess batches and before the variant
 * quiescence.  A drawn best move answers Score::Cp(0), depth 1, a one-move pv.
 * Move work, depth-0 analysis and chess batches are unchanged, and
 * fnnue_backend_set_draw_rules keeps applying to chess batches only. */
int fnnue_backend_set_variant_draw_rules(fnnue_backend *b, int on);
int fnnue_backend_variant_draw_rules(fnnue_backend *b, int *on);

/* ---- MultiPV at two plies (ABI 3.11) ----
 * One line of a response with its whole pv, as the reference keeps one
 * Vec<Uci> per MultiPV line at the searched depth ([ref] src/ipc.rs:68-93). */
typedef struct {
  int64_t score;        /* as fnnue_pv_line */
  int32_t psqt;         /* of the pv's last position, from the ply's side to move (fnnue_line2) */
  int32_t positional;
  char pv[14];          /* "e7e8q e2e1q": one or two UCI moves, space-separated, NUL-terminated; variant moves
                           as fnnue_vmove_uci spells them ("N@f3 e7e5") */
  uint8_t score_kind;   /* FNNUE_SCORE_* */
  uint8_t pv_len;       /* 1 or 2 */
} fnnue_pv_line2;
/* fnnue_backend_go_lines with every line's whole pv, and fnnue_backend_go_pv's
 * `reply` (cap entries, or NULL).  The responses and the replies are
 * fnnue_backend_go_pv's on the same channel, field by field but for time_ms /
 * nps: the call searches at the channel's own plies.  A response has lines iff
 * it belongs to an analysis batch with multipv >= 1, it is not skipped, its
 * ply has a legal move and its net's setting (chess and the variants each have
 * their own) is at one or two plies.  At two plies it has min(multipv, the
 * ply's legal moves) lines in fnnue_topk_replies' order (the variants:
 * fnnue_vtopk_replies'), line 0 being the response's own score, score_kind,
 * best move, reply, psqt and positional; scores are Cp(value * 100 /
 * normalize_to_pawn), Mate(1) for FNNUE_BEST_MATE, Mate(-1) for
 * FNNUE_BEST_MATED and FNNUE_BEST_LOST.  At one ply the lines are
 * fnnue_backend_go_lines' own in this record, pv_len 1.  Every other response
 * has none.  fnnue_backend_lines_bound stays the bound: lines_cap below it is
 * FNNUE_E_CAPACITY before any work.  One more kernel per piece
 * (fnnue_topk_replies_device's, beside the second reduction), the lines travel
 * in the piece's results image; no new wait; budget, errors and the recovery
 * of a piece with a rejected game as fnnue_backend_go_timeout. */
int fnnue_backend_go_lines_pv(fnnue_backend *b, const fnnue_acquired *batches, size_t nbatches,
                              fnnue_position_response *out, size_t cap, uint32_t *off, int32_t *batch_rc,
                              fnnue_pv_line2 *lines, size_t lines_cap, uint32_t *line_off, fnnue_move *reply,
                              uint32_t timeout_ms);
/* fnnue_backend_analysis_json_lines for these lines: a response with L >= 1
 * lines at depth d is L rows of d nulls and the entry, each entry holding that
 * line's own pv whatever its length: {"pv":[[null,null,["e2e4","e7e5"]],
 * [null,null,["d2d4","d7d5"]]],"score":[[null,null,{"cp":31}],[null,null,
 * {"cp":28}]],"depth":2,...}.  A response with one line prints as
 * fnnue_backend_analysis_json_pv prints it with that line's reply; a response
 * without lines, or not in `matrix` form, as fnnue_backend_analysis_json_pv
 * prints it without a reply (the call takes none: a batch that is not in
 * matrix form goes through fnnue_backend_analysis_json_pv with its replies). */
int fnnue_backend_analysis_json_lines_pv(const fnnue_position_response *r, size_t n, const fnnue_pv_line2 *lines,
                                         const uint32_t *line_off, char *buf, size_t cap, size_t *len);

#ifdef __cplusplus
}
#endif
#endif
