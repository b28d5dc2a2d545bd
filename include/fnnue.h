/*
 * fnnue.h — C ABI of the MI355X batched NNUE evaluator (libfnnue.so).
 *
 * This is the drop-in boundary for fishnet's static-evaluation path.  The
 * reference has no FFI for NNUE: it drives a Stockfish child over UCI text
 * pipes.  Each entry point below names the reference interface it replaces.
 *
 *   [ref] = /root/reference (schlawg/fishnet).  Upstream = Stockfish 15.1
 *   (submodule Stockfish/, empty in the reference checkout).
 *
 * Conventions
 *  - Every function returns FNNUE_OK (0) or a negative FNNUE_E_* code and then
 *    sets a thread-local message readable with fnnue_last_error().  No aborts,
 *    no exits.  On error no output is guaranteed (the caller maps any error to
 *    fishnet's PositionFailed{batch_id}, [ref] src/ipc.rs:100-103,
 *    src/queue.rs:207-213: the whole batch is dropped, never partial results).
 *  - Host buffers are owned by the caller; device memory of a ctx is owned by
 *    the library.  *_device entry points take device pointers and a hipStream_t
 *    (as void*), enqueue work and return without synchronising.
 *  - A fnnue_net is immutable and may be shared across threads; a fnnue_ctx
 *    must not be used from two threads at once (one ctx per GPU — the analogue
 *    of one engine per worker, [ref] src/main.rs:158-170).  Calls on one ctx
 *    share its device workspace: *_device calls on different streams are
 *    ordered by the library (a call on a new stream waits for the previous
 *    call's stream), so they serialise rather than race.
 *  - Outputs per position are the two raw Stockfish NNUE terms, before
 *    optimism / material scaling (upstream evaluate_nnue.cpp evaluate()):
 *      psqt       = (psqtAcc[stm][bucket] - psqtAcc[~stm][bucket]) / 2
 *      positional = Network[bucket].propagate(transformed features)
 *    Stockfish's NNUE value is (psqt + positional) / 16 (OutputScale).
 */
#ifndef FNNUE_H
#define FNNUE_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define FNNUE_OK 0
#define FNNUE_E_ARG (-1)        /* bad argument (null pointer, size, mode)           */
#define FNNUE_E_IO (-2)         /* file could not be read / written                   */
#define FNNUE_E_FORMAT (-3)     /* .nnue version / hash / truncated / trailing bytes  */
#define FNNUE_E_ARCH (-4)       /* architecture not supported (HD)                     */
#define FNNUE_E_DEVICE (-5)     /* HIP runtime error or no such device                */
#define FNNUE_E_POSITION (-6)   /* invalid position in a batch (kings, pieces, stm)   */
#define FNNUE_E_OOM (-7)        /* host or device allocation failed                    */
#define FNNUE_E_MOVE (-8)       /* illegal or unparsable UCI move                      */
#define FNNUE_E_FEN (-9)        /* unparsable FEN                                      */
#define FNNUE_E_CAPACITY (-10)  /* output buffer too small                             */
#define FNNUE_E_TIMEOUT (-11)   /* fnnue_backend_go overran its time budget           */

typedef struct fnnue_net fnnue_net; /* parsed, validated, immutable host copy of a .nnue */
typedef struct fnnue_ctx fnnue_ctx; /* one GPU: device-resident net + workspaces          */

/* Packed position, 36 bytes.  sq[s>>1] holds square s (A1=0..H8=63) in its low
 * nibble for even s and high nibble for odd s, as a Stockfish Piece code
 * (W_PAWN=1..W_KING=6, B_PAWN=9..B_KING=14, 0 = empty; upstream types.h).
 * stm: 0 = white, 1 = black.  Castling rights, en-passant square and move
 * counters do not enter the NNUE features and are not stored. */
typedef struct {
  uint8_t sq[32];
  uint8_t stm;
  uint8_t pad[3];
} fnnue_pos;

/* Packed position of a Fairy-Stockfish variant (48 bytes): the board and side
 * to move as fnnue_pos, then the pieces in hand (crazyhouse pockets): hand[0..4]
 * = white P N B R Q, hand[5..9] = black P N B R Q, each <= 16; all zero for
 * variants without pockets. */
typedef struct {
  uint8_t sq[32];
  uint8_t stm;
  uint8_t hand[10];
  uint8_t pad[5];
} fnnue_vpos;

/* ---- errors ---- */
const char *fnnue_last_error(void);
/* ABI version: (major << 16) | minor. */
uint32_t fnnue_abi_version(void);

/* ---- net loading ----
 * Replaces `setoption name EvalFile value <path>` sent to the engine
 * ([ref] src/stockfish.rs:209-211; path from src/assets.rs:128-133, 449-453;
 * upstream evaluate_nnue.cpp load_eval/read_parameters).  Accepts plain and
 * COMPRESSED_LEB128 tensors, checks version 0x7AF32F20, the structure hash
 * chain and exact EOF. */
int fnnue_net_load(const char *path, fnnue_net **out);
int fnnue_net_load_mem(const void *buf, size_t len, fnnue_net **out);
/* Net identity ([ref] build.rs:7 pins nn-ad9b42354671.nnue; build.rs:100-112
 * deletes a corrupt download): fnnue_net_load / fnnue_net_load_variant compute
 * the SHA-256 of the file, and when its basename is nn-<12 lowercase hex>.nnue
 * (upstream's naming: the first 12 hex digits of the digest) a mismatch fails
 * with FNNUE_E_FORMAT.  digest: 32 bytes (also for nets loaded from memory). */
int fnnue_net_sha256(const fnnue_net *net, uint8_t *digest);
/* hd = TransformedFeatureDimensions (1024 for nn-ad9b42354671, [ref] build.rs:7). */
int fnnue_net_info(const fnnue_net *net, uint32_t *hd, uint32_t *file_hash, const char **desc);
void fnnue_net_free(fnnue_net *net);

/* Deterministic synthetic net in the exact .nnue file format (the pinned net is
 * not shipped with the reference checkout).  flags: FNNUE_SYNTH_*.  The buffer
 * is allocated by the library; release it with fnnue_buffer_free. */
#define FNNUE_SYNTH_LEB128 1u     /* write tensors COMPRESSED_LEB128                  */
#define FNNUE_SYNTH_WRAP 2u       /* large FT weights: int16 accumulators wrap around */
#define FNNUE_SYNTH_FC1_PAD 4u    /* non-zero fc_1 padding weights (inputs 30,31)      */
#define FNNUE_SYNTH_HEAVY 8u      /* a heavy column in every third slice (s % 3 == 1):
                                   * those slices fail the SWAR bound, the others pass */
int fnnue_net_synthesize(uint64_t seed, uint32_t hd, uint32_t flags, void **buf, size_t *len);
void fnnue_buffer_free(void *buf);

/* ---- Fairy-Stockfish variant nets (BASELINE config 5) ----
 * The reference routes every variant to Fairy-Stockfish ([ref]
 * src/queue.rs:530-539, src/assets.rs:384-391) and runs it with its classical
 * eval (`Use NNUE false`, src/stockfish.rs:248-260); these entry points are the
 * NNUE evaluation of such positions with Fairy-Stockfish's variant feature set
 * ("HalfKAv2 variants", 8x8 boards, 64 own-king squares, no mirroring; pocket
 * features for crazyhouse) in front of the SF 15.1 layer stacks.  Recalled,
 * not read: parity unpinned.  Same file format; the feature
 * transformer hash is 0x5F234CB8 ^ 2*HD; widths 256, 512, 1024. */
#define FNNUE_VARIANT_CHESS 0
#define FNNUE_VARIANT_CRAZYHOUSE 1 /* 64 x (704 board + 160 hand) features */
#define FNNUE_VARIANT_ATOMIC 2     /* 64 x 704 board features (also kingofthehill, racingkings, threecheck) */
/* The board-only feature set of atomic with the variant's own rules (no
 * explosions, one king per side always: a position without is
 * FNNUE_E_POSITION).  kingofthehill: chess, over with a king on d4 e4 d5 e5.
 * racingkings: start 8/8/8/8/8/8/krbnNBRK/qrbnNBRQ w - - 0 1, no pawns and no
 * castling rights (such a FEN is FNNUE_E_FEN), no move gives check, over with
 * a king on rank 8 unless black may still catch up.
 * threecheck (ABI 3.8): chess with a counter of remaining checks per colour, 3
 * at the start; a move that leaves the other king attacked takes one off the
 * mover's, and a position with a counter at 0 is over, won by that colour.  The
 * counters travel in the FEN as "3+3" (remaining, white then black) between
 * the en-passant square and the halfmove clock, or as a trailing "+w+b"
 * (checks given); neither: 3+3; both, a digit outside 0..3, a malformed field
 * or both counters 0: FNNUE_E_FEN.  The counters are no part of fnnue_vpos. */
#define FNNUE_VARIANT_KINGOFTHEHILL 3
#define FNNUE_VARIANT_RACINGKINGS 4
#define FNNUE_VARIANT_THREECHECK 5
int fnnue_net_load_variant(const char *path, int variant, fnnue_net **out);
int fnnue_net_load_variant_mem(const void *buf, size_t len, int variant, fnnue_net **out);
int fnnue_net_variant(const fnnue_net *net, int *variant);
/* variant: FNNUE_VARIANT_CRAZYHOUSE .. _RACINGKINGS.  A threecheck net is
 * atomic-format bytes loaded with FNNUE_VARIANT_THREECHECK; that id is
 * FNNUE_E_ARG here, as every id above racingkings has been since ABI 3.2. */
int fnnue_net_synthesize_variant(uint64_t seed, uint32_t hd, int variant, uint32_t flags, void **buf, size_t *len);
/* FEN (crazyhouse holdings as "[PNbq]" after the placement or as a 9th
 * placement field; "~" promotion marks ignored; kingofthehill / racingkings /
 * threecheck: plain chess FENs, holdings and marks refused) -> packed variant position. */
int fnnue_vpos_from_fen(int variant, const char *fen, fnnue_vpos *out);
/* Test inputs: `count` seeded pseudo-legal random walks from the variant's
 * start position (captures go to the capturer's hand and drops come back out
 * for crazyhouse; captures explode for atomic, kings never removed), up to
 * max_plies each.  FNNUE_PLAYOUT_FINAL: the last position of each walk;
 * FNNUE_PLAYOUT_PLIES: every position as CHAIN groups (off[], n_groups + 1). */
int fnnue_random_vpositions(uint64_t seed, int variant, size_t count, uint32_t max_plies, int mode, fnnue_vpos *out,
                            size_t cap, uint32_t *off, size_t off_cap, size_t *n_out, size_t *n_groups);
/* Variant games (the expansion of IncomingBatch::from_acquired for the
 * variants the reference sends to Fairy-Stockfish, [ref] src/queue.rs:524-552,
 * :530-539): crazyhouse FENs with holdings / promoted marks and UCI moves with
 * drops ("P@e4"), atomic captures with explosions, kingofthehill,
 * racingkings and threecheck games (no move after the game's end, no
 * racingkings check, the check counters carried along);
 * every move checked for legality in its variant (shakmaty's Uci::to_move).
 * Host replay: the root and the position after every move (n_moves + 1
 * records). */
int fnnue_game_vpositions(int variant, const char *fen, const char *moves, fnnue_vpos *out, size_t cap,
                          size_t *n_out);
/* Same plus every legal 1-ply child (drops included) of each position, as STAR
 * groups (off has n_groups + 1 entries). */
int fnnue_game_vchildren(int variant, const char *fen, const char *moves, fnnue_vpos *out, size_t cap, uint32_t *off,
                         size_t off_cap, size_t *n_out, size_t *n_groups);
/* perft of the variant move generator (known answers pin it). */
int fnnue_vperft(int variant, const char *fen, int depth, uint64_t *nodes);
/* Up to `plies` uniformly random legal moves (drops included) from `fen`, as
 * space-separated UCI; stops when no move is left (mate, stalemate, the
 * variant's end of the game) or a king exploded. */
int fnnue_random_vgame(uint64_t seed, int variant, const char *fen, uint32_t plies, char *moves, size_t cap,
                       size_t *len);
/* Test / bench inputs: every ply of `count` seeded random LEGAL games of the
 * variant from its start position (L ~ U[0, max_plies] plies, drops included),
 * as CHAIN groups; a game ends early with no legal move or an exploded king
 * (that position is the game's last: see fnnue_eval_vpositions on game-over
 * records).  Deterministic for (seed, index). */
int fnnue_random_vgames(uint64_t seed, int variant, size_t count, uint32_t max_plies, int threads, fnnue_vpos *out,
                        size_t cap, uint32_t *off, size_t off_cap, size_t *n_out, size_t *n_groups);
/* The batch expansion on the device, as fnnue_build_batch[_device] (same text
 * layout, modes FNNUE_PLAYOUT_PLIES / _CHILDREN, sizes reported on
 * FNNUE_E_CAPACITY), for variant games; records are those of the host replay.
 * ctx supplies the device and stream (any net). */
int fnnue_build_vbatch_device(fnnue_ctx *ctx, int variant, const char *d_text, const uint32_t *d_fen_off,
                              const uint32_t *d_moves_off, size_t ngames, int mode, fnnue_vpos *d_out, size_t cap,
                              uint32_t *d_off, size_t off_cap, size_t *n_out, size_t *n_groups, void *stream);
int fnnue_build_vbatch(fnnue_ctx *ctx, int variant, const char *text, size_t text_len, const uint32_t *fen_off,
                       const uint32_t *moves_off, size_t ngames, int mode, fnnue_vpos *out, size_t cap, uint32_t *off,
                       size_t off_cap, size_t *n_out, size_t *n_groups);
/* Evaluation of variant positions on a context created from a variant net
 * (fnnue_ctx_create / fnnue_multi_create): the LDS-stationary feature
 * transformer over the variant tiles, then the MFMA layer stacks.
 * Game-over records: an atomic position with exactly one king (the other
 * exploded — how atomic games end, and every child that captures next to the
 * enemy king) has no NNUE evaluation; its result is psqt = positional = 0 and
 * it is not an error (the game's result is the caller's: fnnue_game_end,
 * the backend's mate 0).  Any other position without one king per side fails
 * the call with FNNUE_E_POSITION, the message naming its index. */
int fnnue_eval_vpositions(fnnue_ctx *ctx, const fnnue_vpos *pos, size_t n, int32_t *psqt, int32_t *positional);
int fnnue_eval_vpositions_device(fnnue_ctx *ctx, const fnnue_vpos *d_pos, size_t n, int32_t *d_psqt,
                                 int32_t *d_positional, void *stream);
/* Grouped variant evaluation with accumulator reuse, as fnnue_eval_groups[_device]
 * (FNNUE_GROUP_CHAIN: a game's plies, e.g. fnnue_build_vbatch's output;
 * FNNUE_GROUP_STAR: a parent and its children): each accumulator is derived
 * from the previous ply's / the parent's by the changed board and pocket
 * features (a crazyhouse capture adds the captured piece's hand row, a drop
 * removes one), refreshed when the perspective's king moved or more than two
 * features left or entered (atomic explosions).  Results are identical to
 * fnnue_eval_vpositions on the same positions. */
int fnnue_eval_vgroups(fnnue_ctx *ctx, const fnnue_vpos *pos, size_t npos, const uint32_t *off, size_t ngroups,
                       int mode, int32_t *psqt, int32_t *positional);
int fnnue_eval_vgroups_device(fnnue_ctx *ctx, const fnnue_vpos *d_pos, const uint32_t *d_off, size_t ngroups,
                              size_t npos, int mode, int32_t *d_psqt, int32_t *d_positional, void *stream);

/* ---- device context ----
 * Replaces spawning + initialising an engine process ([ref] src/stockfish.rs:
 * 132-153 spawn, 203-233 init).  Uploads the net to `device` (HIP ordinal). */
int fnnue_device_count(int *count);
int fnnue_ctx_create(const fnnue_net *net, int device, fnnue_ctx **out);
/* Device image of a net: one contiguous buffer, so rank 0 can RCCL-broadcast it
 * over xGMI and the other ranks adopt it (copied into ctx-owned memory). */
int fnnue_net_image_size(const fnnue_net *net, size_t *bytes);
int fnnue_net_image_pack(const fnnue_net *net, void *host_buf, size_t bytes);
int fnnue_ctx_create_from_image(int device, uint32_t hd, const void *device_image, size_t bytes, fnnue_ctx **out);
/* Pointer to the ctx's own device image (for broadcasting from rank 0). */
int fnnue_ctx_image(fnnue_ctx *ctx, const void **device_image, size_t *bytes);
void fnnue_ctx_free(fnnue_ctx *ctx);

/* ---- several GPUs from one process ----
 * The reference runs one engine per core ([ref] src/main.rs:156-170,
 * src/configure.rs:196-206: Cores::All = available_parallelism).  A
 * fnnue_multi owns one context per listed device: the net is uploaded once to
 * devices[0] and RCCL-broadcast over xGMI (ncclCommInitAll, one communicator
 * per device, this process); batches are sharded with no data-path
 * collective — contiguous position ranges, or whole groups balanced by
 * position count (fnnue_partition_groups) — and each device's results land in
 * its disjoint slice of the caller's buffers.  Same results as one context. */
typedef struct fnnue_multi fnnue_multi;
int fnnue_multi_create(const fnnue_net *net, const int *devices, int ndev, fnnue_multi **out);
/* Several contexts, each with its own stream, workspace and staging, possibly
 * on one GPU (ABI 3.9): as fnnue_multi_create, except that an ordinal may
 * repeat and no RCCL communicator is made — the image is packed once on the
 * host and copied to every context.  Everything after creation is the same
 * fnnue_multi: the same sharding, host threads, streams and error reports, so
 * this is also how the sharding path is tested on a one-GPU box
 * (devices = {0, 0, 0}).  Contexts that share a GPU share its time: no
 * speed-up is implied. */
int fnnue_multi_create_replicas(const fnnue_net *net, const int *devices, int ndev, fnnue_multi **out);
void fnnue_multi_free(fnnue_multi *m);
int fnnue_multi_size(const fnnue_multi *m, int *ndev);
/* The context of device i (borrowed; owned by m). */
int fnnue_multi_ctx(fnnue_multi *m, int i, fnnue_ctx **ctx);
/* Host buffers, synchronous: one host thread per device (H2D, eval, D2H).
 * An error is the first failing shard's, its message prefixed with
 * "shard i (device d): " (i: the context's place in the multi); an invalid
 * position is named by its index in the caller's buffer, e.g.
 * "shard 2 (device 0): invalid position at index 2041".  The device-buffer
 * calls and fnnue_multi_sync use the same prefix. */
int fnnue_multi_eval_positions(fnnue_multi *m, const fnnue_pos *pos, size_t n, int32_t *psqt, int32_t *positional);
int fnnue_multi_eval_groups(fnnue_multi *m, const fnnue_pos *pos, size_t npos, const uint32_t *off, size_t ngroups,
                            int mode, int32_t *psqt, int32_t *positional);
/* Device buffers: arrays of one pointer / count per device (device i's
 * buffers live on device i); device i's work is enqueued on streams[i] (a
 * hipStream_t of device i, as void*) or, when `streams` or streams[i] is NULL,
 * on its context's own stream, so the caller can order it after the work that
 * wrote the inputs (or synchronise first).  Returns without synchronising the
 * host, at any batch size.  fnnue_multi_sync waits for every device's
 * context work and reports latched errors (as fnnue_ctx_check). */
int fnnue_multi_eval_positions_device(fnnue_multi *m, const fnnue_pos *const *d_pos, const size_t *n,
                                      int32_t *const *d_psqt, int32_t *const *d_positional, void *const *streams);
int fnnue_multi_eval_groups_device(fnnue_multi *m, const fnnue_pos *const *d_pos, const uint32_t *const *d_off,
                                   const size_t *ngroups, const size_t *npos, int mode, int32_t *const *d_psqt,
                                   int32_t *const *d_positional, void *const *streams);
int fnnue_multi_sync(fnnue_multi *m);
/* Fairy-Stockfish variant positions over every device of a multi built from a
 * variant net (BASELINE config 5 on 8 GPUs): contiguous shards, as
 * fnnue_multi_eval_positions[_device]. */
int fnnue_multi_eval_vpositions(fnnue_multi *m, const fnnue_vpos *pos, size_t n, int32_t *psqt, int32_t *positional);
int fnnue_multi_eval_vpositions_device(fnnue_multi *m, const fnnue_vpos *const *d_pos, const size_t *n,
                                       int32_t *const *d_psqt, int32_t *const *d_positional, void *const *streams);
/* Grouped variant positions on every device (fnnue_eval_vgroups_device per
 * device, one shard of whole games each), as fnnue_multi_eval_groups_device. */
int fnnue_multi_eval_vgroups_device(fnnue_multi *m, const fnnue_vpos *const *d_pos, const uint32_t *const *d_off,
                                    const size_t *ngroups, const size_t *npos, int mode, int32_t *const *d_psqt,
                                    int32_t *const *d_positional, void *const *streams);
/* Splits groups off[0..ngroups] into nparts contiguous runs of whole groups
 * with about equal position counts: part k = groups [cut[k], cut[k+1]),
 * cut has nparts + 1 entries.  Host only. */
int fnnue_partition_groups(const uint32_t *off, size_t ngroups, int nparts, uint32_t *cut);

/* ---- evaluation, host buffers (synchronous) ----
 * Copies in, runs the device path, copies out.  Position validity is checked
 * on the device; an invalid position fails the whole call with
 * FNNUE_E_POSITION (message: its index) and no outputs are guaranteed.
 * Static eval of independent positions, accumulators from scratch.  Replaces
 * one `position fen ... ` + eval round trip per position ([ref]
 * src/stockfish.rs:274-283 / StockfishStub::go :44-54) with one batched call. */
int fnnue_eval_positions(fnnue_ctx *ctx, const fnnue_pos *pos, size_t n, int32_t *psqt, int32_t *positional);

/* Grouped evaluation with accumulator reuse.  Group g is pos[off[g] .. off[g+1]).
 *  FNNUE_GROUP_CHAIN: a game's plies in order; each accumulator is derived
 *    from the previous ply's (incremental add/sub of changed features, refresh
 *    on own-king moves) — upstream update_accumulator along the StateInfo chain.
 *    Feed it the expansion of an analysis batch ([ref] src/queue.rs:571-600).
 *  FNNUE_GROUP_STAR: pos[off[g]] is a parent, the rest are its children; each
 *    child is derived from the parent's accumulator.
 * Results are identical to fnnue_eval_positions on the same positions. */
#define FNNUE_GROUP_CHAIN 0
#define FNNUE_GROUP_STAR 1
/* pos holds npos positions; off has ngroups + 1 entries, off[0] = 0,
 * non-decreasing, off[ngroups] = npos (else FNNUE_E_ARG, nothing read past
 * pos[npos - 1]). */
int fnnue_eval_groups(fnnue_ctx *ctx, const fnnue_pos *pos, size_t npos, const uint32_t *off, size_t ngroups,
                      int mode, int32_t *psqt, int32_t *positional);

/* ---- evaluation, device buffers (asynchronous on `stream`, a hipStream_t) ----
 * Inputs already resident in HBM; results written to device memory.  Position
 * validity errors are latched on the device: call fnnue_ctx_check() after
 * synchronising to turn them into FNNUE_E_POSITION. */
int fnnue_eval_positions_device(fnnue_ctx *ctx, const fnnue_pos *d_pos, size_t n, int32_t *d_psqt,
                                int32_t *d_positional, void *stream);
int fnnue_eval_groups_device(fnnue_ctx *ctx, const fnnue_pos *d_pos, const uint32_t *d_off, size_t ngroups,
                             size_t npos, int mode, int32_t *d_psqt, int32_t *d_positional, void *stream);
/* Big + small net over the same CHAIN / STAR batch (BASELINE config 3 "big +
 * small net"; later Stockfish's dual NNUE evaluates a small HalfKAv2_hm net
 * beside the big one on the same features): results identical to two
 * fnnue_eval_groups_device calls, but the plan (deltas, segments, feature
 * lists) is built once, in the big context's workspace, and the small net's
 * feature transformer and layer stacks run on the small context's stream
 * beside the big net's on `stream`.  Both contexts: chess nets on one device,
 * sliced feature transformer.  No host synchronisation. */
int fnnue_eval_groups_dual_device(fnnue_ctx *big, fnnue_ctx *small, const fnnue_pos *d_pos, const uint32_t *d_off,
                                  size_t ngroups, size_t npos, int mode, int32_t *d_psqt, int32_t *d_positional,
                                  int32_t *d_psqt_small, int32_t *d_positional_small, void *stream);
/* Synchronises the ctx's device and reports (and clears) latched errors. */
int fnnue_ctx_check(fnnue_ctx *ctx);

/* ---- batch building (host) ----
 * FEN -> packed position.  Accepts standard, X-FEN and Shredder-FEN castling. */
int fnnue_pos_from_fen(const char *fen, fnnue_pos *out);
/* Every position of a game: the root and the position after each move, i.e.
 * the expansion of IncomingBatch::from_acquired for an analysis batch
 * ([ref] src/queue.rs:543-600; moves checked for legality like
 * Uci::to_move, :545).  `moves` is space-separated UCI (standard or Chess960
 * castling).  Writes n_moves + 1 positions. */
int fnnue_game_positions(const char *fen, const char *moves, fnnue_pos *out, size_t cap, size_t *n_out);
/* Same, plus every legal 1-ply child of each position, as STAR groups:
 * out[off[g]] is ply g, followed by its children.  off has n_groups+1 entries. */
int fnnue_game_children(const char *fen, const char *moves, fnnue_pos *out, size_t cap, uint32_t *off,
                        size_t off_cap, size_t *n_out, size_t *n_groups);
/* Has the game ended on the board after `moves`?  *flags = FNNUE_END_*: no
 * legal move, the side to move's king attacked, its king exploded (atomic),
 * the side to move has lost by the variant's own rule (kingofthehill: the
 * other king on the hill; racingkings: one king on rank 8 — the racingkings
 * draw with both kings there is FNNUE_END_NO_MOVES alone; threecheck: a check
 * counter at 0 — the mover's after its last check, so with FNNUE_END_CHECK; a
 * root FEN whose side to move's own counter is 0 is over the same way, won).
 * A position without a legal move is where the engine answers `score mate 0`
 * (checkmate / explosion / variant loss) or `score cp 0` (stalemate, draw) with `bestmove (none)`
 * ([ref] src/stockfish.rs:359-376).  variant: FNNUE_VARIANT_* (host replay). */
#define FNNUE_END_NO_MOVES 1
#define FNNUE_END_CHECK 2
#define FNNUE_END_EXTINCT 4
#define FNNUE_END_VARIANT 8
/* Only on a child record of fnnue_build_vchildren (never from fnnue_game_end):
 * the child's side to move has already won by the variant's rule (racingkings:
 * the mover failed to catch up), so the parent's mover lost by playing it. */
#define FNNUE_END_WON 0x40
/* (FNNUE_END_DRAW, 0x10: only on a searched record, set by the searches' draw
 * rules, ABI 3.12 below; never from fnnue_game_end or a builder.) */
int fnnue_game_end(int variant, const char *fen, const char *moves, int *flags);
/* Seeded random playouts from the start position (splitmix64; L ~ U[min,max]
 * plies of uniformly random legal moves, stopping at mate, stalemate or the
 * 50-move rule).  Deterministic for a given (seed, index) regardless of threads.
 *  FNNUE_PLAYOUT_FINAL: out[i] = final position of playout i (n_out = count).
 *  FNNUE_PLAYOUT_PLIES: every ply of every playout as CHAIN groups.
 *  FNNUE_PLAYOUT_CHILDREN: every ply and its legal children as STAR groups.
 * For the grouped modes off[] receives group offsets (off_cap >= groups+1). */
#define FNNUE_PLAYOUT_FINAL 0
#define FNNUE_PLAYOUT_PLIES 1
#define FNNUE_PLAYOUT_CHILDREN 2
int fnnue_random_playouts(uint64_t seed, size_t count, uint32_t min_plies, uint32_t max_plies, int mode,
                          int threads, fnnue_pos *out, size_t cap, uint32_t *off, size_t off_cap, size_t *n_out,
                          size_t *n_groups);
/* perft node count (board-code self test against published known answers). */
int fnnue_perft(const char *fen, int depth, uint64_t *nodes);

/* ---- batch building on the device ----
 * The batch expansion of fnnue_game_positions / fnnue_game_children for a
 * whole batch at once, on the GPU (FEN parse, UCI replay with Chess960
 * castling / en passant / promotion, legal children): replaces the
 * per-game host loop of IncomingBatch::from_acquired ([ref] src/queue.rs:
 * 518-627; wire format src/api.rs:293-309) and produces the positions where
 * the evaluator reads them.  Results are record for record those of the host
 * builder.
 * d_text (device memory): game g's FEN in [fen_off[g], moves_off[g]) and its
 * space-separated UCI moves in [moves_off[g], fen_off[g + 1]); d_fen_off has
 * ngames + 1 entries, d_moves_off ngames (both device memory).
 *  FNNUE_PLAYOUT_PLIES: every ply of every game; group g = game g (CHAIN).
 *  FNNUE_PLAYOUT_CHILDREN: one STAR group per ply: the ply, then its legal
 *    children in generation order.
 * Synchronous on `stream` (sizes are read back).  *n_out / *n_groups are set
 * even when the call fails with FNNUE_E_CAPACITY (retry with bigger buffers);
 * FNNUE_E_FEN / FNNUE_E_MOVE name the first failing game and ply. */
int fnnue_build_batch_device(fnnue_ctx *ctx, const char *d_text, const uint32_t *d_fen_off,
                             const uint32_t *d_moves_off, size_t ngames, int mode, fnnue_pos *d_out, size_t cap,
                             uint32_t *d_off, size_t off_cap, size_t *n_out, size_t *n_groups, void *stream);
/* Same with host buffers (staged through the ctx's stream). */
int fnnue_build_batch(fnnue_ctx *ctx, const char *text, size_t text_len, const uint32_t *fen_off,
                      const uint32_t *moves_off, size_t ngames, int mode, fnnue_pos *out, size_t cap, uint32_t *off,
                      size_t off_cap, size_t *n_out, size_t *n_groups);
/* perft on the device (depth <= 3 per thread; shallower levels expanded on
 * the host): pins the device move generator on published counts. */
int fnnue_perft_device(fnnue_ctx *ctx, const char *fen, int depth, uint64_t *nodes);
/* A random legal game from `fen`: up to `plies` uniformly random legal moves
 * (splitmix64 seed), space-separated UCI (Chess960 notation when the position
 * needs it), NUL-terminated; *len = string length.  Test-input generator. */
int fnnue_random_game(uint64_t seed, const char *fen, uint32_t plies, char *moves, size_t cap, size_t *len);

/* ---- one-ply search on the device (ABI 3.4) ----
 * What a search over a position's children needs beyond their records: the
 * move that leads to each child and whether the child is checkmated or
 * stalemated; then, per STAR group, the best child.  These entry points are
 * for chess nets (standard, chess960, fromPosition); the Fairy-Stockfish
 * variants have their own below (ABI 3.6: fnnue_build_vchildren,
 * fnnue_vsearch1), whose end-flag bytes also carry FNNUE_END_EXTINCT /
 * FNNUE_END_VARIANT and, on a child, FNNUE_END_WON.
 *
 * A move code: from | to << 6 | promo << 12 (squares A1 = 0 .. H8 = 63; promo 0
 * or the piece type 2..5 = n b r q).  Castling carries the squares the game's
 * notation spells: the king's destination, or the rook's square when the game
 * needs Chess960 notation, so the code prints without its board.  0: no move. */
typedef uint16_t fnnue_move;
/* "e2e4", "e7e8q" (NUL-terminated, at most 6 bytes); the code 0 prints as "".
 * FNNUE_E_ARG for promo 1, 6 or 7 or a set bit 15.  Host only. */
int fnnue_move_uci(fnnue_move m, char out[8]);
/* fnnue_build_batch[_device] in FNNUE_PLAYOUT_CHILDREN mode (records and
 * offsets byte for byte, same capacity protocol, same errors) plus two arrays
 * parallel to the records (cap entries each): moves[r] the move that leads to
 * record r (0 for a ply's own record), end[r] the FNNUE_END_NO_MOVES /
 * FNNUE_END_CHECK flags of record r itself, plies and children alike. */
int fnnue_build_children_device(fnnue_ctx *ctx, const char *d_text, const uint32_t *d_fen_off,
                                const uint32_t *d_moves_off, size_t ngames, fnnue_pos *d_out, size_t cap,
                                uint32_t *d_off, size_t off_cap, fnnue_move *d_moves, uint8_t *d_end, size_t *n_out,
                                size_t *n_groups, void *stream);
int fnnue_build_children(fnnue_ctx *ctx, const char *text, size_t text_len, const uint32_t *fen_off,
                         const uint32_t *moves_off, size_t ngames, fnnue_pos *out, size_t cap, uint32_t *off,
                         size_t off_cap, fnnue_move *moves, uint8_t *end, size_t *n_out, size_t *n_groups);
/* The best child of a STAR group [off[g], off[g + 1]) (its first record is the
 * parent), by the rule of the backend's move work: a child with NO_MOVES and
 * any of CHECK | EXTINCT | VARIANT is a mate in one and beats everything; a
 * child with NO_MOVES alone is worth 0; any other child
 * -(((int64)psqt + positional) / 16) (C truncation); a child with
 * FNNUE_END_WON (whatever its other bits) ranks below all of these, worth 0:
 * it is chosen only when every child has it.  The first maximum (the lowest
 * index) wins.  An empty group gives an all-zero record.  (End bytes that use
 * bits 0 and 1 only — every chess record — rank as they did before ABI 3.6.) */
#define FNNUE_BEST_NONE 0 /* no child: `end` says mate 0 (NO_MOVES and a deciding flag) or cp 0 */
#define FNNUE_BEST_CP 1
#define FNNUE_BEST_MATE 2 /* mate in 1 */
#define FNNUE_BEST_LOST 3 /* every move loses at once (FNNUE_END_WON children only): mate -1 */
typedef struct {
  int32_t psqt, positional; /* of the best child, negated (as move work reports them); 0 when none */
  int32_t value;            /* Stockfish internal units, side to move of the parent; 0 for mate / lost / none */
  uint32_t nodes;           /* children */
  uint32_t best;            /* index of the best child within the group (1-based record index), 0 when none */
  fnnue_move move;          /* 0 when none (or without a moves array) */
  uint8_t kind;             /* FNNUE_BEST_* */
  uint8_t end;              /* the parent's FNNUE_END_* flags */
} fnnue_best;
/* The reduction alone, one kernel on `stream` (no atomics, no host
 * synchronisation): psqt / positional / end (and moves, which may be NULL)
 * hold npos entries, off ngroups + 1 (offsets beyond npos are clamped), out
 * ngroups records.  Any net. */
int fnnue_best_children_device(fnnue_ctx *ctx, const int32_t *d_psqt, const int32_t *d_positional,
                               const uint8_t *d_end, const fnnue_move *d_moves, const uint32_t *d_off,
                               size_t ngroups, size_t npos, fnnue_best *d_out, void *stream);
int fnnue_best_children(fnnue_ctx *ctx, const int32_t *psqt, const int32_t *positional, const uint8_t *end,
                        const fnnue_move *moves, const uint32_t *off, size_t ngroups, size_t npos, fnnue_best *out);
/* Depth 1 for every ply of every game (text in the builder's layout): the
 * children expansion, their STAR evaluation and the reduction, in the
 * context's grow-only scratch.  out: one record per ply (cap records), off:
 * CHAIN offsets per game (ngames + 1 entries); *n_out = plies, *n_groups =
 * games, set also with FNNUE_E_CAPACITY (before any ply is expanded).  The
 * builder's sizing read-backs synchronise `stream`; the evaluation and the
 * reduction are enqueued behind them (fnnue_ctx_check reports a position the
 * evaluator rejects).  A chess net's context; FNNUE_E_ARCH otherwise. */
int fnnue_search1_device(fnnue_ctx *ctx, const char *d_text, const uint32_t *d_fen_off, const uint32_t *d_moves_off,
                         size_t ngames, fnnue_best *d_out, size_t cap, uint32_t *d_off, size_t off_cap,
                         size_t *n_out, size_t *n_groups, void *stream);
int fnnue_search1(fnnue_ctx *ctx, const char *text, size_t text_len, const uint32_t *fen_off,
                  const uint32_t *moves_off, size_t ngames, fnnue_best *out, size_t cap, uint32_t *off,
                  size_t off_cap, size_t *n_out, size_t *n_groups);

/* ---- MultiPV at depth 1: the k best children of a group (ABI 3.5) ----
 * fnnue_best_children's rule extended to a total order: the mates in one
 * first, in index order; then the children by value (a stalemating child worth
 * 0), descending; equal values by lower index; then the FNNUE_END_WON children
 * (kind FNNUE_BEST_LOST), in index order.  A chess ply has at most
 * FNNUE_MAX_CHILDREN children. */
#define FNNUE_MAX_CHILDREN 218
typedef struct {
  int32_t psqt, positional; /* of this child, negated with wrap-around, as fnnue_best reports them */
  int32_t value;            /* internal units, parent's side to move; 0 for a mate */
  uint32_t child;           /* 1-based record index within the group */
  fnnue_move move;          /* 0 without a moves array */
  uint8_t kind;             /* FNNUE_BEST_CP / _MATE / _LOST; FNNUE_BEST_NONE = unused slot (all zero) */
  uint8_t reserved;         /* 0 */
} fnnue_line;
/* Group g owns the slots [line_off[g], line_off[g + 1]) of `lines` (line_off:
 * ngroups + 1 entries, non-decreasing; the slot count is the group's k and may
 * differ from group to group).  Slot j receives the j-th child in the order
 * above; slots beyond the group's children are written all-zero; a group
 * without a slot, or an empty group, writes nothing.  Slot 0 equals the
 * group's fnnue_best field by field (psqt, positional, value, best == child,
 * move, kind).  The other arrays, the clamping of offsets beyond npos and the
 * launch (one kernel on `stream`, no atomics, no host synchronisation) are
 * fnnue_best_children_device's.  Any net.  The device form never writes at or
 * beyond lines_cap; the host form refuses line_off[ngroups] > lines_cap with
 * FNNUE_E_CAPACITY. */
int fnnue_topk_children_device(fnnue_ctx *ctx, const int32_t *d_psqt, const int32_t *d_positional,
                               const uint8_t *d_end, const fnnue_move *d_moves, const uint32_t *d_off,
                               size_t ngroups, size_t npos, const uint32_t *d_line_off, fnnue_line *d_lines,
                               size_t lines_cap, void *stream);
int fnnue_topk_children(fnnue_ctx *ctx, const int32_t *psqt, const int32_t *positional, const uint8_t *end,
                        const fnnue_move *moves, const uint32_t *off, size_t ngroups, size_t npos,
                        const uint32_t *line_off, fnnue_line *lines, size_t lines_cap);
/* fnnue_search1[_device] plus, per ply, its k best children: ply p's k slots
 * are lines[p * k .. p * k + k) (k in 1..FNNUE_MAX_CHILDREN, anything else
 * FNNUE_E_ARG).  The fnnue_best records and the CHAIN offsets are those of
 * fnnue_search1; same steps, same scratch, same capacity protocol, and
 * lines_cap < plies * k is FNNUE_E_CAPACITY too (before any ply is expanded,
 * *n_out set).  A chess net's context; FNNUE_E_ARCH otherwise. */
int fnnue_search1_lines_device(fnnue_ctx *ctx, const char *d_text, const uint32_t *d_fen_off,
                               const uint32_t *d_moves_off, size_t ngames, uint32_t k, fnnue_best *d_out, size_t cap,
                               uint32_t *d_off, size_t off_cap, fnnue_line *d_lines, size_t lines_cap, size_t *n_out,
                               size_t *n_groups, void *stream);
int fnnue_search1_lines(fnnue_ctx *ctx, const char *text, size_t text_len, const uint32_t *fen_off,
                        const uint32_t *moves_off, size_t ngames, uint32_t k, fnnue_best *out, size_t cap,
                        uint32_t *off, size_t off_cap, fnnue_line *lines, size_t lines_cap, size_t *n_out,
                        size_t *n_groups);

/* ---- one-ply search for the Fairy-Stockfish variants (ABI 3.6) ----
 * crazyhouse, atomic, kingofthehill, racingkings and threecheck, on a variant
 * net's context.
 *
 * A variant move code is a fnnue_move that can also spell a drop: from == to
 * (the drop square) with the promo field holding the dropped piece type 1..5
 * (P N B R Q), printed "N@f3".  A promotion is never from == to, so the two
 * forms cannot collide; every other move is encoded as for chess (castling:
 * the king's two-square step, or king-takes-rook when the game needs Chess960
 * notation).  FNNUE_E_ARG for from == to with promo 0, for promo 6 or 7, for
 * promo 1 with from != to, and for a set bit 15.  Host only. */
int fnnue_vmove_uci(fnnue_move m, char out[8]);
/* fnnue_build_vbatch[_device] in FNNUE_PLAYOUT_CHILDREN mode (records and
 * offsets byte for byte, same capacity protocol, same errors) plus moves[r],
 * the variant move code that leads to record r (0 for a ply's own record), and
 * end[r], record r's own FNNUE_END_NO_MOVES | CHECK | EXTINCT | VARIANT flags
 * under the variant's rules (as fnnue_game_end computes them); a child also
 * carries FNNUE_END_WON when its side to move has already won. */
int fnnue_build_vchildren_device(fnnue_ctx *ctx, int variant, const char *d_text, const uint32_t *d_fen_off,
                                 const uint32_t *d_moves_off, size_t ngames, fnnue_vpos *d_out, size_t cap,
                                 uint32_t *d_off, size_t off_cap, fnnue_move *d_moves, uint8_t *d_end, size_t *n_out,
                                 size_t *n_groups, void *stream);
int fnnue_build_vchildren(fnnue_ctx *ctx, int variant, const char *text, size_t text_len, const uint32_t *fen_off,
                          const uint32_t *moves_off, size_t ngames, fnnue_vpos *out, size_t cap, uint32_t *off,
                          size_t off_cap, fnnue_move *moves, uint8_t *end, size_t *n_out, size_t *n_groups);
/* fnnue_search1[_lines][_device] for a variant net's context: the same three
 * steps (fnnue_build_vchildren, fnnue_eval_vgroups STAR, the reduction) in the
 * context's scratch, the same capacity protocol.  `variant` must be one the
 * context's net evaluates (its own; an atomic net also kingofthehill,
 * racingkings and threecheck): FNNUE_E_ARCH otherwise, and on a chess context.  A crazyhouse
 * ply may have more than FNNUE_MAX_CHILDREN children; k stays 1..218. */
int fnnue_vsearch1_device(fnnue_ctx *ctx, int variant, const char *d_text, const uint32_t *d_fen_off,
                          const uint32_t *d_moves_off, size_t ngames, fnnue_best *d_out, size_t cap, uint32_t *d_off,
                          size_t off_cap, size_t *n_out, size_t *n_groups, void *stream);
int fnnue_vsearch1(fnnue_ctx *ctx, int variant, const char *text, size_t text_len, const uint32_t *fen_off,
                   const uint32_t *moves_off, size_t ngames, fnnue_best *out, size_t cap, uint32_t *off,
                   size_t off_cap, size_t *n_out, size_t *n_groups);
int fnnue_vsearch1_lines_device(fnnue_ctx *ctx, int variant, const char *d_text, const uint32_t *d_fen_off,
                                const uint32_t *d_moves_off, size_t ngames, uint32_t k, fnnue_best *d_out, size_t cap,
                                uint32_t *d_off, size_t off_cap, fnnue_line *d_lines, size_t lines_cap, size_t *n_out,
                                size_t *n_groups, void *stream);
int fnnue_vsearch1_lines(fnnue_ctx *ctx, int variant, const char *text, size_t text_len, const uint32_t *fen_off,
                         const uint32_t *moves_off, size_t ngames, uint32_t k, fnnue_best *out, size_t cap,
                         uint32_t *off, size_t off_cap, fnnue_line *lines, size_t lines_cap, size_t *n_out,
                         size_t *n_groups);

/* ---- two-ply search on the device (ABI 3.7) ----
 * Full-width minimax over two plies, chess nets only.  For a ply P with the
 * children c = 1..n in generation order, b_c is child c's own depth-1 record:
 * fnnue_best_children's result for the STAR group (child c, its children).
 * The key of child c, from P's side to move:
 *   end[c] has NO_MOVES and a deciding flag (CHECK): mate in one   rank 3             pv c
 *   end[c] has NO_MOVES alone: a stalemating move                  rank 2, value 0    pv c
 *   b_c.kind == FNNUE_BEST_MATE: the reply mates                   rank 1             pv c, reply
 *   otherwise                                                      rank 2, -b_c.value pv c, reply
 * The higher rank wins, then the higher value, then the lower child index (the
 * first maximum, as at depth 1).  A ply without a legal move is
 * FNNUE_BEST_NONE with its own end flags. */
#define FNNUE_BEST_MATED 4 /* every move allows a mate in one: Score::Mate(-1) */
typedef struct {
  int32_t psqt, positional; /* of the pv's last position, from P's side to move: a two-move pv -> the
                               grandchild's terms as they are; a one-move pv -> the child's, negated with
                               wrap-around (as fnnue_best); 0 when none */
  int32_t value;            /* FNNUE_BEST_CP only, else 0 */
  uint32_t nodes;           /* children + all grandchildren of P */
  uint32_t best;            /* 1-based index of the child in P's group; 0 when none */
  uint32_t reply_index;     /* 1-based index of the reply in the child's group; 0 when the pv has one move */
  fnnue_move move, reply;   /* reply 0 when the pv has one move */
  uint8_t kind;             /* FNNUE_BEST_NONE / _CP / _MATE / _MATED */
  uint8_t end;              /* P's own end flags */
  uint8_t pv_len;           /* 0, 1 or 2 */
  uint8_t reserved;         /* 0 */
} fnnue_best2;
/* The second reduction alone (no atomics, no host synchronisation): end / moves
 * (moves may be NULL) hold npos entries and off ngroups + 1, as for
 * fnnue_best_children (offsets beyond npos are clamped; an empty group gives an
 * all-zero record).  child_best holds one fnnue_best per child record, dense,
 * in record order: the children of the first group with any, then the next
 * group's (npos less the non-empty groups, after clamping).  The entry of a
 * child without a legal move is read for its psqt / positional only, taken as
 * the child's own terms from its own side to move (fnnue_search2 stores them
 * there); the record negates them.  nodes = the group's children + the sum of
 * their entries' nodes.  End bytes are read as chess end bytes (bits 0, 1).
 * Any net. */
int fnnue_best_replies_device(fnnue_ctx *ctx, const uint8_t *d_end, const fnnue_move *d_moves, const uint32_t *d_off,
                              size_t ngroups, size_t npos, const fnnue_best *d_child_best, fnnue_best2 *d_out,
                              void *stream);
int fnnue_best_replies(fnnue_ctx *ctx, const uint8_t *end, const fnnue_move *moves, const uint32_t *off,
                       size_t ngroups, size_t npos, const fnnue_best *child_best, fnnue_best2 *out);
/* Depth 2 for every ply of every game: fnnue_search1's signature, capacity
 * protocol (*n_out = plies, *n_groups = games, set also with
 * FNNUE_E_CAPACITY, before anything is expanded) and errors.  The plies are
 * walked in chunks, cut at ply boundaries so that a chunk's grandchild records
 * stay within FNNUE_SEARCH2_RECORDS (environment; default 16M, never below one
 * ply's maximum of 219 * 219); the results do not depend on it.  The children's
 * boards and depth-1 records (112 bytes per child) are held for the whole
 * call.  Host waits: the builder's sizing read-backs and one for the chunk cuts.
 * A chess net's context; FNNUE_E_ARCH otherwise. */
int fnnue_search2_device(fnnue_ctx *ctx, const char *d_text, const uint32_t *d_fen_off, const uint32_t *d_moves_off,
                         size_t ngames, fnnue_best2 *d_out, size_t cap, uint32_t *d_off, size_t off_cap,
                         size_t *n_out, size_t *n_groups, void *stream);
int fnnue_search2(fnnue_ctx *ctx, const char *text, size_t text_len, const uint32_t *fen_off,
                  const uint32_t *moves_off, size_t ngames, fnnue_best2 *out, size_t cap, uint32_t *off,
                  size_t off_cap, size_t *n_out, size_t *n_groups);
/* fnnue_search2 plus the children's depth-1 records it reduced: child_best[d]
 * and child_map[d] = (ply, 1-based child index) for every child of every ply,
 * in record order (child_cap entries each; *n_children is set also with
 * FNNUE_E_CAPACITY).  For tests and tools. */
int fnnue_search2_children(fnnue_ctx *ctx, const char *text, size_t text_len, const uint32_t *fen_off,
                           const uint32_t *moves_off, size_t ngames, fnnue_best2 *out, size_t cap, uint32_t *off,
                           size_t off_cap, fnnue_best *child_best, uint32_t *child_map, size_t child_cap,
                           size_t *n_out, size_t *n_groups, size_t *n_children);

/* ---- two-ply search for the Fairy-Stockfish variants (ABI 3.10) ----
 * The rule of ABI 3.7 with the variants' ranks.  f_c is child c's end byte as
 * fnnue_build_vchildren writes it, b_c child c's own depth-1 record
 * (fnnue_best_children under the ABI 3.6 ranks).  The key of child c from P's
 * side to move, the conditions tested in this order:
 *   f_c has FNNUE_END_WON, whatever else is set          rank 0, value 0   FNNUE_BEST_LOST   pv c
 *   f_c has NO_MOVES and CHECK, EXTINCT or VARIANT       rank 4            FNNUE_BEST_MATE   pv c
 *   f_c has NO_MOVES alone (stalemate, racingkings draw) rank 2, value 0   FNNUE_BEST_CP     pv c
 *   b_c.kind == FNNUE_BEST_LOST: every reply loses       rank 3            FNNUE_BEST_MATE   pv c, b_c.move
 *   b_c.kind == FNNUE_BEST_MATE: the reply wins at once  rank 1            FNNUE_BEST_MATED  pv c, reply
 *   otherwise                                            rank 2, -b_c.value FNNUE_BEST_CP    pv c, reply
 * The higher rank wins, then the higher value, then the lower index.  The
 * record is fnnue_best2 as it is (kind may also be FNNUE_BEST_LOST); psqt /
 * positional of a two-move pv are b_c's as they are, those of a one-move pv the
 * child's own terms negated with wrap-around; nodes = children + the sum of
 * b_c.nodes; a ply without a legal move is FNNUE_BEST_NONE.  On end bytes that
 * use bits 0 and 1 only and child kinds NONE / CP / MATE the result equals
 * fnnue_best_replies' byte for byte.  Signature, buffers, clamping and launch
 * are fnnue_best_replies[_device]'s.  The key keeps the child's whole 32-bit
 * index, so a group may have as many children as npos <= 2^32 - 1 allows;
 * anything larger is FNNUE_E_ARG.  Any net. */
int fnnue_vbest_replies_device(fnnue_ctx *ctx, const uint8_t *d_end, const fnnue_move *d_moves, const uint32_t *d_off,
                               size_t ngroups, size_t npos, const fnnue_best *d_child_best, fnnue_best2 *d_out,
                               void *stream);
int fnnue_vbest_replies(fnnue_ctx *ctx, const uint8_t *end, const fnnue_move *moves, const uint32_t *off,
                        size_t ngroups, size_t npos, const fnnue_best *child_best, fnnue_best2 *out);
/* fnnue_search2[_device] / fnnue_search2_children for a variant net's context:
 * the same steps (fnnue_build_vchildren's level 1, the children's boards and
 * counts, chunks of whole plies within FNNUE_SEARCH2_RECORDS, per chunk the
 * expansion, fnnue_eval_vgroups STAR and the first reduction, then
 * fnnue_vbest_replies), the same capacity protocol and FNNUE_SEARCH2_TRACE.  A
 * ply whose records alone exceed the budget (a crazyhouse ply has no fixed
 * bound) is a chunk of its own; the results do not depend on the budget.  The
 * children's boards stay resident for the call: 88 bytes (kingofthehill,
 * racingkings, threecheck) or 104 (crazyhouse, atomic) per child, plus its
 * 24-byte record.  `variant` as for fnnue_vsearch1;
 * FNNUE_E_ARCH otherwise, and on a chess context.  Move codes are
 * fnnue_vmove_uci's.  The counts come back zeroed on every error that is not
 * FNNUE_E_CAPACITY, a null context included. */
int fnnue_vsearch2_device(fnnue_ctx *ctx, int variant, const char *d_text, const uint32_t *d_fen_off,
                          const uint32_t *d_moves_off, size_t ngames, fnnue_best2 *d_out, size_t cap, uint32_t *d_off,
                          size_t off_cap, size_t *n_out, size_t *n_groups, void *stream);
int fnnue_vsearch2(fnnue_ctx *ctx, int variant, const char *text, size_t text_len, const uint32_t *fen_off,
                   const uint32_t *moves_off, size_t ngames, fnnue_best2 *out, size_t cap, uint32_t *off,
                   size_t off_cap, size_t *n_out, size_t *n_groups);
int fnnue_vsearch2_children(fnnue_ctx *ctx, int variant, const char *text, size_t text_len, const uint32_t *fen_off,
                            const uint32_t *moves_off, size_t ngames, fnnue_best2 *out, size_t cap, uint32_t *off,
                            size_t off_cap, fnnue_best *child_best, uint32_t *child_map, size_t child_cap,
                            size_t *n_out, size_t *n_groups, size_t *n_children);

/* ---- MultiPV at two plies: the k best lines of a ply (ABI 3.11) ----
 * The second reduction's key extended to a total order, as fnnue_topk_children
 * extends the first's (the tie-break, the lower child index, is part of the
 * key, so the keys of a group are unique).  Best first, chess ranks:
 *   the mates in one, in index order;
 *   the values descending (a stalemating move 0, any other child -b_c.value),
 *     equal values by lower index;
 *   the children whose reply mates (FNNUE_BEST_MATED), in index order.
 * Variant ranks (descending fnnue_vbest_replies score): mate in one; every
 * reply loses at once (FNNUE_BEST_MATE, pv c, b_c.move); the values; the reply
 * wins at once (FNNUE_BEST_MATED); the FNNUE_END_WON children (FNNUE_BEST_LOST,
 * a one-move pv); each class in index order, the values as above. */
typedef struct {
  int32_t psqt, positional; /* of the pv's last position from the ply's side to move, exactly as fnnue_best2
                               reports them when this child is the best: a two-move pv -> b_c's as they are;
                               a one-move pv -> the child's own terms negated with wrap-around */
  int32_t value;            /* FNNUE_BEST_CP only, else 0 */
  uint32_t child;           /* 1-based record index in the ply's group */
  uint32_t reply_index;     /* 0 for a one-move pv */
  fnnue_move move, reply;   /* reply 0 for a one-move pv */
  uint8_t kind;             /* FNNUE_BEST_CP / _MATE / _MATED / _LOST; FNNUE_BEST_NONE = unused slot (all zero) */
  uint8_t pv_len;           /* 1 or 2 */
  uint16_t reserved;        /* 0 */
} fnnue_line2;
/* The ranking alone, one kernel on `stream` (no atomics, no host
 * synchronisation): fnnue_best_replies' arrays (end, moves or NULL, off,
 * child_best: dense, in record order; offsets beyond npos are clamped) and
 * fnnue_topk_children's slots: group g owns lines[line_off[g] .. line_off[g + 1])
 * (ngroups + 1 non-decreasing entries; the count may differ per group), slot j
 * receives the j-th child in the order above, slots beyond the group's children
 * are written all-zero, an empty group or one without a slot writes nothing.
 * Slot 0 equals the group's fnnue_best2 on every shared field (psqt,
 * positional, value, best == child, reply_index, move, reply, kind, pv_len).
 * The device form never writes at or beyond lines_cap; the host form refuses
 * line_off[ngroups] > lines_cap with FNNUE_E_CAPACITY.  fnnue_vtopk_replies:
 * the variants' ranks; npos > 2^32 - 1 is FNNUE_E_ARG.  Any net. */
int fnnue_topk_replies_device(fnnue_ctx *ctx, const uint8_t *d_end, const fnnue_move *d_moves, const uint32_t *d_off,
                              size_t ngroups, size_t npos, const fnnue_best *d_child_best,
                              const uint32_t *d_line_off, fnnue_line2 *d_lines, size_t lines_cap, void *stream);
int fnnue_topk_replies(fnnue_ctx *ctx, const uint8_t *end, const fnnue_move *moves, const uint32_t *off,
                       size_t ngroups, size_t npos, const fnnue_best *child_best, const uint32_t *line_off,
                       fnnue_line2 *lines, size_t lines_cap);
int fnnue_vtopk_replies_device(fnnue_ctx *ctx, const uint8_t *d_end, const fnnue_move *d_moves, const uint32_t *d_off,
                               size_t ngroups, size_t npos, const fnnue_best *d_child_best,
                               const uint32_t *d_line_off, fnnue_line2 *d_lines, size_t lines_cap, void *stream);
int fnnue_vtopk_replies(fnnue_ctx *ctx, const uint8_t *end, const fnnue_move *moves, const uint32_t *off,
                        size_t ngroups, size_t npos, const fnnue_best *child_best, const uint32_t *line_off,
                        fnnue_line2 *lines, size_t lines_cap);
/* fnnue_search2[_device] / fnnue_vsearch2[_device] plus, per ply p, its k best
 * lines at lines[p * k .. p * k + k) (k in 1..FNNUE_MAX_CHILDREN, anything else
 * FNNUE_E_ARG; a crazyhouse ply may have more children, k stays 1..218).  The
 * fnnue_best2 records and the offsets are fnnue_[v]search2's byte for byte;
 * the ranking runs once after the last chunk, beside the second reduction, and
 * adds no host wait.  The capacity protocol is fnnue_search1_lines':
 * lines_cap < plies * k is FNNUE_E_CAPACITY too (before anything is expanded,
 * *n_out set).  Nets and errors as fnnue_search2 / fnnue_vsearch2. */
int fnnue_search2_lines_device(fnnue_ctx *ctx, const char *d_text, const uint32_t *d_fen_off,
                               const uint32_t *d_moves_off, size_t ngames, uint32_t k, fnnue_best2 *d_out, size_t cap,
                               uint32_t *d_off, size_t off_cap, fnnue_line2 *d_lines, size_t lines_cap, size_t *n_out,
                               size_t *n_groups, void *stream);
int fnnue_search2_lines(fnnue_ctx *ctx, const char *text, size_t text_len, const uint32_t *fen_off,
                        const uint32_t *moves_off, size_t ngames, uint32_t k, fnnue_best2 *out, size_t cap,
                        uint32_t *off, size_t off_cap, fnnue_line2 *lines, size_t lines_cap, size_t *n_out,
                        size_t *n_groups);
int fnnue_vsearch2_lines_device(fnnue_ctx *ctx, int variant, const char *d_text, const uint32_t *d_fen_off,
                                const uint32_t *d_moves_off, size_t ngames, uint32_t k, fnnue_best2 *d_out,
                                size_t cap, uint32_t *d_off, size_t off_cap, fnnue_line2 *d_lines, size_t lines_cap,
                                size_t *n_out, size_t *n_groups, void *stream);
int fnnue_vsearch2_lines(fnnue_ctx *ctx, int variant, const char *text, size_t text_len, const uint32_t *fen_off,
                         const uint32_t *moves_off, size_t ngames, uint32_t k, fnnue_best2 *out, size_t cap,
                         uint32_t *off, size_t off_cap, fnnue_line2 *lines, size_t lines_cap, size_t *n_out,
                         size_t *n_groups);

/* ---- repetition and fifty-move draws in the device search (ABI 3.12) ----
 * Stockfish scores a node as a draw when its rule-50 counter has reached 100
 * and the node is not checkmate, and when the position stands for the third
 * time, counting the game before the root; fishnet sends `position fen ...
 * moves ...` so that the engine has that history ([ref] src/stockfish.rs:
 * 274-283).  The rule, per game, plies 0..n, ply 0 the root FEN:
 *  - clock(0) is the FEN's fifth field when it is an unsigned decimal number,
 *    saturating at 65535; 0 when the field is missing or not a number.
 *  - clock(i+1) is 0 when move i moves a pawn or captures (en passant
 *    included), else clock(i) + 1 (saturating).  Castling counts up.
 *  - The identity of a position is its piece placement, side to move, castling
 *    rights (the rooks' squares as the rules keep them) and en-passant square,
 *    the square counting only when a pawn of the side to move attacks it (the
 *    pseudo-legal test of SF 15.1).  The boards set the square on every double
 *    push and a root's comes verbatim from its FEN; the identity normalises it.
 *  - A searched position X is reached from ply P by one move (a child) or two
 *    (a grandchild).  Its history is the game's plies 0..P and the path's
 *    intermediate position; seen(X) is the number of history positions with X's
 *    identity; clock(X) follows the clock rule from clock(P).
 *  - X is drawn when seen(X) >= 2 (the third occurrence: Stockfish's is_draw
 *    with the search ply at most 2, where a first repetition inside the tree
 *    cannot happen), or when clock(X) >= 100 and X is not checkmate (its end
 *    byte is not NO_MOVES with CHECK).
 *  - P itself is never tested (the engine does not test its root): a ply with
 *    clock 120, or one that stands for the third time, is searched as usual.
 * A 64-bit key finds candidates; a record is marked only after the identity
 * has been compared on the boards themselves, so a key collision cannot change
 * a result.  (Equal identities cannot straddle an irreversible move, so only
 * the plies since the last one are looked at: an optimisation, never a
 * condition.)
 *
 * A drawn record carries FNNUE_END_DRAW in its end byte and ranks, in
 * fnnue_best_children, fnnue_topk_children, fnnue_best_replies and
 * fnnue_topk_replies (and the variants' forms: ABI 3.16 sets it there),
 * exactly as a record whose end byte is FNNUE_END_NO_MOVES alone: worth 0, the
 * pv ends there, kind FNNUE_BEST_CP, its terms those of a one-move pv.
 * Checkmate (NO_MOVES with a deciding flag) and FNNUE_END_WON take precedence,
 * and the search never sets the bit on those.  `nodes` does not change: the
 * same records are generated, a drawn child's own grandchildren are counted,
 * and its depth-1 record is ignored as a stalemating child's is (the search
 * stores the drawn child's own terms in that record's psqt / positional, as for
 * a child without a legal move).  End bytes without the bit give the results of
 * ABI 3.11 byte for byte.
 *
 * Out of scope: move work; insufficient material; draw tests on the root.
 * (Variant batches and the fnnue_vsearch* calls have their own rule and their
 * own switch: ABI 3.16, below.) */
#define FNNUE_END_DRAW 0x10
/* One per ply: its clock and the number of earlier plies of the same game with
 * its identity (saturating at 255). */
typedef struct {
  uint16_t clock;
  uint8_t seen;
  uint8_t reserved; /* 0 */
} fnnue_ply_history;
/* Every ply's history of every game: the builder's text layout, fnnue_search1's
 * capacity protocol (out: cap records, off: CHAIN offsets per game, ngames + 1
 * entries; *n_out = plies and *n_groups = games are set also with
 * FNNUE_E_CAPACITY), FNNUE_E_FEN / FNNUE_E_MOVE naming the game.  Chess rules.
 * fnnue_game_history is host only (the host replay, as fnnue_game_end);
 * the other two run on the device over the boards the replay leaves behind
 * (any net's context): a kernel that reads each game's clock field, one thread
 * per ply for the key and the move's reversibility, one thread per ply walking
 * back to the last irreversible move.  fnnue_ctx_game_history stages host
 * buffers through the context's stream. */
int fnnue_game_history(const char *text, size_t text_len, const uint32_t *fen_off, const uint32_t *moves_off,
                       size_t ngames, fnnue_ply_history *out, size_t cap, uint32_t *off, size_t off_cap,
                       size_t *n_out, size_t *n_groups);
int fnnue_game_history_device(fnnue_ctx *ctx, const char *d_text, const uint32_t *d_fen_off,
                              const uint32_t *d_moves_off, size_t ngames, fnnue_ply_history *d_out, size_t cap,
                              uint32_t *d_off, size_t off_cap, size_t *n_out, size_t *n_groups, void *stream);
int fnnue_ctx_game_history(fnnue_ctx *ctx, const char *text, size_t text_len, const uint32_t *fen_off,
                           const uint32_t *moves_off, size_t ngames, fnnue_ply_history *out, size_t cap,
                           uint32_t *off, size_t off_cap, size_t *n_out, size_t *n_groups);
/* The switch (default off) for fnnue_search1, fnnue_search1_lines,
 * fnnue_search2, fnnue_search2_children, fnnue_search2_lines and their _device
 * forms on a chess net's context: behind the expansion the history is computed,
 * the plies with a descendant that can be drawn at all (clock >= 98, or an
 * identity that already stands twice since the last irreversible move) are
 * compacted into a list, and a marking pass over that list alone applies each
 * record's move code to its parent board and ORs FNNUE_END_DRAW into the end
 * bytes, before the reductions.  A variant net's context accepts the setting
 * and ignores it.  FNNUE_DRAW_KEY_BITS in the environment (read per call, for
 * tests) truncates the key to that many bits (1..63). */
int fnnue_set_search_draws(fnnue_ctx *ctx, int on);
int fnnue_get_search_draws(const fnnue_ctx *ctx, int *on);

/* ---- capture quiescence below the search's leaves (ABI 3.13) ----
 * A bare static evaluation values the child after QxP as "a pawn up" also when
 * the pawn is defended.  Every engine the reference drives resolves captures
 * before it trusts an evaluation; this is the plain form of that, without
 * pruning.  The rule, for a chess position X and a depth d in 0..FNNUE_QUIESCE_MAX:
 *  - s(X) = trunc(((int64)psqt(X) + positional(X)) / 16), C truncation, from X's
 *    side to move, as fnnue_best_children takes it.
 *  - caps(X) is the set of X's legal moves after which the opponent has one
 *    piece fewer: en passant included, capturing promotions included (one move
 *    per promotion piece); a Chess960 castling move spelled king-takes-own-rook
 *    is no capture, nor is a quiet promotion.  Their order is the order of X's
 *    children in fnnue_build_children, restricted to captures.
 *  - Q_0(X) = s(X), line(X) = [];
 *    Q_d(X) = max(s(X), max over c in caps(X) of -Q_{d-1}(X.c)) for d >= 1.
 *    Candidate 0 is standing pat, the captures follow in order, and a later
 *    candidate replaces the current one only when it is strictly greater (the
 *    first maximum wins).  line(X) is empty for stand pat, else [c] +
 *    line_{d-1}(X.c); the line's end is the position after its last capture.
 *  - Checks, mates and stalemates are not recognised inside the tree: a side in
 *    check may stand pat, and a position without a legal move has no captures
 *    and is worth s.  This is the plain rule; "quiescence checks" (ABI 3.14,
 *    below) is the opt-in rule Q' that recognises evasions and mates.
 *  - The reported terms are the psqt / positional of the line's end, negated
 *    with int32 wrap-around (as fnnue_best negates) exactly when the line has an
 *    odd number of captures.  For terms that do not wrap, value ==
 *    trunc((psqt + positional) / 16) therefore holds for the reported triple.
 *  - nodes(X) is the number of capture records in the whole tree below X (every
 *    capture of every node above the last level), 0 at depth 0.
 *
 * In the searches, with quiescence depth d > 0 (fnnue_set_search_quiesce): a
 * leaf is a record j >= 1 of a ply's STAR group in a one-ply search, or of a
 * child's STAR group in a two-ply search.  Every leaf whose end byte has
 * neither FNNUE_END_NO_MOVES nor FNNUE_END_DRAW gets its (psqt, positional)
 * replaced by the reported terms of Q_d(leaf) before any reduction runs.
 * Nothing else changes: the reductions, ranks, tie rules, kinds, `nodes`,
 * `pv_len` and the pv are as before (the pv does not show the capture line),
 * records j = 0, leaves with NO_MOVES or DRAW and the terms a drawn or
 * stalemated child reports of its own are untouched.  A position below a
 * capture cannot repeat an earlier one and its clock is 0, so quiescence nodes
 * are never tested for draws and the two settings compose.  With depth 0 every
 * byte of every result is that of ABI 3.12.
 *
 * On the device the tree is level-synchronous (quiesce.hip): per level the
 * captures are counted, scanned, written as STAR groups [node, its captures]
 * and evaluated; a node without a capture forms no group.  Each level's size
 * is read back once (the calls synchronise their stream), and no level holds
 * more than FNNUE_QUIESCE_RECORDS records (environment, read per call; default
 * and most 16M, least 256): a slice of the leaves whose tree would is cut
 * down and redone; a single leaf's tree is never cut.  Results do not depend on the
 * slicing.  Out of scope: move work, check evasions, quiet promotions, any
 * pruning, extending the pv with the capture line (the variants: ABI 3.15). */
#define FNNUE_QUIESCE_MAX 4
typedef struct {            /* 20 bytes */
  int32_t psqt, positional; /* of the line's end, oriented to the position's side to move */
  int32_t value;            /* Q_d */
  uint32_t nodes;           /* capture records below the position */
  fnnue_move move;          /* the line's first capture, 0 when standing pat */
  uint8_t len;              /* captures in the line, 0..d */
  uint8_t reserved;         /* FNNUE_QUIET_DECIDED with quiescence checks and a decided result, else 0 */
} fnnue_quiet;
/* Host only: the game's last position followed by its capture children
 * (caps() above, in order) with their move codes, mv[0] = 0; cap entries in out
 * and mv.  *n_out is set also with FNNUE_E_CAPACITY; FNNUE_E_FEN / FNNUE_E_MOVE
 * as fnnue_game_children. */
int fnnue_game_captures(const char *fen, const char *moves, fnnue_pos *out, size_t cap, fnnue_move *mv,
                        size_t *n_out);
/* One fnnue_quiet per ply of every game, CHAIN offsets per game: signature
 * shape, capacity protocol and errors are fnnue_search1[_device]'s.  depth >
 * FNNUE_QUIESCE_MAX: FNNUE_E_ARG; a variant net's context: FNNUE_E_ARCH.  Depth
 * 0 gives the ply's own terms, nodes 0 and len 0. */
int fnnue_quiesce_device(fnnue_ctx *ctx, const char *d_text, const uint32_t *d_fen_off, const uint32_t *d_moves_off,
                         size_t ngames, uint32_t depth, fnnue_quiet *d_out, size_t cap, uint32_t *d_off,
                         size_t off_cap, size_t *n_out, size_t *n_groups, void *stream);
int fnnue_quiesce(fnnue_ctx *ctx, const char *text, size_t text_len, const uint32_t *fen_off,
                  const uint32_t *moves_off, size_t ngames, uint32_t depth, fnnue_quiet *out, size_t cap,
                  uint32_t *off, size_t off_cap, size_t *n_out, size_t *n_groups);
/* The quiescence depth (default 0, at most FNNUE_QUIESCE_MAX: FNNUE_E_ARG) of
 * fnnue_search1, fnnue_search1_lines, fnnue_search2, fnnue_search2_children,
 * fnnue_search2_lines and their _device forms.  A variant net's context accepts
 * the setting and ignores it. */
int fnnue_set_search_quiesce(fnnue_ctx *ctx, int depth);
int fnnue_get_search_quiesce(const fnnue_ctx *ctx, int *depth);
/* Diagnostics: the slices of leaves (whole frontiers count as one) the
 * context's quiescence has worked through since it was created. */
int fnnue_quiesce_slices(const fnnue_ctx *ctx, uint64_t *slices);

/* ---- check evasions and mates inside the capture quiescence (ABI 3.14) ----
 * The plain rule lets a side in check stand pat and scores a capture that
 * mates as the material it takes.  "Quiescence checks", an opt-in setting
 * (fnnue_set_search_quiesce_checks, off by default), replaces Q_d by Q'_d.
 * For a chess position X and a remaining depth d in 0..FNNUE_QUIESCE_MAX:
 *  - chk(X): X's side to move is in check.
 *  - cand(X): all of X's legal moves when chk(X), in the order of X's children
 *    in fnnue_build_children; caps(X) otherwise, unchanged.
 *  - Mated: if chk(X) and X has no legal move, X is mated at every d, 0
 *    included: value -FNNUE_VALUE_MATE, line empty, nodes 0.
 *  - Horizon: otherwise Q'_0(X) = s(X).  A side in check that still has a move
 *    stands pat at the horizon; this is a stated limit.
 *  - In check, d >= 1: Q'_d(X) = max over cand(X) of the negated child result.
 *    No standing pat: candidate 0 is the first evasion, and a later candidate
 *    replaces the current one only when it is strictly greater.
 *  - Not in check, d >= 1: as Q_d, stand pat is candidate 0, then the captures.
 *    A position that is not in check and has no capture stands pat: stalemate
 *    is not recognised, as before.
 *  - Negating a decided (mate) child result moves it one ply toward zero:
 *    child -32000 gives the parent 31999, child 31999 gives -31998, and so on.
 *    Undecided results negate as before.
 *  - Reported terms.  A decided result reports psqt = 0 and positional = 16 *
 *    value, so value == trunc((psqt + positional) / 16) still holds, and its
 *    `reserved` byte carries FNNUE_QUIET_DECIDED.  An undecided result reports
 *    the terms of its line's end exactly as Q_d does, with `reserved` 0; with
 *    the setting off `reserved` is always 0.
 *  - nodes counts every record of the tree, evasions included; move / len
 *    describe the line, which may start with and contain quiet evasions.
 *  - Domain: static values must satisfy |s| < FNNUE_VALUE_MATE - 64 (real nets
 *    are far below).  Beyond that, results are unspecified with the setting on.
 *  - Draws: a quiet evasion can repeat an earlier position, so "a node below a
 *    capture cannot repeat" no longer covers every node of the tree.  Nodes
 *    inside the tree are still not tested for draws; leaves with DRAW or
 *    NO_MOVES stay untouched, as before.
 *
 * In the searches a leaf at search depth p (1 in the one-ply searches, 2 in
 * the two-ply ones) whose Q' is decided gets the terms (0, 16 * v) with |v| =
 * FNNUE_VALUE_MATE - (p + n), n the mate's distance inside the tree: the leaf
 * counts plies from the searched ply.  The reductions, ranks and kinds are
 * untouched: a coded mate is an ordinary FNNUE_BEST_CP value, which ranks
 * below a flagged mate in 1 and above a flagged FNNUE_BEST_MATED.
 * fnnue_quiesce[_device] reports distances from the ply itself (p = 0).  With
 * the setting off, or with quiescence depth 0 in the searches, every byte of
 * every result is that of ABI 3.13.  The setting governs fnnue_search1[_lines],
 * fnnue_search2[_children|_lines], their _device forms and
 * fnnue_quiesce[_device]; a variant net's context accepts and ignores it.
 * Evasion records count toward FNNUE_QUIESCE_RECORDS like capture records.
 * Out of scope: quiet checks or quiet promotions as candidates, stalemate and
 * draw tests inside the tree, pruning (the variants: ABI 3.15). */
#define FNNUE_VALUE_MATE 32000
#define FNNUE_QUIET_DECIDED 1
int fnnue_set_search_quiesce_checks(fnnue_ctx *ctx, int on);
int fnnue_get_search_quiesce_checks(const fnnue_ctx *ctx, int *on);
/* Host only: the game's last position followed by cand() of it in order, with
 * the move codes (mv[0] = 0) and *in_check = chk(); capacity and error protocol
 * as fnnue_game_captures.  A position in check lists every legal move, any
 * other its captures. */
int fnnue_game_quiet_moves(const char *fen, const char *moves, fnnue_pos *out, size_t cap, fnnue_move *mv,
                           int *in_check, size_t *n_out);

/* ---- capture quiescence for the variant searches (ABI 3.15) ----
 * The same tree for crazyhouse, atomic, kingofthehill, racingkings and
 * threecheck, with the variant's legality and its end of the game inside the
 * tree.  For a variant position X (board, pockets, en-passant square and
 * threecheck counters as the variant's replay gives them), a remaining depth d
 * in 0..FNNUE_QUIESCE_MAX and the setting `checks`:
 *  - s(X) = trunc((psqt + positional) / 16), as above.
 *  - over(X), decided without generating a move, at every d (0 included), with
 *    checks on or off: X's side to move has no king (atomic: exploded): lost.
 *    The variant's own end of the game: lost (a king on the hill; the other
 *    side's threecheck counter at 0; the other racing king alone on rank 8 with
 *    no catch-up), won (the own king alone on rank 8; a threecheck position
 *    whose own counter is 0) or drawn (both racing kings on rank 8).  Lost is
 *    worth -FNNUE_VALUE_MATE, won +FNNUE_VALUE_MATE, drawn 0; all three are
 *    decided: line empty, nodes 0, terms (0, 16 * value), reserved =
 *    FNNUE_QUIET_DECIDED.
 *  - vcaps(X): X's legal moves (never drops, never castling) whose capture
 *    square holds an opponent's piece: the target square, or for en passant the
 *    square behind an empty en-passant square.  Their order is that of X's
 *    children in fnnue_build_vchildren, one move per promotion piece.  Legality
 *    is the variant's: an atomic capture that explodes the own king is no
 *    candidate, one that explodes the other king is, atomic kings never
 *    capture, and a racingkings capture may not give check.
 *  - chk(X), with `checks` only: X's side to move's king is in danger by the
 *    variant's rule (atomic kings next to each other are never in danger);
 *    racingkings positions are never in check.
 *  - cand(X): all legal moves in children order when chk(X), crazyhouse drops
 *    included; vcaps(X) otherwise.
 *  - A position that is not over: chk(X) without a legal move is mated at every
 *    d (value -FNNUE_VALUE_MATE, decided).  Otherwise d = 0 gives s(X) (a side
 *    in check with a move stands pat at the horizon); d >= 1 with chk(X) gives
 *    the maximum over cand(X) of the negated child results, candidate 0 being
 *    the first evasion; d >= 1 otherwise has standing pat as candidate 0, then
 *    the captures.  A later candidate replaces the current one only when it is
 *    strictly greater.
 *  - Negating a decided child: v > 0 gives -(v - 1), v < 0 gives -(v + 1), and
 *    0 stays 0 and stays decided.  Undecided results negate their terms with
 *    int32 wrap-around.
 *  - nodes, move, len and the reported terms are as in ABI 3.13 / 3.14; move is
 *    a variant move code (fnnue_vmove_uci), so a line may start with a drop.
 *  - Domain: |s| < FNNUE_VALUE_MATE - 64.  A crazyhouse capture keeps the
 *    pieces on board and in hand constant and an atomic one lowers them, so
 *    every record of the tree is inside the evaluator's domain; a position with
 *    one king exploded evaluates to (0, 0) and the rule overrides its value.
 *  - Stated limits: stalemate and draws by repetition are not recognised
 *    inside the tree; quiet checks, quiet promotions and quiet drops are no
 *    candidates; there is no pruning.
 *
 * In the variant searches (fnnue_set_search_vquiesce, depth > 0) the leaves
 * that take part are the records j >= 1 of a ply's STAR group (one ply) or of
 * a child's (two plies) whose end byte has none of FNNUE_END_NO_MOVES,
 * FNNUE_END_DRAW, FNNUE_END_WON.  Each gets the reported terms of its Q before
 * any reduction; a decided non-zero result is written as (0, 16 * v) with |v| =
 * FNNUE_VALUE_MATE - (p + n), p the leaf's search depth (1 or 2) and n the
 * distance inside the tree, a decided draw as (0, 0).  Reductions, variant
 * ranks, kinds, nodes, pv_len and the pv are untouched.  Slicing
 * (FNNUE_QUIESCE_RECORDS) and fnnue_quiesce_slices are as for chess. */
#define FNNUE_VQ_CHECK 1 /* chk(X) (with `checks` only, never with an over bit) */
#define FNNUE_VQ_LOST 2
#define FNNUE_VQ_WON 4
#define FNNUE_VQ_DRAWN 8
/* Host only: the game's last position followed by cand() of it in order, with
 * the variant move codes (mv[0] = 0); *state: FNNUE_VQ_* bits.  An over
 * position lists nothing.  Capacity and error protocol are
 * fnnue_game_quiet_moves's. */
int fnnue_game_vquiet_moves(int variant, const char *fen, const char *moves, int checks, fnnue_vpos *out, size_t cap,
                            fnnue_move *mv, int *state, size_t *n_out);
/* One fnnue_quiet per ply of every game, CHAIN offsets per game: signature
 * shape, capacity protocol and errors are fnnue_vsearch1[_device]'s.
 * FNNUE_E_ARCH on a chess net's context or for a variant the net does not
 * serve; FNNUE_E_ARG for depth > FNNUE_QUIESCE_MAX.  Distances count from the
 * ply itself (p = 0). */
int fnnue_vquiesce_device(fnnue_ctx *ctx, int variant, const char *d_text, const uint32_t *d_fen_off,
                          const uint32_t *d_moves_off, size_t ngames, uint32_t depth, int checks, fnnue_quiet *d_out,
                          size_t cap, uint32_t *d_off, size_t off_cap, size_t *n_out, size_t *n_groups, void *stream);
int fnnue_vquiesce(fnnue_ctx *ctx, int variant, const char *text, size_t text_len, const uint32_t *fen_off,
                   const uint32_t *moves_off, size_t ngames, uint32_t depth, int checks, fnnue_quiet *out, size_t cap,
                   uint32_t *off, size_t off_cap, size_t *n_out, size_t *n_groups);
/* The quiescence depth (default 0, at most FNNUE_QUIESCE_MAX: FNNUE_E_ARG) and
 * its checks setting for fnnue_vsearch1[_lines], fnnue_vsearch2[_children|
 * _lines] and their _device forms.  A chess net's context accepts the setting
 * and ignores it, as a variant net's context keeps ignoring
 * fnnue_set_search_quiesce[_checks].  With depth 0 every byte of every result
 * is that of ABI 3.14. */
int fnnue_set_search_vquiesce(fnnue_ctx *ctx, int depth, int checks);
int fnnue_get_search_vquiesce(const fnnue_ctx *ctx, int *depth, int *checks);

/* ---- repetition and fifty-move draws in the variant searches (ABI 3.16) ----
 * The rule of ABI 3.12 for crazyhouse, atomic, kingofthehill, racingkings and
 * threecheck.  It is this project's own (no engine output pins it); everything
 * not named here is ABI 3.12's text unchanged: P itself is never tested; the
 * history of a searched position X is the game's plies 0..P plus the path's
 * intermediate position; X is drawn when seen(X) >= 2, or when clock(X) >= 100
 * and X is not decided; `nodes` is unchanged; a drawn child's depth-1 record
 * holds the child's own terms; keys are filters, every mark is confirmed on the
 * boards.
 *  - Identity, all variants: chess's.  Placement, side to move, the castling
 *    rooks as the rules keep them, and the en-passant square counted only when a
 *    pawn of the side to move attacks it.
 *  - Identity, crazyhouse: also both pockets and the promoted marks (two
 *    positions that differ only in which queen turns into a pawn when captured
 *    are different positions).
 *  - Identity, threecheck: also both check counters (a placement that returns
 *    after a check was given is a different position).
 *  - Clock (atomic, kingofthehill, racingkings, threecheck): clock(i+1) is 0
 *    when move i moves a pawn or removes a piece from the board (a capture; an
 *    atomic explosion removes at least two), else clock(i) + 1, saturating at
 *    65535.  Castling counts up, and so does a checking move in threecheck.
 *    clock(0) is the FEN's fifth field by chess's rule; in threecheck it is the
 *    first field from the fifth on that contains no '+' (so "... - 3+3 98 60",
 *    whose fifth field holds the counters, has clock 98, and "... - 0 1 +0+0"
 *    has clock 0).
 *  - Crazyhouse has no clock rule: a captured piece comes back from the pocket,
 *    so neither a capture nor a pawn move makes a position unreachable, and
 *    lichess, whose games these are, does not apply the fifty-move rule there.
 *    fnnue_ply_history.clock is 0 on every crazyhouse ply, nothing is drawn by a
 *    clock, and the repetition history is the whole game: no window cuts it.
 *  - "Not checkmate" becomes "not decided": a record is never marked when its
 *    end byte has FNNUE_END_WON, or FNNUE_END_NO_MOVES together with the check,
 *    exploded-king or FNNUE_END_VARIANT bit (a mate, an exploded king, a king on
 *    the hill or on rank 8, a third check).  A racingkings draw and a stalemate
 *    (NO_MOVES alone) may be marked; they are worth 0 either way.
 *  - The window: in the four clocked variants equal identities cannot straddle
 *    a clock-resetting move, so the walk stops there (an optimisation, as in
 *    3.12; a threecheck counter change needs none, the identities differ).  In
 *    crazyhouse the walk goes back to the root, and a ply is on the marking
 *    list as soon as any ply of its game up to it has been seen before.
 * Out of scope: move work, antichess and horde, insufficient material, draw
 * tests on the root, draws inside the quiescence tree.
 *
 * The history calls follow fnnue_game_history's protocol and errors, with
 * FNNUE_E_ARG for chess or an unknown variant.  fnnue_game_vhistory is host
 * only (the host variant replay).  The other two replay on the device and need
 * a context only for its device, stream and scratch: any net's context serves,
 * a chess net's included, whatever variant is asked for. */
int fnnue_game_vhistory(int variant, const char *text, size_t text_len, const uint32_t *fen_off,
                        const uint32_t *moves_off, size_t ngames, fnnue_ply_history *out, size_t cap, uint32_t *off,
                        size_t off_cap, size_t *n_out, size_t *n_groups);
int fnnue_game_vhistory_device(fnnue_ctx *ctx, int variant, const char *d_text, const uint32_t *d_fen_off,
                               const uint32_t *d_moves_off, size_t ngames, fnnue_ply_history *d_out, size_t cap,
                               uint32_t *d_off, size_t off_cap, size_t *n_out, size_t *n_groups, void *stream);
int fnnue_ctx_game_vhistory(fnnue_ctx *ctx, int variant, const char *text, size_t text_len, const uint32_t *fen_off,
                            const uint32_t *moves_off, size_t ngames, fnnue_ply_history *out, size_t cap,
                            uint32_t *off, size_t off_cap, size_t *n_out, size_t *n_groups);
/* The switch (default off) for fnnue_vsearch1[_lines], fnnue_vsearch2[_children|
 * _lines] and their _device forms, at the place fnnue_set_search_draws acts for
 * chess: the marks are set behind the expansion and before the quiescence and
 * the reductions, so a drawn leaf is not quiesced.  A chess net's context
 * accepts the setting and ignores it, as a variant net's context keeps ignoring
 * fnnue_set_search_draws.  FNNUE_DRAW_KEY_BITS applies.  With the setting off
 * every byte of every result is that of ABI 3.15. */
int fnnue_set_search_vdraws(fnnue_ctx *ctx, int on);
int fnnue_get_search_vdraws(const fnnue_ctx *ctx, int *on);

/* ---- diagnostics ----
 * Runs the int8 MFMA operand-layout self test on `device`; 0 if the hardware
 * layout matches the kernels' assumption. */
int fnnue_selftest_mfma(int device);
/* Feature-transformer implementation for fnnue_eval_positions*:
 *  FNNUE_FT_SLICED: LDS-stationary weight tiles, positions planned and sorted
 *    on the device; for fnnue_eval_groups*, the incremental
 *    updates run on the same tiles (segments of positions that share the
 *    perspective's king square).
 *  FNNUE_FT_GATHER: one wave per position (groups: per group) gathering rows
 *    from L2/HBM.
 *  FNNUE_FT_AUTO (default): chess positions calls of at most
 *    FNNUE_FT_GATHER_MAX positions gather (the sliced plan and its tile loads
 *    are a fixed ~60-80 us that a small call does not amortise: move work's
 *    children, a few games' positions), larger ones and every grouped call
 *    run sliced.
 * All are bit-identical; the environment variable FNNUE_FT_IMPL=
 * gather|sliced|auto sets the default for new contexts. */
#define FNNUE_FT_SLICED 0
#define FNNUE_FT_GATHER 1
#define FNNUE_FT_AUTO 2
#define FNNUE_FT_GATHER_MAX 16384
int fnnue_ctx_set_ft_impl(fnnue_ctx *ctx, int impl);
/* SWAR row sums in the sliced feature transformer: pairs of int16 columns
 * summed as 32-bit words.  Exact whenever no reachable
 * accumulator's even column leaves int16 range; the library checks that from
 * the weights (fnnue_net_accumulator_bound < 32768) and turns SWAR on by
 * itself (FNNUE_SWAR=0 in the environment keeps it off).  Results are
 * identical either way; set_swar(1) fails with FNNUE_E_ARCH on a net whose
 * bound does not allow it. */
int fnnue_net_accumulator_bound(const fnnue_net *net, int32_t *bound);
int fnnue_ctx_swar(const fnnue_ctx *ctx, int *enabled, int32_t *bound);
int fnnue_ctx_set_swar(fnnue_ctx *ctx, int enable);
/* The decision is made per 64-column slice (ABI 3.3).  Slice s of a net of
 * width hd covers columns [32s, 32s + 32) of each half; a SWAR word never
 * spans two slices, so every slice whose own bound is below 32768 runs SWAR
 * rows and the others run packed int16 rows, in one launch.
 * fnnue_net_slice_bounds writes the hd / 64 slice bounds (cap >= hd / 64, else
 * FNNUE_E_ARG; *nslices is set either way); their maximum is
 * fnnue_net_accumulator_bound.  fnnue_ctx_swar_slices reports bit masks over
 * the slices (at most 48): eligible (bound < 32768) and enabled.  A new
 * context enables every eligible slice (none with FNNUE_SWAR=0).
 * fnnue_ctx_set_swar_slices sets the enabled mask: FNNUE_E_ARG for a bit
 * >= nslices, FNNUE_E_ARCH for an ineligible slice.  fnnue_ctx_swar reports
 * enabled != 0 and the net bound; fnnue_ctx_set_swar(1) enables every eligible
 * slice (FNNUE_E_ARCH when there is none), (0) clears the mask. */
int fnnue_net_slice_bounds(const fnnue_net *net, int32_t *bounds, size_t cap, size_t *nslices);
int fnnue_ctx_swar_slices(const fnnue_ctx *ctx, uint64_t *eligible, uint64_t *enabled, uint32_t *nslices);
int fnnue_ctx_set_swar_slices(fnnue_ctx *ctx, uint64_t mask);

/* Kernel timing with HIP events on the launch stream: when enabled, every
 * chunk launched by a *_device call records events around the feature-
 * transformer kernel and the layer-stack kernel.  fnnue_ctx_timing_read
 * synchronises on the last event, returns the number of timed launches and the
 * summed kernel times (ms), and resets the accumulators.
 * enable: FNNUE_TIMING_OFF (0), FNNUE_TIMING_ALL (1, any other non-zero value:
 * four events per chunk, plan / FT kernel / stacks), FNNUE_TIMING_FT (2: only
 * the two events around the FT main kernel; plan and stack times read 0).  An
 * event record between two kernels costs the stream a few microseconds, so a
 * throughput measurement times with FNNUE_TIMING_FT. */
#define FNNUE_TIMING_OFF 0
#define FNNUE_TIMING_ALL 1
#define FNNUE_TIMING_FT 2
int fnnue_ctx_set_timing(fnnue_ctx *ctx, int enable);
int fnnue_ctx_timing_read(fnnue_ctx *ctx, uint32_t *launches, double *ft_ms, double *stack_ms);
/* Same, split into the FT plan kernels, the FT main kernel (ft_slices /
 * ft_segments / ft_scratch / ft_groups) and the layer stacks. */
int fnnue_ctx_timing_phases(fnnue_ctx *ctx, uint32_t *launches, double *plan_ms, double *ft_ms, double *stack_ms);

#ifdef __cplusplus
}
#endif
#endif /* FNNUE_H */
