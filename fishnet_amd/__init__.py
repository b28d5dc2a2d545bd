"""fishnet_amd — MI355X-native batched NNUE static evaluator for fishnet's
analysis path (HIP/CDNA4 kernels behind the C ABI in include/fnnue.h)."""
from .nnue import (  # noqa: F401
    Evaluator, FnnueError, MultiEvaluator, Net, device_count, partition_groups, game_children, game_positions, perft, pos_from_fen,
    pack_games, random_game, random_playouts, random_vpositions, selftest_mfma, synthesize_net,
    synthesize_variant_net, vpos_from_fen, game_vpositions, game_vchildren, vperft, random_vgame, random_vgames,
    game_end, END_NO_MOVES, END_CHECK, END_EXTINCT, END_VARIANT, END_WON, BEST_LOST, vmove_uci,
    Best, BEST_DTYPE, BEST_NONE, BEST_CP, BEST_MATE, move_uci, Line, LINE_DTYPE, MAX_CHILDREN,
    BEST2_DTYPE, BEST_MATED, LINE2_DTYPE, END_DRAW, PLY_HISTORY_DTYPE, game_history,
    QUIET_DTYPE, QUIESCE_MAX, game_captures, game_quiet_moves, VALUE_MATE, QUIET_DECIDED,
    game_vquiet_moves, VQ_CHECK, VQ_LOST, VQ_WON, VQ_DRAWN, game_vhistory,
)
from ._native import (  # noqa: F401
    GROUP_CHAIN, GROUP_STAR, PLAYOUT_CHILDREN, PLAYOUT_FINAL, PLAYOUT_PLIES, VARIANT_ATOMIC, VARIANT_CRAZYHOUSE,
    VARIANT_KINGOFTHEHILL, VARIANT_RACINGKINGS, VARIANT_THREECHECK,
)
