/*
 * include/fpc_engine.h -- C-ABI of the MI355X-native batched self-play engine for 4-player chess.
 *
 * This is the drop-in boundary for the MCTS.search hot path of jorr3/Alphazero-4-player-chess.
 * The reference has no C-ABI of its own: its boundary is the pybind11 module `alphazero_cpp`
 * (/root/reference/src/cpp/wrapper.cpp:15-254) plus three Python files on top of it
 * (src/py/mcts.py, src/py/four_player_chess_board.py, src/py/fen_parser.py).  Every entry point
 * below names the reference interface it replaces.  The Python class surface the training loop
 * uses (Board, Move, Node, MCTS, FourPlayerChess ...) is rebuilt over these entry points by the
 * ctypes shim in alphazero-4-player-chess_amd/alphazero_cpp.py.
 *
 * Conventions: plain pointers and sizes, no C++/torch types; every function returns 0 on
 * success or a negative fpc_status; fpc_last_error() gives the message (the shim raises
 * RuntimeError, mirroring the exception translator at wrapper.cpp:17-27).  All compute runs on the
 * GPU; there is no CPU fallback -- without a HIP device fpc_create fails with FPC_ENODEVICE.
 * One engine handle per GPU / per host thread (thread-compatible, not thread-safe).
 */
#ifndef FPC_ENGINE_H_
#define FPC_ENGINE_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define FPC_MAX_SQ 196      /* 14 x 14 */
#define FPC_MAX_PL 16       /* pieces per colour kept in a piece list */
#define FPC_NO_SQ 255
#define FPC_MAX_MOVES 256   /* pseudo-legal moves per position handled on device (reference buffer: 300, engine/board.h:706) */

typedef enum fpc_status {
  FPC_OK = 0,
  FPC_EINVAL = -1,      /* bad argument */
  FPC_ENODEVICE = -2,   /* no HIP device / HIP runtime failure */
  FPC_ENOMEM = -3,
  FPC_ESELECT = -4,     /* node.cpp:72-75 "Failed to select a child." */
  FPC_EPOLICY = -5,     /* legal policy mass is 0/NaN: the reference expands every index and throws (mcts.py:76,84) */
  FPC_ECAPACITY = -6,   /* node/board pool or move buffer overflow (reference: abort(), engine/board.h:482-486) */
  FPC_EMOVE = -7,       /* engine/board.cpp:1046-1054 "piece missing for move" */
  FPC_EUNSUPPORTED = -8,/* reserved */
  FPC_ESTATE = -9,      /* call sequence error */
  FPC_EWEIGHTS = -10,   /* weight blob malformed / not loaded */
  FPC_ECOMM = -11       /* RCCL failure (library missing, communicator error): message names the ncclResult */
} fpc_status;

/* chess::GameResult, engine/board.h:438-444 */
enum { FPC_IN_PROGRESS = 0, FPC_WIN_RY = 1, FPC_WIN_BG = 2, FPC_STALEMATE = 3 };

/*
 * One position == chess::Board state (engine/board.h:696-706) as a 288-byte POD.
 * piece byte: 0 = empty, else 0x80 | colour<<5 | type<<2  (engine/board.h:101-104;
 * colour RED 0 BLUE 1 YELLOW 2 GREEN 3, type PAWN 0 .. KING 5).
 * pl[c][i] is the square (row*R+col) of the i-th entry of piece_list_[c] IN REFERENCE LIST ORDER:
 * that order is observable (it decides which move GetGameResult looks at first,
 * engine/board.cpp:904-925) and is mutated by MakeMove/UndoMove, so it is part of the state.
 */
typedef struct fpc_board {
  uint8_t sq[FPC_MAX_SQ];
  uint8_t pl[4][FPC_MAX_PL];
  uint8_t plen[4];
  uint8_t king[4];         /* king_locations_ (FPC_NO_SQ if captured) */
  uint8_t castle[4];       /* bit0 kingside, bit1 queenside (constant through tree/self-play moves) */
  uint8_t turn;
  uint8_t pad[15];
} fpc_board;               /* sizeof == 288 */

/* One legal move as the reference's Board::GetLegalMoves() reports it (board.cpp:94-118). */
typedef struct fpc_move {
  uint8_t from, to;
  uint8_t capture;         /* piece byte on `to` (0 none) */
  uint8_t promo;           /* 1 if the reference emits this move 4x (N,B,R,Q promotion variants, engine/board.cpp:82-88) */
  uint16_t flat;           /* Move::GetFlatIndex(), move.cpp:100-104 */
  uint16_t pad;
} fpc_move;

typedef struct fpc_config {
  int board_size;          /* rows_ == cols_  : 8 (literal snapshot) or 14      engine/board.h:22-23 */
  int invalid_area;        /* invalid_area    : 2 or 3                           engine/board.h:24    */
  int max_games;           /* concurrent games on this GPU (num_parallel_games, alphazero.py:303)    */
  int max_sims;            /* upper bound for num_searches (mcts.py:36)                              */
  int avg_children;        /* node pool = 1 + max_sims*avg_children per game; 0 -> default 96        */
  int device;              /* HIP device ordinal                                                     */
  int nn_dtype;            /* 0 = bf16, 1 = fp16 (MFMA operand type of the internal ResNet)          */
} fpc_config;

typedef struct fpc_engine fpc_engine;

int  fpc_create(const fpc_config *cfg, fpc_engine **out);
void fpc_destroy(fpc_engine *e);
const char *fpc_last_error(const fpc_engine *e);   /* e may be NULL: last create() failure */
int  fpc_abi_version(void);

/* ---- static geometry: fpchess::Board statics, board.cpp:9-14 / wrapper.cpp:176-181 ---- */
int fpc_num_action_channels(int board_size);       /* 4R+4C+8 */
int fpc_action_space_size(int board_size);
int fpc_is_legal_location(int board_size, int invalid_area, int row, int col);  /* engine/board.h:647-654 */
/* fpchess::Move codec, move.cpp:23-104.  fpc_flat_to_move returns FPC_NO_SQ in *to when the
 * target falls off the board (BoardLocation() "missing"). */
int fpc_move_flat_index(int board_size, int from, int to);   /* -1: GetIndex() throws */
int fpc_flat_to_move(int board_size, int flat, int *from, int *to);

/* ---- host-side construction: chess::Board::Board, engine/board.cpp:1172-1248 ----
 * (sq[i], piece[i]) in python-dict insertion order, exactly what pybind hands the reference ctor.
 * Reproduces the constructor's piece_list_ order (unordered_map iteration + std::sort). */
int fpc_board_from_dict(fpc_board *out, int board_size, int turn, const uint8_t *sq, const uint8_t *piece,
                        int n, const uint8_t *castle4 /* nullable */);

/* ---- batched position kernels (one wavefront per position) -------------------------------
 * boards[] live in HOST memory; they are uploaded, processed on the GPU and written back
 * (the reference mutates piece-list order in place in all of these). */
/* Board::GetLegalMoves  (board.cpp:94-118): moves[i*FPC_MAX_MOVES ..] in reference order */
int fpc_boards_legal_moves(fpc_engine *e, fpc_board *boards, int n, fpc_move *moves, int *counts);
/* Board::GetGameResult(opt_player) (engine/board.cpp:891-939); player[i] = -1 -> side to move */
int fpc_boards_game_result(fpc_engine *e, fpc_board *boards, int n, const int *player, int *results);
/* Board::TakeAction(Move(flat)) (board.cpp:234-239, move.cpp:39-61): out[i] = copy + MakeMove */
int fpc_boards_take_action(fpc_engine *e, const fpc_board *boards, const int *flat, int n, fpc_board *out);
/* Board::GetEncodedStates (board.cpp:305-356): out_host [n,24,R,R] f32, rotated by boards[0].turn */
int fpc_boards_encode(fpc_engine *e, const fpc_board *boards, int n, float *out_host);
/* FourPlayerChess.get_legal_moves_mask (four_player_chess_board.py:36-56): out_host [n,A_ch,R,R] f32 */
int fpc_boards_legal_mask(fpc_engine *e, fpc_board *boards, int n, float *out_host);
/* Board::GetAttackedSquaresPlayers / GetAttackedSquaresTeams / IsAttackedByPlayer (wrapper.cpp:204-206; board.cpp:120-232):
 * out_host [n][6][R*R] bytes, 1 = attacked -- maps 0..3 by colour (fpchess IsAttackedByPlayer: its own probe set, rays
 * through the cut corners), maps 4..5 by team (the engine's IsAttackedByTeam); every row x column of the array */
int fpc_boards_attack_maps(fpc_engine *e, const fpc_board *boards, int n, uint8_t *out_host);
/* Board::CalculateHeuristic (engine/board.cpp:1263-1292), pure host arithmetic on the POD */
int fpc_board_heuristic(const fpc_board *b, int team);

/* ---- MCTS.search (mcts.py:17-43) ---------------------------------------------------------
 * begin:   fresh root per game, visit_count = 1 (mcts.py:29-32; 0 under FPC_RULES_VISITS); roots uploaded once.
 * Then either drive it step by step with an external evaluator (the reference's
 * `neural_net(x) -> (logits, value)` seam, mcts.py:65-66):
 *     for each of num_searches:  fpc_search_select -> evaluator -> fpc_search_expand
 * or let the engine run all simulations with its internal MFMA ResNet: fpc_search_run. */
int fpc_search_begin(fpc_engine *e, const fpc_board *roots, int n_games, double c_puct);
/* get_expandable_leaves + GetEncodedStates (mcts.py:18-26,65): selects one leaf per live game,
 * handles terminal leaves (node.cpp:31-42), encodes the leaves.  *n_live = leaves to evaluate.
 * enc_dev: DEVICE pointer, [n_games,24,R,R] f32 (slot g = game g; dead games are all-zero). */
int fpc_search_select(fpc_engine *e, int *n_live, const float **enc_dev);
/* softmax/ParseActionspace/mask/renormalise + BackpropagateNodes + ExpandNodes (mcts.py:67-89).
 * logits_dev [n_games, A] f32 and value_dev [n_games] f32 are DEVICE pointers (slot g = game g). */
int fpc_search_expand(fpc_engine *e, const float *logits_dev, const float *value_dev);
/* fpc_search_expand of this simulation followed by fpc_search_select of the next one, as ONE launch
 * (k_expand_select): what the loop mcts.py:36-38 does between two evaluator calls.  Same arguments and
 * results as the two calls it replaces; use plain fpc_search_expand after the last evaluation. */
int fpc_search_expand_select(fpc_engine *e, const float *logits_dev, const float *value_dev, int *n_live, const float **enc_dev);
/* all `sims` simulations with the internal network (weights from fpc_load_weights) */
int fpc_search_run(fpc_engine *e, int sims);
/* How fpc_search_run evaluates the policy head (net.py:22-26 + mcts.py:67-76):
 *   FPC_POLICY_FULL  (default) the whole Linear A -> A, softmax over all A outputs, mask, renormalise
 *                    -- the reference's arithmetic, op for op;
 *   FPC_POLICY_LEGAL the Linear only at the leaf's legal moves (the softmax denominator cancels in
 *                    mask + renormalise): the same priors up to f32 rounding, 1/50th of the weight
 *                    traffic.  Not bit-comparable with FULL; deviates where a legal logit lies ~87
 *                    below the global maximum (FULL flushes that child to zero).  Opt-in. */
enum { FPC_POLICY_FULL = 0, FPC_POLICY_LEGAL = 1 };
int fpc_set_policy_mode(fpc_engine *e, int mode);
/* ---- N4: root Dirichlet noise and the non-strict ("fixed") rule set ---------------
 * Strict reference semantics (every quirk of SURVEY 8a-Q, bit-exact with the reference) are the default.
 * fpc_set_rules switches individual corrections on for real training runs; none of them is covered by a
 * parity claim against the reference -- they are held against the oracle running the same rule set. */
enum {
  FPC_RULES_STRICT = 0,
  FPC_RULES_PUCT = 1,        /* Q2 + Q3: U = C P sqrt(N_parent) / (1 + N), child value seen from the parent (-W/N)   node.cpp:53-63 */
  FPC_RULES_ROTATION = 2,    /* Q6: every sample is rotated by its OWN side to move (encode and policy decode)       board.cpp:322,354-355 */
  FPC_RULES_PLANES = 4,      /* Q7: input plane 6*rel_colour + type, no -1 wrap                                       board.cpp:336 */
  FPC_RULES_FULL_MOVES = 8,  /* Q9: tree/self-play moves promote (to a queen), hop the rook when castling, update rights  node.cpp:87-92 */
  FPC_RULES_FIXED = 15,
  /* Q5 + the terminal value (node.cpp:31-42, mcts.py:20-25).  Independent of the four bits above; when a descent ends on
   * a leaf whose GetGameResult is not FPC_IN_PROGRESS:
   *   value   backed up along the path, leaf first, sign alternating as ever: 0 for FPC_STALEMATE, else +1 if the winning
   *           team (FPC_WIN_RY -> 0, FPC_WIN_BG -> 1) is the leaf's side-to-move team (turn & 1), else -1 (clear: 0 / -1,
   *           which calls "its first legal move takes a king" a loss of the side to move);
   *   search  the game STAYS in the search (clear: it leaves it).  The row is dead for this step, sims_done += 1, a
   *           leaf-parallel step's selection of that game ends there with no pending visit added, and the next step
   *           selects again; every further visit of the same terminal leaf backs up again (N += 1, W += +-v).  No second
   *           descent within a step.  A terminal ROOT still leaves the search (it can never have a child), with the value
   *           above.  Budgets and max_sims count terminal backups as before.
   * After a search, alive == 0 then means an error or a terminal root. */
  FPC_RULES_TERMINAL = 16,
  FPC_RULES_TRAINING = 31,   /* FPC_RULES_FIXED | FPC_RULES_TERMINAL */
  /* Q1 (node.h:28): N counts backups; every node is born with N = 0.  Independent of the five bits above and may be
   * combined with any of them, strict included.  fpc_abi_version() is unchanged: additions only.
   *   birth      every node is born with N = 0, W = 0 (clear: N = 1): the children an expansion makes, a fresh root
   *              (fpc_search_begin), a fresh row of fpc_search_advance_refill and the childless root a failed advance leaves.
   *   invariant  a node's N is the number of backups through it -- the completed simulations whose path held it,
   *              expansions plus terminal backups.  After a fresh search in which game g completed s simulations
   *              root_visits[g] == sims_done[g] == s, and if the root was expanded the children's visits sum to s - 1 (the
   *              first simulation expanded the root itself).
   *   selection  the arithmetic is unchanged: both formulas read q = 0 where N' == 0 (but see fpc_search_set_fpu), 1 + N'
   *              keeps the exploration term finite, and a node with children has N >= 1, so log(sqrt(0)) is never read.
   *              Under strict rules the first descent below a root with N = 1 sees log(sqrt(1)) = 0 and the lowest index
   *              wins: specified, not an error.  Virtual loss, collisions, terminal backups (FPC_RULES_TERMINAL: N += 1 on
   *              every repeat), root noise, both policy heads and live rows are as specified above; none mentions the
   *              birth count.
   *   reuse      a never-selected child has N = 0; re-rooted on it the game is in the state of a fresh root.  kept_visits[i]
   *              is the new root's N as before -- now "simulations through it", 0 for a fresh row and for a never-visited
   *              child -- and the host's accounting follows: max_i kept_visits[i] simulations count as issued, and
   *              fpc_search_set_budget's base[g] = kept_visits[g] (clear: both - 1).  Its capacity rule reads
   *              base[g] + budget[g] > max_sims unchanged.
   *   play       fpc_search_play's weights are powtab[N_k], powtab[0] = 0 for every temperature > 0.  If S == 0 -- no child
   *              has a visit; unreachable with the bit clear -- the pick is child min(nc - 1, (int)(uniform * nc)).  At
   *              temperature 0 the first child with the largest N already gives child 0.
   *   tuples     fpc_collect_tuples stores all nc pairs, with a visit count of 0 where there were none; a record whose
   *              visits sum to 0 decodes to a zero pi row (fpc_replay_batch and tuples.dense_pi alike). */
  FPC_RULES_VISITS = 32,
  FPC_RULES_SELFPLAY = 63    /* FPC_RULES_TRAINING | FPC_RULES_VISITS */
};
/* The five bits above: rules 0..31 (FPC_EINVAL outside, as ever; the call clears FPC_RULES_VISITS). */
int fpc_set_rules(fpc_engine *e, int rules);
/* All six bits: rules 0..63 (additions only, fpc_abi_version() unchanged).  fpc_set_rules keeps the range it always had --
 * a caller that relied on 32 being refused still gets FPC_EINVAL -- and every rule set with FPC_RULES_VISITS goes through
 * this call; for 0..31 the two calls are the same.  FPC_EINVAL (no state changed): null engine, rules outside 0..63. */
int fpc_set_rule_bits(fpc_engine *e, int rules);
/* ---- first-play urgency (opt-in; additions only, fpc_abi_version() unchanged) ---------------------------------------
 * The value the descent gives a child whose effective count N' = N + VL is 0, in the FPC_RULES_PUCT branch only (the
 * strict branch keeps q = 0):
 *   FPC_FPU_ZERO    (default) q = 0: the arithmetic as it always was;
 *   FPC_FPU_PARENT  q = W_p / (double)N_p - reduction, W_p and N_p the STORED statistics of the node the descent stands on
 *                   (no virtual loss goes into them; N_p >= 1 because the node has children), f64 without contraction,
 *                   evaluated as written: the node's value seen by its own side to move, the frame -W_c / N_c already uses
 *                   for a visited child.  A child with N' > 0 is untouched.
 * Without FPC_RULES_VISITS every child is born with N = 1, no child ever has N' == 0 and the setting has no effect; it is
 * accepted all the same.  Persistent, like fpc_search_set_leaves; applies from the next selection.
 * FPC_EINVAL (no state changed): null engine, mode outside 0..1, reduction not finite. */
enum { FPC_FPU_ZERO = 0, FPC_FPU_PARENT = 1 };
int fpc_search_set_fpu(fpc_engine *e, int mode, double reduction);
/* Root noise for the NEXT searches (mcts.py:45-56 defines add_dirichlet_noise and never calls it):
 * prior'_j = (1 - eps) prior_j + eps g_j / sum_k g_k over the root's legal moves j in ascending flat order,
 * gamma: host array [n_games][FPC_MAX_MOVES] of Gamma(alpha, 1) draws made (and seeded) by the caller;
 * NULL switches the noise off. */
int fpc_search_set_root_noise(fpc_engine *e, const float *gamma, int n_games, float eps);
/* ---- leaf-parallel search (opt-in, held against a model of these semantics, not against the reference) ----------
 * Each simulation step selects up to `leaves` = K leaves per game instead of one, kept apart by virtual loss, so the
 * network sees up to K*G rows.  Row r = k*G + g holds the k-th leaf game g selected in this step (K = 1: today's
 * layout, today's kernels).  The descent sees N' = N + VL and W' = W - vl*VL (strict) / W + vl*VL (FPC_RULES_PUCT),
 * VL = pending visits of the step; a descent that ends on a pending leaf (a collision) or on a terminal leaf ends the
 * game's selection for the step.  Expansion walks a game's live rows in ascending k.  fpc_search_run(sims) runs
 * ceil(sims/K) steps, the last of the remainder; every leaf counts against max_sims.
 * Persistent; may be changed between the steps of a running search (it applies to the NEXT selection).  Step-wise
 * callers: *n_live counts live rows, enc_dev is [K*G,24,R,R], logits_dev / value_dev have K*G rows.
 * FPC_EINVAL: leaves outside 1..FPC_MAX_LEAVES, virtual_loss negative or not finite, K*G > max_games (rows must fit:
 * checked here during a running search, at fpc_search_begin, and by every call that selects leaves). */
#define FPC_MAX_LEAVES 8
int fpc_search_set_leaves(fpc_engine *e, int leaves, double virtual_loss);

/* ---- subtree reuse (opt-in, held against a model of these semantics, not against the reference, which builds a fresh
 * tree for every ply) ---------------------------------------------------------------------------------------------
 * Re-roots the FINISHED search (fpc_search_results has been read; otherwise FPC_ESTATE) on the moves played: new game i
 * continues old game src_game[i] (NULL: game i) from the root child whose move is flat[i], and the engine is then in the
 * state fpc_search_begin leaves it in, with G = n_games: fpc_search_run or the step entry points continue the search.
 * The child becomes the root (its N and W as they are) and keeps its whole subtree -- N, W, P, moves, the children's
 * order, every materialised state; the rest of the old tree is dropped.  The new root's state is made from the old
 * root's by the move if the child was never selected (every child starts with N = 1, Q1), without a GetGameResult /
 * legal-moves pass.  Per game: alive, no error, sims_done = 0.
 * Budget: a root kept with N = n has had n - 1 simulations through it, so the call counts max_i(kept_visits[i]) - 1
 * simulations as issued; kept + new simulations beyond max_sims give FPC_ECAPACITY as after fpc_search_begin (create the
 * engine with max_sims = 2 x the per-ply simulations to be safe).
 * Root noise, if set: applied here to the children of an already expanded new root (child i, in ascending flat
 * order, takes the i-th draw of its game's row; the arithmetic of the expansion); an unexpanded root gets it when it is expanded.
 * Leaf-parallel: no pending visit survives.  The work is done out of place (games move to lower indices): the first call
 * allocates a second set of tree arrays and a second board pool (FPC_ENOMEM if that fails).
 * FPC_EINVAL: src_game not strictly ascending within 0..G-1 (ascending keeps the reference's delete-from-the-list
 * batch order, which the batch-wide rotation Q6 depends on), n_games < 1, leaves * n_games > max_games, root noise set
 * for another number of games.  A flat[i] that is no root child of src_game[i] kills that game with its error set, and
 * the call returns FPC_EMOVE after advancing the others.
 * roots_out (nullable): the new root states; kept_visits (nullable): the new roots' visit counts. */
int fpc_search_advance(fpc_engine *e, const int *src_game /* nullable: 0..n_games-1 */, const int *flat,
                       int n_games, fpc_board *roots_out /* nullable */, int *kept_visits /* nullable */);
/* ---- subtree reuse with refill (opt-in; additions only, fpc_abi_version() unchanged) ---------------------------------
 * fpc_search_advance that also STARTS games, in the same single launch: a self-play batch stays full when a finished
 * game's row is handed to a new start position while the other rows keep their subtrees.  Needs a finished search,
 * exactly as fpc_search_advance does (FPC_ESTATE otherwise).  New game i is one of two kinds:
 *   src_game[i] >= 0:  it continues old game src_game[i] from the root child whose move is flat[i]; everything
 *                      fpc_search_advance specifies holds word for word (the kept subtree, the state of a never-selected
 *                      child, root noise on an expanded new root, FPC_EMOVE for a move that is no root child after the
 *                      others are advanced, the out-of-place work);
 *   src_game[i] == -1: a fresh root on fresh[i], in the state fpc_search_begin leaves a game in: N = 1, W = 0, no
 *                      children, board slot 0 = fresh[i], one node, one board, alive, no error, sims_done = 0, no leaf and
 *                      no pending visit; kept_visits[i] = 1, roots_out[i] = fresh[i], flat[i] is ignored.  Root noise, if
 *                      set, reaches the root when it is expanded, from row i.
 * src_game == NULL means identity: the call is fpc_search_advance.  fresh entries at kept positions are not read, and
 * fresh may be NULL when there is no -1.  Old games that nobody names are dropped.  A kept game may land at a higher
 * index than it had as well as at a lower one.  n_games may exceed the finished search's game count, up to
 * max_games / leaves.  Afterwards the engine is in the state fpc_search_begin / fpc_search_advance leave it in, with
 * G = n_games; max_i(kept_visits[i]) - 1 simulations count as issued (a fresh root contributes 0), and every row, fresh
 * or kept, shares what is left of max_sims.
 * FPC_EINVAL (nothing is uploaded or launched, the finished search stays as it was): the non-negative entries of
 * src_game are not strictly ascending among themselves; an entry < -1 or >= G; a -1 with fresh == NULL; a fresh board
 * fpc_search_begin would refuse; n_games < 1; leaves * n_games > max_games; root noise uploaded for another number of
 * games. */
int fpc_search_advance_refill(fpc_engine *e, const int *src_game /* nullable */, const int *flat,
                              const fpc_board *fresh /* host [n_games], nullable */, int n_games,
                              fpc_board *roots_out /* nullable */, int *kept_visits /* nullable */);
/* ---- per-game simulation budgets (opt-in; additions only, fpc_abi_version() unchanged) ------------------------------
 * fpc_search_run(sims) and the step entry points give every game of the batch the same number of simulations.  A budget
 * caps them per game: budget[g] bounds sims_done[g], the simulations game g COMPLETES in this search (expansions plus
 * terminal backups: the number fpc_search_results reports).  A game whose sims_done has reached its budget selects no
 * leaf: its row is dead for the step (leaf_node = leaf_slot = -1), exactly as the row of a root that Q5 removed is,
 * and nothing else about the game changes -- it stays alive, carries no error, and nothing in its tree, its pools or its
 * counters is written.  Leaf-parallel search: descent k (0-based) of a step is made only while
 * sims_done[g] + k < budget[g], with sims_done as it stands when the step's selection starts; the game's remaining rows
 * of the step are dead rows.  The gate is exact: a game never completes more than budget[g] simulations, also when K does
 * not divide it; budget[g] == 0 selects nothing.
 * Applies to the search in progress: call it after fpc_search_begin, fpc_search_advance or fpc_search_advance_refill and
 * before that search's first selection.  budget == NULL clears the budgets; so does every later fpc_search_begin /
 * fpc_search_advance(_refill): budgets belong to one ply.
 * Step counts stay the caller's: fpc_search_run(sims) still runs ceil(sims / K) steps and the step entry points as many
 * as they are called for -- the budget only idles rows, so pass max_g budget[g]; further steps are harmless (every row is
 * dead).  Under strict rules the batch-wide rotation (Q6) is that of the first LIVE row; a budget-idle row is not live.
 * Capacity is per game while budgets are set.  base[g] = kept_visits[g] - 1 after an advance (0 for a fresh row) and 0
 * after fpc_search_begin; FPC_ECAPACITY when base[g] + budget[g] > max_sims for some g (the message names the first such
 * game; nothing changes).  While budgets are set the selecting calls do not apply the batch-wide
 * "issued + n <= max_sims" check: each game is bounded by its own budget, which is what the log table, the node pool, the
 * board pool and the path buffer need.  fpc_search_run still refuses sims > max_sims.
 * FPC_ESTATE: no search in progress; a selection has been issued since the last begin / advance; a finished search whose
 * results have been read and which was not advanced (reading the results right after a begin / advance, before any
 * selection, changes nothing and closes nothing).  FPC_EINVAL (nothing uploaded, no state changed): null engine,
 * n_games != the search's game count, a negative entry. */
int fpc_search_set_budget(fpc_engine *e, const int *budget /* host [n_games], nullable */, int n_games);

/* ---- live-row numbering (opt-in; additions only, fpc_abi_version() unchanged) -----------------------------------------
 * Refill, budgets, FPC_RULES_TERMINAL and leaf-parallel collisions leave dead rows in a step, and with the switch off a
 * dead row is evaluated like a live one.  With it on, every selection's live rows (leaf_node[r] >= 0, r = k*G + g) are
 * numbered j = 0..n_live-1 IN ASCENDING r on the device (k_live_rows), and everything between the selection and the
 * expansion works on that numbering: the network's row j is the j-th live leaf.  The trees are the same bit for bit --
 * fpc_search_results, fpc_search_grandchildren, sims_done, alive and the error words do not change under any rule set,
 * K, budget, reuse, refill, root noise or policy head: a row's network output is a function of that row's input and the
 * weights alone, and under strict rules the batch-wide rotation (Q6) is that of the first live row, which is row 0 of
 * the numbering.  Only where a leaf's row lies in the network batch changes.
 *   fpc_search_run     the policy Linear computes ceil(n_live / 256) row tiles instead of ceil(rows / 256): a batch of
 *                      more than 256 slots whose live leaves fit one tile streams the weights once.
 *   step entry points  *n_live as before; enc_dev is [rows,24,R,R] with the live leaves in rows 0..n_live-1 (ascending
 *                      r) and rows n_live.. all-zero; logits_dev / value_dev are read at rows 0..n_live-1 ONLY (buffers
 *                      of n_live rows are enough).  With *n_live == 0 nothing needs evaluating, as before.
 *   fpc_nn_forward     untouched.
 * Persistent, like fpc_search_set_leaves; applies from the next selection.  May be called before fpc_search_begin, after
 * fpc_search_begin / fpc_search_advance(_refill) and before that search's first selection, and on a finished search.
 * FPC_ESTATE: a selection has been issued and the search's results have not been read (fpc_search_set_budget's rule).
 * FPC_EINVAL: null engine, `on` outside 0..1.  The first call with on = 1 allocates 4 * max_games + 1 ints. */
int fpc_search_set_live_rows(fpc_engine *e, int on);

/* ---- MCTS solver (opt-in; additions only, fpc_abi_version() unchanged; held against tests/solver_model.py) -------------
 * FPC_RULES_TERMINAL lets a search go on past terminal leaves, but a terminal leaf reached again is materialised, judged
 * and averaged into W / N again.  With the solver every node carries one byte of proof status, seen from the node's OWN
 * side to move -- the frame of the terminal value v: */
enum { FPC_PROOF_UNKNOWN = 0, FPC_PROOF_WIN = 1, FPC_PROOF_LOSS = 2, FPC_PROOF_DRAW = 3 };
/* The proven value pv is +1 for WIN, -1 for LOSS, 0 for DRAW.  The proof is over the TREE's children: the legal moves whose
 * prior was not flushed to exactly zero, judged by the engine's GetGameResult (Q13 included).
 * The solver is IN EFFECT only while the switch is on and the rule set holds both FPC_RULES_PUCT and FPC_RULES_TERMINAL;
 * under any other rule set the call is accepted and changes nothing (fpc_search_set_fpu's convention).  In effect, one
 * descent of game g is today's except for:
 *   1. proven root      a root that has children and a status other than 0: the row is dead and nothing is written --
 *                       exactly a budget-idle row; the game stays alive, carries no error, sims_done does not move.  A
 *                       childless root takes today's path, a terminal root leaves the search as ever.
 *   2. excluded child   among the children of the node the descent stands on, a child with status WIN (the move that loses)
 *                       is no candidate.  The argmax over the others is the arithmetic as it is: strict >, lowest index on
 *                       ties, the FPU q0 unchanged.  No candidate gives FPC_ESELECT as ever (unreachable while (a) holds).
 *   3. proven backup    a chosen child with a status other than 0 ends the descent: pv(status) is backed up from that node
 *                       along the path, leaf first, sign alternating, N += 1 each; sims_done += 1; the row is dead, no
 *                       pending visit is added and the game's selection of the step ends there -- the bookkeeping of a
 *                       terminal backup, counted by budgets and max_sims the same way, without board materialisation,
 *                       GetGameResult or move generation.  The check comes before the collision check.
 *   4. marking          a descent that ends on an unknown leaf whose GetGameResult is not in progress makes today's terminal
 *                       backup, then sets the leaf's status from v (+1 WIN, -1 LOSS, 0 DRAW) and propagates: with c the node
 *                       just proven and p its parent, stop if there is no parent or p is proven already; if c is LOSS, p
 *                       becomes WIN; otherwise stop if any child of p is unknown, else p becomes LOSS if all are WIN and
 *                       DRAW if not; continue with p as c.  A status never changes once it is set.
 * Invariants: (a) an unknown node with children has at least one unknown child; (b) a proven non-root node is never
 * descended through; (c) under leaf-parallel search a proof ends the game's selection of the step, so no descent of the
 * same step sees it and a proven node has VL == 0 when a descent reaches it -- rows of the same step that are pending below
 * a node proven later are expanded and backed up as ever.
 * Lifetime: fpc_search_begin clears the statuses; fpc_search_advance(_refill) carries them with the subtree (in the second
 * tree set, beside N / W / P), fresh rows and the childless root of a failed advance get 0 -- whenever the arrays exist,
 * switch on or off.  A new root that is proven and has children is idle from the first step; its kept_visits is as ever.
 * fpc_search_play with the solver in effect: a root proven WIN plays its first child with status LOSS, a root proven DRAW
 * its first child with status DRAW, at every temperature; a root proven LOSS or unknown takes today's draw.  Everything
 * after the pick (the move, the result, next_out) is unchanged.
 * Unchanged on purpose: fpc_collect_tuples stores the visit counts as they are, fpc_search_run does not end early when
 * every row is idle.
 * fpc_search_set_solver is persistent, like fpc_search_set_leaves, and follows fpc_search_set_live_rows' call-sequence
 * rule.  FPC_ESTATE: a selection has been issued and the search's results have not been read.  FPC_EINVAL: null engine,
 * `on` outside 0..1.  The first on = 1 allocates the status arrays (one byte per node; for both tree sets once the second
 * exists), zeroed; FPC_ENOMEM if that fails. */
int fpc_search_set_solver(fpc_engine *e, int on);
/* The statuses of each root and of its children in the tree's child order (the order fpc_search_results reports), entries
 * past a root's children 0.  Follows the rules of fpc_search_results (FPC_ESTATE before any fpc_search_begin, FPC_EINVAL
 * for a negative max_children); does not finish a search.  All zero if the solver was never switched on. */
int fpc_search_proofs(fpc_engine *e, int max_children, uint8_t *root_proof /* host [G] */,
                      uint8_t *child_proof /* host [G][max_children], nullable */);

/* ---- forced playouts and policy target pruning at the root (opt-in; additions only, fpc_abi_version() unchanged; held
 * against tests/forced_model.py) ----------------------------------------------------------------------------------------
 * Root Dirichlet noise (fpc_search_set_root_noise) distorts the training target twice: a noised move gets too few
 * simulations to show that it is good, or it gets simulations that PUCT alone would never have spent and that go straight
 * into the visit counts.  KataGo's pair: a visited root child is guaranteed sqrt(factor * P * N) simulations, and when the
 * target is read the visits that only the forcing put there are taken out again.  Both are root-only, need no per-node
 * state and are computed from the stored statistics.
 * factor == 0: off (the default).  factor > 0: both, with that k (KataGo uses 2).  IN EFFECT only while the factor is > 0
 * and the rule set holds both FPC_RULES_PUCT and FPC_RULES_VISITS (without FPC_RULES_VISITS every child is born with N = 1
 * and "has been visited" means nothing); under any other rule set the call is accepted and changes nothing
 * (fpc_search_set_fpu's convention).
 * SELECTION, in effect, at the ROOT level of a descent only (the node the descent stands on is node 0).  For child i with
 * effective count N' = N + VL, prior P (f32) and the root's effective count Nn (the value sqrtNp is made from):
 *     nf_i = sqrt(factor * (double)P_i * (double)Nn)          f64, as written
 *     if (N'_i > 0 && (double)N'_i < nf_i)  u_i = +infinity
 * Everything else is the arithmetic as it is: strict >, the lowest index wins, also across the passes of 64 children, so
 * among several forced children the first is taken.  A child with N' == 0 is never forced (FPU and q = 0 decide it as
 * ever).  A child the solver excludes (status WIN) stays excluded even if forced; a forced child that is proven ends the
 * descent with a proven backup, as any chosen proven child does.  A forced descent is an ordinary simulation for budgets,
 * max_sims, virtual loss, collisions and terminal backups.  Below the root nothing changes.
 * TARGET, per game, from the root's STORED N_p and its children's stored N_k, W_k, P_k (k in tree order) and the search's
 * c_puct as C; f64 throughout, no contraction, evaluated as written:
 *     b  = first k with the largest N_k;   T_b = N_b;   if N_b == 0: T_k = N_k for all k, done
 *     sq = sqrt((double)N_p)
 *     ub = -(W_b / (double)N_b) + C * (double)P_b * sq / (double)(1 + N_b)
 *     for k != b:  T = N_k
 *       if N_k > 0:
 *         F = (int)sqrt(factor * (double)P_k * (double)N_p)
 *         q = -(W_k / (double)N_k);   a = C * (double)P_k * sq
 *         repeat at most F times:  if T == 0 or q + a / (double)T >= ub: stop;  T = T - 1
 *             (u of the child at count T - 1 with q held fixed; 1 + (T - 1) == T)
 *         if T < N_k and T <= 1: T = 0            (a child reduced to a single playout is pruned outright)
 *       T_k = T
 * CONSUMERS, in effect: fpc_collect_tuples stores T_k where it stores N_k; fpc_search_play draws from powtab[T_k] (the
 * argmax is unchanged in outcome: T_b = N_b is still the first largest) and the solver's pick still overrides the draw;
 * fpc_search_results and fpc_search_grandchildren keep reporting the stored counts.  The target is computed when it is
 * read: nothing is written into the tree.
 * fpc_search_set_forced is persistent, like fpc_search_set_leaves, and follows fpc_search_set_live_rows' call-sequence
 * rule.  FPC_ESTATE: a selection has been issued and the search's results have not been read.  FPC_EINVAL (no state
 * changed): null engine, a factor that is negative or not finite. */
int fpc_search_set_forced(fpc_engine *e, double factor);
/* The pruned visit counts T_k of each root's children in the tree's child order (the order fpc_search_results reports),
 * entries past a root's children 0; the stored visit counts when forcing is not in effect.  Follows the rules of
 * fpc_search_results (FPC_ESTATE before any fpc_search_begin, FPC_EINVAL for a negative max_children); does not finish a
 * search. */
int fpc_search_targets(fpc_engine *e, int max_children, int *child_target /* host [G][max_children] */);

/* ---- playout cap randomization: per-game fast searches (opt-in; additions only, fpc_abi_version() unchanged; held against
 * tests/playout_cap_model.py) ---------------------------------------------------------------------------------------------
 * KataGo pairs forced playouts and target pruning with playout cap randomization: each ply, each game draws either a FULL
 * search (N simulations, root noise, forcing; its policy target is trained) or a FAST search (n << N simulations, no noise,
 * no forcing; no policy target is taken from it).  Games finish sooner for the same network evaluations, every position
 * still gets a value target, and the policy targets that remain all come from full-strength searches.  The simulation
 * counts are fpc_search_set_budget's, dead rows cost nothing under fpc_search_set_live_rows; this call is the rest.
 * fast[g] != 0: game g's search of THIS ply is a fast search.  IN EFFECT for game g while the mask is set and fast[g] == 1;
 * a full row (fast[g] == 0, or no mask) behaves bit for bit as without the call.
 *   SELECTION  the forced-playout rule (fpc_search_set_forced) is not applied to game g, at any leaf k of a leaf-parallel
 *              step; all other arithmetic is unchanged.
 *   TARGET     the pruning is not applied to game g: fpc_search_targets reports the stored N_k, fpc_collect_tuples stores
 *              N_k, fpc_search_play draws from powtab[N_k]; the solver's pick still overrides the draw.
 *   RECORD     fpc_collect_tuples sets FPC_TUPLE_FAST in fpc_tuple::flags, whether or not forcing is in effect.
 *   NOISE      is not the engine's business: k_tree_advance blends the noise inside the advance launch, before a mask can
 *              be set.  The caller hands a fast row an all-zero gamma row (fpc_search_set_root_noise: a row whose sum is
 *              not positive keeps its priors un-noised).
 * Budgets, live rows, first-play urgency, the solver's statuses, virtual loss, fpc_search_results,
 * fpc_search_grandchildren and sims_done do not change.
 * The call sequence is fpc_search_set_budget's: the mask belongs to one ply; call it after fpc_search_begin,
 * fpc_search_advance or fpc_search_advance_refill and before that search's first selection.  fast == NULL clears the mask,
 * and so does every later fpc_search_begin / fpc_search_advance(_refill).  FPC_ESTATE as for fpc_search_set_budget.
 * FPC_EINVAL (nothing uploaded, no state changed): null engine, n_games != the search's game count, an entry above 1.
 * The first call allocates max_games bytes. */
int fpc_search_set_fast_rows(fpc_engine *e, const uint8_t *fast /* host [n_games], nullable */, int n_games);

/* ---- device-side move choice (opt-in): what a self-play ply does between the finished search and fpc_search_advance /
 * the next fpc_search_begin -- choose each game's move from the root's visit counts (alphazero.py:104-118), make it
 * (TakeAction, :119) and judge the game (GetGameResult, :120-123) -- as ONE launch (k_play_ply, one wave per game); the
 * host sees two ints per game.  Needs a FINISHED search, exactly as fpc_search_advance does (fpc_search_results has been
 * read -- with every array NULL it reads the error words and nothing else; otherwise FPC_ESTATE).  Reads the tree and
 * writes nothing into it (no N, W, P, pooled board, alive, err or sims_done changes): the same call with the same
 * arguments returns the same outputs, and fpc_collect_tuples, fpc_search_advance and fpc_search_begin may follow in any
 * order.
 * THE DRAW, per game g with children k = 0..nc-1 in the tree's child order (the order fpc_search_results reports):
 *   temperature > 0:  w_k = powtab[N_k], powtab[v] = pow((double)v, 1.0 / temperature) for v = 0..max_sims+15, computed by
 *                     the HOST libm (as the PUCT log table is) and uploaded when the temperature differs from the cached
 *                     one; the device evaluates no transcendental.  c_k = c_{k-1} + w_k in f64, strictly left to right
 *                     (one lane walks the at most 256 adds; no wave scan, which would round differently off temperature
 *                     1); S = c_{nc-1}; x = uniform[g] * S (one f64 multiply); the pick is the first k with c_k > x, or
 *                     nc-1 if there is none.  At temperature 1 every term is an integer and the arithmetic is exact.
 *   temperature == 0: the first child with the largest N (arena.py's rule).
 * THE MOVE: next = the root state (board slot 0) copied, the move made, GetGameResult run for the side to move, under
 * the engine's current rule set: flat_out, result_out and next_out are bit for bit what fpc_search_results(roots_out) ->
 * fpc_boards_take_action(roots, flat) -> fpc_boards_game_result(next, NULL) give for the picked moves, the piece-list
 * order GetGameResult leaves behind included.
 * A game that carries a search error or has a childless root (a root that is terminal, or that a failed
 * fpc_search_advance left behind) gets flat_out = -1, result_out = -1 and next_out = its root state.  A game whose
 * root merely left the search early because a simulation reached a terminal leaf (Q5) has children and is played like
 * any other, as the host loop plays it.  A move that cannot be made is reported as fpc_boards_take_action reports it
 * (FPC_EMOVE, "game i: piece missing for move") after the other games are done; it is tracked in an array of the call's
 * own, never in the search's error words.
 * FPC_EINVAL (nothing is uploaded or launched): uniform, flat_out or result_out NULL; a uniform that is NaN or outside
 * [0, 1); a temperature that is negative, NaN or infinite, or for which pow(max_sims + 15, 1 / temperature) is not
 * finite (use 0 for argmax). */
int fpc_search_play(fpc_engine *e, double temperature, const double *uniform /* host [G] */,
                    int *flat_out /* host [G] */, int *result_out /* host [G] */,
                    fpc_board *next_out /* host [G], nullable */);

/* Root read-back == what alphazero.py:104-110 reads through Node.GetChildren /
 * GetMoveMade().GetFlatIndex() / GetVisitCount().  Arrays are [n_games][max_children].
 * roots_out (nullable): the root states with the piece-list order the search left them in. */
int fpc_search_results(fpc_engine *e, fpc_board *roots_out, int *root_visits, int *n_children, int *sims_done,
                       int max_children, int *child_flat, int *child_visits, float *child_prior,
                       double *child_value_sum);
/* children of root child `child_idx` of game `game` (second tree level, for parity tests) */
int fpc_search_grandchildren(fpc_engine *e, int game, int child_idx, int max_children, int *n,
                             int *flat, int *visits);

/* ---- internal ResNet (net.py:6-63), BN folded, MFMA implicit-GEMM ------------------------ */
/* blob format: see alphazero-4-player-chess_amd/weights.py (header + folded tensors) */
int fpc_load_weights(fpc_engine *e, const void *blob, uint64_t nbytes);
/* forward only: enc_dev [n,24,R,R] f32 -> logits_dev [n,A] f32, value_dev [n] f32 (DEVICE pointers) */
int fpc_nn_forward(fpc_engine *e, const float *enc_dev, int n, float *logits_dev, float *value_dev);

/* ---- device-side weight pack: the network refreshed from the LIVE torch module, without a host blob ------------------
 * Hand-written kernels (csrc/fpc_pack.h) read the module's fp32 parameters where they lie in device memory and write the
 * sections of the version-3 blob -- BN fold (weights._fold op for op in f32), fp32 -> the engine's 16-bit type (round to
 * nearest even, subnormals kept), the policy Linear's NCHW -> NHWC input permutation, zero padding and MFMA fragment
 * order -- what weights.export_weights produces, computed op for op in f32 with correctly rounded divide and square root.
 * (Byte for byte the same blob wherever torch's CPU sqrt is correctly rounded too; on builds where it is one unit off for
 * some variances -- DESIGN 7.3 -- the HOST blob deviates from this spec in those BatchNorm channels.)  Every pointer of the descriptor is DEVICE memory (host
 * memory in the emulator build, as with fpc_replay_batch), fp32, contiguous. */
typedef struct fpc_conv_src {     /* one Conv2d(3x3, padding 1) + BatchNorm2d */
  const float *w;                 /* [cout][cin][3][3] */
  const float *b;                 /* [cout], nullable = zeros */
  const float *bn_weight, *bn_bias, *bn_mean, *bn_var;   /* [cout] each */
  float eps;                      /* (float)bn.eps: torch adds it in f32 */
  int cin, cout;
} fpc_conv_src;
typedef struct fpc_net_src {
  int hidden, nblocks;
  fpc_conv_src stem, pconv, vconv;
  const fpc_conv_src *c1, *c2;    /* HOST arrays [nblocks] of descriptors */
  const float *fc_w, *fc_b;       /* policy Linear [A][A] (input index ch*RR+pos, torch's NCHW flatten), [A] */
  const float *vfc_w, *vfc_b;     /* value Linear [24*RR], [1] */
} fpc_net_src;
/* fc_layout: 1 or 2 as in the blob header; 0 = what weights.default_fc_layout(R) chooses (2 where k_fcw has a one-round
 * K-split on this device, else 1).  The dtype is the engine's nn_dtype.
 * All three calls launch on the engine's stream, which is synchronised before they return; the caller must have finished
 * whatever wrote the parameters (the Python binding synchronises torch's current stream first).
 * Errors -- nothing is launched, and the loaded network stays as it was and stays usable:
 *   FPC_EINVAL    NULL engine, descriptor or required pointer; cin / cout that do not fit the engine's board (stem 24 ->
 *                 hidden, blocks hidden -> hidden, policy conv hidden -> A_ch, value conv hidden -> 24); cap too small;
 *                 blob_dev not 16-byte aligned; fc_layout outside 0..2;
 *   FPC_EWEIGHTS  a shape fpc_load_weights would refuse (hidden not a multiple of 64 or outside 64..512, layout 2 without
 *                 a one-round split), with its messages.
 * Every hidden width these calls and fpc_load_weights accept -- 64, 128, ..., 512 -- forwards: 128 and 256 on the tower
 * kernels, every other one on k_conv3x3 per layer (192 / 320 / 448 as slabs of 64 input channels, 384 / 512 as slabs of
 * 128).  Held by tests: hidden 64 on every board of 8..14 a side and hidden 192..512 at 8x8 element by element
 * (tests/test_tower_probe_gpu.py), all eight widths through load + forward (tests/test_nn_gpu.py). */
/* size of the blob such a network packs into */
int fpc_weights_blob_size(const fpc_engine *e, int hidden, int nblocks, int fc_layout, uint64_t *nbytes);
/* header + sections (64-byte aligned, order and padding of csrc/fpc_nn.h's blob comment) into blob_dev[0..cap); exists in
 * the emulator build too.  nbytes (nullable): the blob's size. */
int fpc_weights_pack(fpc_engine *e, const fpc_net_src *src, int fc_layout, void *blob_dev, uint64_t cap, uint64_t *nbytes);
/* fpc_load_weights without a host blob.  Same geometry as the loaded network (hidden, nblocks, Np, Kp, fc_layout): packs
 * straight into the live weight allocations, re-derives the tower kernels' weight streams and the legal-only head's
 * row-major copy in place and reads the value bias back (4 bytes) -- no hipFree, no hipMalloc.  First load or another
 * geometry: allocates exactly as fpc_load_weights does, then packs.  Emulator build: FPC_EWEIGHTS, as fpc_load_weights. */
int fpc_load_weights_device(fpc_engine *e, const fpc_net_src *src, int fc_layout);
/* ---- opt-in int8 weights for the policy Linear (blob version 4, kernel k_fcw8) -- the default stays 16 bit.
 * Weight type of the policy Linear for the NEXT size / pack / device-load call above (a host blob given to the plain load
 * call carries its own type in the header).  Persistent.  FPC_EINVAL: null engine, type outside 0..1.
 * With FPC_FC_W8 those three calls return FPC_EWEIGHTS on a bf16 engine or where fc_layout resolves to 1, and the pack
 * and the device load return FPC_EWEIGHTS -- nothing written, the loaded network as it was -- if the policy Linear holds
 * a non-finite weight. */
enum { FPC_FC_W16 = 0, FPC_FC_W8 = 1 };
int fpc_set_fc_weight_type(fpc_engine *e, int type);
/* "k_fcw8" | "k_fcw" | "k_fc16" | "" before a load: the kernel that runs the policy Linear for the loaded weights */
const char *fpc_nn_fc_kernel(fpc_engine *e);
/* HIP-event time of the pack kernels of the last fpc_weights_pack / fpc_load_weights_device made with fpc_set_timing on
 * (else FPC_ESTATE) */
int fpc_weights_pack_ms(fpc_engine *e, float *ms_out);

/* ---- training tuples and their episode-end exchange ---------------------------------------
 * The reference keeps (state, pi, z) tuples as Python objects: Board::AppendToMemory(MemoryEntry(state,
 * action_probs)) per ply (alphazero.py:104-112), rewards assigned when the game ends
 * (handle_terminal_state, alphazero.py:53-78; heuristic scoring at max_game_length, :161-175).  Here a
 * tuple is a fixed-size POD built ON THE DEVICE from the finished search (root mailbox + side to move +
 * sparse pi = the root's (child flat index, visit count) pairs) and kept in a device buffer until the
 * episode ends.  Dense reference-shaped tensors (GetEncodedState [24,R,R], pi [A] = N / sum N) are
 * rebuilt from it on receipt (alphazero-4-player-chess_amd/tuples.py). */
#define FPC_TUPLE_MAXC 256
typedef struct fpc_tuple {
  uint8_t sq[FPC_MAX_SQ];        /* root mailbox (piece bytes as in fpc_board) */
  uint8_t turn;                  /* side to move at the root */
  uint8_t flags;                 /* FPC_TUPLE_* bits; 0 unless fpc_search_set_fast_rows marked the game */
  uint16_t n;                    /* number of (flat, visits) pairs */
  float z;                       /* filled by fpc_tuples_set_z */
  int32_t game, ply;             /* caller's game id and ply */
  uint16_t flat[FPC_TUPLE_MAXC];
  uint16_t visits[FPC_TUPLE_MAXC];
  uint8_t pad1[44];
} fpc_tuple;                     /* sizeof == 1280 */
enum { FPC_TUPLE_FAST = 1 };     /* fpc_tuple::flags: the record comes from a fast search (fpc_search_set_fast_rows): its visit
                                  * counts are the stored N_k of a short search without noise, no policy target for training */
int fpc_tuples_reserve(fpc_engine *e, int capacity);    /* device buffer for `capacity` tuples; drops collected ones */
int fpc_tuples_reset(fpc_engine *e);                    /* new episode: count = 0 */
/* after a finished search (fpc_search_run / the select-expand loop): one tuple per game of that search,
 * appended in game order.  game_id: host array [n_games] (NULL: 0..n_games-1). */
int fpc_collect_tuples(fpc_engine *e, const int *game_id, int ply);
/* z of every collected tuple whose game is game_id[i]: z_team[i][side-to-move team of the tuple]
 * (alphazero.py:128-137: +1 / -1 by team, quirk Q12; :161-175: +-heuristic) */
int fpc_tuples_set_z(fpc_engine *e, const int *game_id, const float *z_team0, const float *z_team1, int n);
int fpc_tuples_count(fpc_engine *e);
int fpc_tuples_read(fpc_engine *e, fpc_tuple *host_out, int first, int n);
/* RCCL, driven from the C++ host (one communicator per engine = per GPU; no torch involved):
 * rank 0 makes the 128-byte id and hands it to the other ranks by whatever channel the caller has. */
int fpc_comm_available(void);     /* 0 when librccl is bound in this process, else FPC_ECOMM (fpc_last_error(NULL) says why):
                                   * lets every rank agree on the exchange path BEFORE any of them enters ncclCommInitRank */
int fpc_comm_unique_id(void *id128);
int fpc_comm_init(fpc_engine *e, const void *id128, int rank, int world);
int fpc_comm_destroy(fpc_engine *e);
/* episode end: one ncclAllGather of the per-rank counts and one of the max-padded tuple
 * arrays over xGMI.  counts_out: host [world].  The gathered tuples stay on the device, rank-major
 * (rank r's tuples first .. counts_out[r] of them), and are read with fpc_gathered_read. */
int fpc_allgather_tuples(fpc_engine *e, int *counts_out, int *total_out);
/* Between the two sits an 8-byte status all-gather that ALWAYS runs: a rank on which anything local failed (an upload, a
 * read-back, growing a buffer) still goes through the counts and the status collective, every rank then leaves before
 * the payload collective -- the failing one with its own error, the others with FPC_ECOMM naming it -- and the
 * communicator stays usable.  Only an error of an RCCL call itself, or a failed read-back of the status words, ends
 * with the communicator aborted (ncclCommAbort) and fpc_comm_init needed again.
 * TEST HOOK: the next fpc_allgather_tuples treats one of its own HIP calls as failed -- 1 counts upload, 2 counts
 * read-back, 3 send-buffer growth, 4 status upload, 5 status read-back; 0 clears it. */
int fpc_debug_comm_fault(fpc_engine *e, int point);
int fpc_gathered_read(fpc_engine *e, fpc_tuple *host_out, int first, int n);

/* ---- device-resident replay: the trainer's two ring buffers (alphazero.py:33-34, replay_buffer.py:4-20) as fpc_tuple
 * arrays in device memory, 1280 B per record, and one launch (k_replay_decode) that turns any selection of slots into the
 * dense batch the optimiser step reads.  Ring semantics are replay_buffer.ReplayBuffer's: append until `capacity`, then
 * overwrite at a cursor that advances modulo capacity; slot i is the i-th element of that buffer's list.  The cursors
 * live on the host.
 * FPC_EINVAL: ring outside 0..FPC_REPLAY_SCRATCH, capacity < 1, null or (fpc_replay_batch) not 16-byte aligned outputs,
 * n or m < 0, a slot outside 0..size-1, a src_index outside the source's count, a ring_of outside -1..FPC_REPLAY_RINGS-1;
 * FPC_ESTATE: push, load or batch on a ring never reserved, FPC_REPLAY_GATHERED before any fpc_allgather_tuples;
 * FPC_ENOMEM: allocation failure.  A call that fails on its arguments leaves every ring as it was. */
#define FPC_REPLAY_RINGS 2              /* 0 experience, 1 validation */
#define FPC_REPLAY_SCRATCH 2            /* a third ring for reserve / load / read / batch only (tuples.dense_batch_device): never a push target */
enum { FPC_REPLAY_COLLECTED = 0,        /* source: this engine's collected tuples, index space of fpc_tuples_read */
       FPC_REPLAY_GATHERED = 1 };       /* source: the last fpc_allgather_tuples, index space of fpc_gathered_read (padding is never copied) */
int fpc_replay_reserve(fpc_engine *e, int ring, int capacity);   /* (re)allocate and empty one ring; its current capacity again only
                                                                  * empties it; on FPC_ENOMEM the ring and its contents are as they were */
/* j = 0..m-1 in order: source tuple src_index[j] (NULL: j) is appended to ring ring_of[j] (NULL: ring 0; -1: dropped).
 * Device to device, one k_replay_store launch per call; of several entries landing on one slot only the last is copied. */
int fpc_replay_push(fpc_engine *e, int source, const int *src_index, const int8_t *ring_of, int m);
int fpc_replay_load(fpc_engine *e, int ring, const fpc_tuple *host, int n);   /* append n records from host memory (resume, tests) */
int fpc_replay_size(fpc_engine *e, int ring);
int fpc_replay_read(fpc_engine *e, int ring, fpc_tuple *host_out, int first_slot, int n);
/* The batch of the records in slot[0..n-1] (host array; any order, repeats allowed), written to DEVICE memory:
 * enc_dev [n,24,R,R] f32 = GetEncodedState of each record by its own side to move (alphazero.py:71-73) under the engine's
 * current rule set, pi_dev [n,A] f32 = visits / sum(visits) at the record's flat indices and 0 elsewhere (bit-identical to
 * the host path's torch arithmetic; a record with n == 0, or whose visits sum to 0, gives a zero row), z_dev [n] f32.  Launched on the engine's
 * stream, which is synchronised before the call returns: any other stream may read the outputs afterwards. */
int fpc_replay_batch(fpc_engine *e, int ring, const int *slot, int n, float *enc_dev, float *pi_dev, float *z_dev);
/* fpc_replay_batch plus w_dev [n] f32, the record's policy-loss weight: 0.0f where the record has FPC_TUPLE_FAST, else
 * 1.0f.  One launch, as fpc_replay_batch; enc_dev, pi_dev and z_dev are bit for bit what fpc_replay_batch writes for the
 * same slots (a fast record's pi row is still decoded).  A null w_dev is FPC_EINVAL. */
int fpc_replay_batch_w(fpc_engine *e, int ring, const int *slot, int n, float *enc_dev, float *pi_dev, float *z_dev, float *w_dev);

/* ---- measurement hooks (bench.py) -------------------------------------------------------- */
typedef struct fpc_stats {
  /* HIP-event time (events recorded on the engine's stream, resolved in fpc_search_results)
   * accumulated since fpc_stats_reset: select+encode | residual tower incl. head convs |
   * policy Linear (+ split-K reduce) | expand+backup.  Every 16th simulation step is timed and its
   * intervals count 16x (the events themselves cost time) */
  double ms_select, ms_tower, ms_fc, ms_expand;
  uint64_t launches_select, launches_nn, launches_expand;
  uint64_t sims;                        /* leaf evaluations + terminal backups */
  uint64_t nodes;                       /* nodes allocated */
} fpc_stats;
int fpc_stats_get(fpc_engine *e, fpc_stats *out);
int fpc_stats_reset(fpc_engine *e);
int fpc_set_timing(fpc_engine *e, int enabled);  /* HIP events around each stage (adds syncs) */
const char *fpc_nn_kernel(fpc_engine *e);        /* name of the kernel that runs the residual tower for the loaded weights:
                                                  * "k_towerw" (hidden 256; hidden 128 off the 14x14 board), "k_towerc" (hidden 128, 14x14: k_tower's
                                                  * skeleton on the compact image), "k_tower" (developer knobs), "k_conv3x3" (per layer), "" before fpc_load_weights */
/* HIP-event time of k_replay_decode alone in the last fpc_replay_batch that ran with fpc_set_timing on (else FPC_ESTATE) */
int fpc_replay_decode_ms(fpc_engine *e, float *ms_out);
/* the same for k_play_ply in the last fpc_search_play */
int fpc_search_play_ms(fpc_engine *e, float *ms_out);
void *fpc_stream(fpc_engine *e);                 /* hipStream_t the engine launches on */
int fpc_memory_is_host(void);                    /* 1 in the wavefront-emulator build of these sources, where every "device" pointer
                                                  * (enc_dev, logits_dev, the fpc_replay_batch outputs, ...) is host memory; 0 in the product */

#ifdef __cplusplus
}
#endif
#endif /* FPC_ENGINE_H_ */
