// fpc_tree_kernels.h -- CDNA4 kernels for the tree side of MCTS.search: one 64-lane wavefront per
// concurrent game (block = 1 wave, grid = games), board state staged in LDS.
//
//   k_board_ops      batched Board::GetLegalMoves / GetGameResult / TakeAction / encode / mask
//   k_attack_maps    GetAttackedSquaresPlayers / GetAttackedSquaresTeams / IsAttackedByPlayer (wrapper.cpp:201-206)
//   k_select         Node::ChooseLeaf: PUCT descent (wave argmax), lazy leaf-board materialisation,
//                    GetGameResult + GetLegalMoves on the leaf, terminal backup        (node.cpp:19-78)
//   k_encode         Board::GetEncodedStates incl. the batch-wide rot90                 (board.cpp:305-356)
//   k_softmax_partials  per-chunk softmax statistics of a logits row (external evaluators; the internal
//                    policy Linear's k_fc_reduce leaves the same records)                (mcts.py:67)
//   k_expand         ParseActionspace / mask / renormalise from those statistics, BackpropagateNodes,
//                    ExpandNodes                                                        (mcts.py:67-89)
//   k_expand_select  k_expand of simulation step s + k_select of step s+1 in one launch
//   k_select_multi / k_expand(_legal)(_select)_multi  the same for the opt-in leaf-parallel search (K leaves per game
//                    per step, virtual loss; fpc_search_set_leaves): the descent is select_game's, row k*G + g per leaf
//   k_tree_advance   opt-in subtree reuse (fpc_search_advance / _refill): re-roots every game's tree on the move played, out of place,
//                    and starts fresh games in the rows that are refilled
//   k_play_ply       opt-in device-side move choice (fpc_search_play): draws each game's move from the finished search's root
//                    visit counts, makes it on the root state and runs GetGameResult on the result
//   k_replay_store / k_replay_decode  opt-in device-resident replay (fpc_replay_*): training records into ring slots, and any
//                    selection of slots into the trainer's dense (state, pi, z) batch in one launch  (alphazero.py:71-73, :104-110)
//
// Reference semantics (file:line relative to /root/reference/src/cpp) are restated per function.
// Nothing here is translated from the reference: its board is a pointer-rich mailbox + std::vector
// piece lists walked serially; here one wave works on a 288-byte LDS image, (piece,direction)
// slots are walked by separate lanes, every pseudo-legal move is legality-tested by its own lane on
// a *virtual* post-move board (no make/undo), and the piece-list reorderings that the reference's
// make/undo loops cause (observable through GetGameResult) are applied in closed form.
#pragma once
#include "fpc_platform.h"
#include "../../include/fpc_engine.h"

#include <type_traits>

namespace fpc {

enum { PAWN = 0, KNIGHT = 1, BISHOP = 2, ROOK = 3, QUEEN = 4, KING = 5 };

struct DevCfg {
  int R, INV, RR, A_ch, A;
  int rules;         // FPC_RULES_* bits (include/fpc_engine.h); 0 = strict reference semantics
  int rcpR;          // 65536 / R + 1: q / R == (q * rcpR) >> 16 exactly for 0 <= q < 4681 (R <= 14)
};
__host__ __device__ __forceinline__ DevCfg make_devcfg(int R, int INV, int rules) {
  return DevCfg{R, INV, R * R, 8 * R + 8, (8 * R + 8) * R * R, rules, 65536 / R + 1};
}
// square index -> row (the integer division by the runtime board size costs ~40 VALU instructions)
__host__ __device__ __forceinline__ int row_of(const DevCfg &c, int q) { return (q * c.rcpR) >> 16; }

// error bits accumulated per game / per board (host maps them to fpc_status)
enum { ERR_SELECT = 1, ERR_POLICY = 2, ERR_CAP_MOVES = 4, ERR_CAP_NODES = 8, ERR_MOVE = 16, ERR_CAP_BOARDS = 32 };

// ---- per-game tree storage (SoA, one contiguous region per game) -------------------------------
struct Tree {
  int *N;            // visit_count                     node.h:70
  double *W;         // value_sum                       node.h:76
  float *P;          // prior (f32 -> double on use)    node.h:75, mcts.py:87
  uint16_t *mv;      // move_made as flat index         node.h:74
  int *parent;       // -1 for root                     node.h:73
  int *child0;       // first child (children contiguous, ascending flat), -1 = not expanded  node.h:78
  uint16_t *nch;
  int *bslot;        // board-pool slot of this node's state, -1 = not materialised yet
  fpc_board *boards; // board pool
  int node_cap, board_cap;
  // per game scalars
  int *nnodes, *nboards, *alive, *sims_done, *err;
  int *leaf_node;    // leaf chosen this step (-1: none)
  int *leaf_slot;    // board-pool slot of that leaf's state (-1: none) -- what k_encode reads
  int *leaf_turn;
  int *leaf_node_nx, *leaf_slot_nx, *leaf_turn_nx;   // the same three for the NEXT step (k_expand_select writes them while
                                                     // other games' expansions still read this step's; the host swaps)
  int *nlegal;
  uint16_t *legal;   // [G][FPC_MAX_MOVES] ascending unique flat indices of the leaf's legal moves
  int *path;         // [G][path_cap] root..leaf node ids of this step's descent (k_select -> k_expand's backup)
  int *path_len;
  int path_cap;
  // root Dirichlet noise (N4; off when null): gamma draws [G][FPC_MAX_MOVES], one per root child in ascending flat order
  const float *noise;
  float noise_eps;
  // per-game simulation budgets (fpc_search_set_budget; null: none): [G] caps on sims_done, read by select_game only
  const int *budget;
  // live-row numbering of the pending selection (fpc_search_set_live_rows, k_live_rows; null: off): [rows] the network row
  // of step row r, -1 for a dead row.  Read by the expansion and k_policy_gemv only.
  const int *inv;
  // first-play urgency (fpc_search_set_fpu; 0 = FPC_FPU_ZERO: off): the q of a child with N' == 0 in select_game's PUCT branch
  int fpu_mode;
  // visit count a node is born with (Q1): 1, or 0 under FPC_RULES_VISITS (the rule setters keep it in step with DevCfg::rules).
  // Every place that creates a node reads it HERE, as a kernel argument, which costs a scalar load beside the store: derived
  // from DevCfg::rules up front, the compiler kept it in a register across the whole expansion and spilled that one to
  // scratch -- a memory round trip in front of the children's stores (0.3 us per step).  The places:
  // k_search_init, expand_finish, and k_tree_advance's fresh row and its childless root after a failed advance.
  int born;
  double fpu_red;
  // proof status per node (fpc_search_set_solver; null until the switch is first turned on): [G][node_cap] FPC_PROOF_*, seen
  // from the node's own side to move.  Read and written by the SOLVE instances of the selecting kernels only; carried by
  // k_tree_advance, read by k_play_ply and k_root_proofs.  Nothing gives a node a birth status: the host zeroes the array
  // (fpc_search_begin, the destination set of an advance), and a status is only ever stored on a node that exists.
  uint8_t *S;
  // forced playouts and policy target pruning at the root (fpc_search_set_forced; 0: off): the factor k.  Read by the FORCE
  // instances of the selecting kernels at the root level only, and by root_targets.  Last in the struct: no other field moves.
  double forced;
  // playout cap randomization (fpc_search_set_fast_rows; null: none): [G] bytes, 1 where the game's search of this ply is a
  // FAST search -- no forcing in its selection (the FORCE instances only read it), no pruning of its target (k_root_targets,
  // k_collect_tuples, k_play_ply), FPC_TUPLE_FAST in its record.  Set and cleared where `budget` is.  The allocation is
  // padded to a multiple of 4 bytes and 4-byte aligned: select_game reads the word that holds a game's byte.  Last in the struct.
  const uint8_t *fast;
};
__host__ __forceinline__ int born_visits(int rules) { return (rules & FPC_RULES_VISITS) ? 0 : 1; }

// ---- LDS image of one wave --------------------------------------------------------------------
constexpr int GEN_SCR = 14;             // per generator slot: a ray has at most 13 targets; slot 7 of a king: 1 step + 2 castlings
struct __attribute__((aligned(16))) WaveLds {
  fpc_board b;                         // 288 B
  // pseudo-legal moves in the reference's generation order.  mw packs what the later phases read:
  //   bits 0-7 to, 8-15 captured piece byte, 17 promotion (the reference emits 4 variants), 20-23 the
  //   mover's piece-list position (generation order key), 24-31 castling: the rook's square (it hops to
  //   from + (to-from)/2), else FPC_NO_SQ
  uint32_t mw[FPC_MAX_MOVES];
  uint8_t mfrom[FPC_MAX_MOVES];
  uint16_t lflat[FPC_MAX_MOVES];       // flat index of legal moves, reference order
  uint16_t lsorted[FPC_MAX_MOVES];     // ascending
  uint8_t lidx[FPC_MAX_MOVES];         // pseudo-move index of k-th legal move
  float pri[FPC_MAX_MOVES];
  uint32_t scr[64][2][GEN_SCR];        // generation scratch: lane x generator slot x targets (same packing as mw)
  uint16_t poff[FPC_MAX_PL + 1];       // first pseudo-move of each piece-list entry
  uint8_t l1pos[FPC_MAX_PL];           // own list: position after the GetGameResult reordering
  uint8_t newlist[3][FPC_MAX_PL];      // reordered lists (own, enemy a, enemy b) before they are copied back
  alignas(4) uint8_t ent[200];         // square -> 16*list + entry for the three lists a move can touch, else 0xFF (cleared 4 bytes per lane)
  int lk[2][48];                       // last move touching each list entry (GetGameResult's loop, GetLegalMoves' loop)
  int M, nlegal, first_legal, result, errbits;
  float scal_f;                        // wave-uniform scalar broadcast slot
};
__device__ __forceinline__ int mv_to(uint32_t w) { return (int)(w & 255u); }
__device__ __forceinline__ uint8_t mv_cap(uint32_t w) { return (uint8_t)(w >> 8); }
__device__ __forceinline__ int mv_promo(uint32_t w) { return (int)((w >> 17) & 1u); }
__device__ __forceinline__ int mv_piece(uint32_t w) { return (int)((w >> 20) & 15u); }
__device__ __forceinline__ int mv_rook(uint32_t w) { return (int)(w >> 24); }

__device__ __forceinline__ bool present(uint8_t p) { return (p & 0x80) != 0; }
__device__ __forceinline__ int colour_of(uint8_t p) { return (p >> 5) & 3; }
__device__ __forceinline__ int type_of(uint8_t p) { return (p >> 2) & 7; }
__device__ __forceinline__ int team_of_colour(int c) { return c & 1; }   // RED/YELLOW 0, BLUE/GREEN 1 (engine/board.h:64-67)
__device__ __forceinline__ int team_of(uint8_t p) { return (p >> 5) & 1; }

// engine/board.h:647-654.  Branch-free on purpose (bitwise & |): these run per lane in divergent code, where
// every short-circuit turns into an exec-mask save/restore and a branch.
__device__ __forceinline__ bool legal_loc(const DevCfg &c, int row, int col) {
  const int mx = c.R - 1;
  const bool in = ((unsigned)row <= (unsigned)mx) & ((unsigned)col <= (unsigned)mx);
  const bool cc = (col < c.INV) | (col > mx - c.INV);
  const bool rr = (row < c.INV) | (row > mx - c.INV);
  return in & !(cc & rr);
}
__host__ __device__ __forceinline__ bool in_array(const DevCfg &c, int row, int col) {
  return ((unsigned)row < (unsigned)c.R) & ((unsigned)col < (unsigned)c.R);
}

// move.cpp:13-20, :84-104: (from,to) -> action plane
__host__ __device__ __forceinline__ int move_plane(const DevCfg &c, int from, int to) {
  const int fr = row_of(c, from), tr = row_of(c, to);
  const int dy = tr - fr, dx = (to - tr * c.R) - (from - fr * c.R);
  const int ay = dy < 0 ? -dy : dy, ax = dx < 0 ? -dx : dx;
  if (dx == 0 || dy == 0 || ax == ay) {
    const int sx = (dx > 0) - (dx < 0), sy = (dy > 0) - (dy < 0);
    // queen_move_offsets (dx,dy): {0,-1},{-1,-1},{-1,0},{-1,1},{0,1},{1,1},{1,0},{1,-1}
    const int key = (sx + 1) * 3 + (sy + 1);
    int dir;
    switch (key) {
      case 0: dir = 1; break; case 1: dir = 2; break; case 2: dir = 3; break;
      case 3: dir = 0; break; case 5: dir = 4; break;
      case 6: dir = 7; break; case 7: dir = 6; break; default: dir = 5; break;
    }
    const int dist = ax > ay ? ax : ay;
    return dir * (c.R - 1) + dist - 1;
  }
  // knight_move_offsets (dx,dy): {-2,-1},{-2,1},{-1,-2},{-1,2},{1,-2},{1,2},{2,-1},{2,1}
  const int k = (dx == -2 ? 0 : dx == -1 ? 2 : dx == 1 ? 4 : 6) + (dy > 0 ? 1 : 0);
  return 8 * (c.R - 1) + k;
}

// Move(flat): move.cpp:39-61.  returns `to` (FPC_NO_SQ when off the array / unaddressable plane)
__host__ __device__ __forceinline__ int flat_to(const DevCfg &c, int flat, int *from_out) {
  const int plane = flat / c.RR, from = flat % c.RR;
  *from_out = from;
  const int nq = c.R - 1;
  int dx, dy;
  if (plane < 8 * nq) {
    const int dir = plane / nq, dist = plane % nq + 1;
    const int qdx[8] = {0, -1, -1, -1, 0, 1, 1, 1};
    const int qdy[8] = {-1, -1, 0, 1, 1, 1, 0, -1};
    dx = qdx[dir] * dist; dy = qdy[dir] * dist;
  } else {
    const int k = plane - 8 * nq;
    if (k >= 8) return FPC_NO_SQ;
    const int ndx[8] = {-2, -2, -1, -1, 1, 1, 2, 2};
    const int ndy[8] = {-1, 1, -2, 2, -2, 2, -1, 1};
    dx = ndx[k]; dy = ndy[k];
  }
  const int row = from / c.R + dy, col = from % c.R + dx;
  if (!in_array(c, row, col)) return FPC_NO_SQ;
  return row * c.R + col;
}

// input plane of a piece seen from the side to move (board.cpp:322-336): strict = 6*rel + type - 1 with
// -1 wrapping to 23 (quirk Q7); FPC_RULES_PLANES = 6*rel + type
__device__ __forceinline__ int piece_plane(uint8_t p, int turn, int rules) {
  int plane = 6 * ((colour_of(p) - turn) & 3) + type_of(p);
  if (!(rules & FPC_RULES_PLANES)) { plane -= 1; if (plane < 0) plane += 24; }
  return plane;
}

// torch.rot90(x, k, (-2,-1)) index map: out[i][j] = in[src]   (board.cpp:252-255)
__device__ __forceinline__ int rot90_src(int R, int k, int i, int j) {
  k &= 3;
  return k == 0 ? i * R + j : k == 1 ? j * R + (R - 1 - i) : k == 2 ? (R - 1 - i) * R + (R - 1 - j) : (R - 1 - j) * R + i;
}

// ---- wave helpers -------------------------------------------------------------------------------
__device__ __forceinline__ int lane_id() { return (int)(threadIdx.x & 63); }

// diagnostic builds only (-DFPC_TREE_STAMPS=<block>; tools/tree_stamps.py): s_memtime at the phase boundaries of the
// tree kernels for ONE game, read back through fpc_debug_tree_stamps.  The product build compiles none of it.
#ifdef FPC_TREE_STAMPS
__device__ unsigned long long g_tree_stamps[32];
#define FPC_TS(I) do { if ((int)blockIdx.x == FPC_TREE_STAMPS && lane_id() == 0) g_tree_stamps[I] = __builtin_amdgcn_s_memtime(); } while (0)
#else
#define FPC_TS(I) do {} while (0)
#endif

__device__ __forceinline__ void lds_load_board(WaveLds *s, const fpc_board *g) {
  const uint32_t *src = reinterpret_cast<const uint32_t *>(g);
  uint32_t *dst = reinterpret_cast<uint32_t *>(&s->b);
  const int l = lane_id();
  dst[l] = src[l];
  if (l < 8) dst[64 + l] = src[64 + l];
  __syncthreads();
}
__device__ __forceinline__ void lds_store_board(const WaveLds *s, fpc_board *g) {
  __syncthreads();
  const uint32_t *src = reinterpret_cast<const uint32_t *>(&s->b);
  uint32_t *dst = reinterpret_cast<uint32_t *>(g);
  const int l = lane_id();
  dst[l] = src[l];
  if (l < 8) dst[64 + l] = src[64 + l];
}

__device__ __forceinline__ bool promotes(const DevCfg &c, int colour, int tr, int tc) {   // engine/board.cpp:58-76
  switch (colour) {
    case 0: return tr == c.R / 4;
    case 1: return tc == 3 * c.R / 4;
    case 2: return tr == 3 * c.R / 4;
    default: return tc == c.R / 4;
  }
}

// Piece-list primitive of RemovePiece / SetPiece (engine/board.cpp:977-1014), wave-cooperative: lanes
// 0..15 hold one entry each, the first entry equal to `sq` is erased (the tail closes up) and `add` (>= 0)
// is appended.  Returns the new length; *found tells whether `sq` was there.  All lanes must call.
__device__ __forceinline__ int wave_list_erase_append(uint8_t *list, int len, int sq, int add, bool *found) {
  const int lane = lane_id();
  const int v = (lane < len && lane < FPC_MAX_PL) ? list[lane] : -1;
  const int nxt = __shfl(v, lane + 1 < 64 ? lane + 1 : lane);
  const unsigned long long hit = __ballot(v == sq);
  __syncthreads();                                   // every entry is in a register before any is rewritten
  const int idx = hit ? (int)__ffsll((long long)hit) - 1 : -1;
  int n = len;
  if (idx >= 0) {
    if (lane >= idx && lane + 1 < len) list[lane] = (uint8_t)nxt;
    n = len - 1;
  }
  if (add >= 0 && n < FPC_MAX_PL) { if (lane == 0) list[n] = (uint8_t)add; ++n; }
  *found = idx >= 0;
  __syncthreads();
  return n;
}

// MakeMove for a tree/self-play move, which carries only (from,to): capture whatever stands on
// `to`, no promotion, no rook hop, no rights update (engine/board.cpp:1028-1096 with a
// Move(flat)/Move(plane,from) argument).  false: "piece missing".
// With FPC_RULES_FULL_MOVES (the non-strict rule set) the move is executed the way the
// reference's own generator describes it (engine/board.cpp:58-88, :256-302, :313-466): a pawn that
// reaches its promotion line becomes a queen, a two-square king move hops the rook, king moves clear the
// mover's castling rights and a rook leaving its home square clears that side's.
// Wave-cooperative and wave-uniform: every lane derives the same scalars from the LDS board, the piece
// lists are edited one entry per lane, lane 0 writes the scalars.  All lanes must call.
// INSTANCE: 0 the one-leaf kernels, 1 the leaf-parallel selection, 2 k_tree_advance, 3 k_play_ply, 4 / 5 the descents of
// 0 / 1 with first-play urgency on, 8 / 9 / 12 / 13 those four with the solver in effect, + 16 those eight with forced
// playouts in effect -- separate
// instances, so that the one-leaf kernels' callees -- and with them the compiler's inlining decisions and the kernels'
// ISA -- stay exactly what they were before leaf-parallel search and subtree reuse
template <int INSTANCE = 0>
__device__ inline bool make_move_wave(fpc_board *b, int from, int to, const DevCfg &c) {
  const int lane = lane_id();
  if (to == FPC_NO_SQ) return false;
  uint8_t piece = b->sq[from];
  const uint8_t cap = b->sq[to];
  bool found;
  __syncthreads();
  if (present(cap)) {  // RemovePiece(to)
    const int cc = colour_of(cap);
    const int n = wave_list_erase_append(b->pl[cc], b->plen[cc], to, -1, &found);
    if (lane == 0) {
      b->plen[cc] = (uint8_t)n;
      b->sq[to] = 0;
      if (type_of(cap) == KING) b->king[cc] = FPC_NO_SQ;
    }
    __syncthreads();
  }
  if (!present(piece)) return false;
  const int pc = colour_of(piece);
  int rook_from = FPC_NO_SQ, rook_to = FPC_NO_SQ;
  uint8_t rights = b->castle[pc];
  if (c.rules & FPC_RULES_FULL_MOVES) {
    const int R = c.R, fr = row_of(c, from), fc = from - fr * R, tr = row_of(c, to), tc = to - tr * R;
    const int ty = type_of(piece);
    if (ty == PAWN) {
      if (promotes(c, pc, tr, tc)) piece = (uint8_t)(0x80 | (pc << 5) | (QUEEN << 2));
    } else if (ty == KING) {
      const int dr = tr - fr, dc = tc - fc;
      if ((dr == 0 && (dc == 2 || dc == -2)) || (dc == 0 && (dr == 2 || dr == -2))) {   // castling: the rook hops next to the king
        const int ur = dr / 2, uc = dc / 2;
        // kingside: rook 3 squares from the king, queenside: 4 (engine/board.cpp:343-465)
        for (int d = 3; d <= 4; ++d) {
          const int rr = fr + ur * d, rc = fc + uc * d;
          if (in_array(c, rr, rc)) {
            const uint8_t rk = b->sq[rr * R + rc];
            if (present(rk) && type_of(rk) == ROOK && colour_of(rk) == pc) { rook_from = rr * R + rc; rook_to = (fr + ur) * R + fc + uc; break; }
            if (present(rk)) break;
          }
        }
      }
      rights = 0;
    } else if (ty == ROOK && rights) {
      int ks, qs;      // rook home squares, engine/board.cpp:256-289
      switch (pc) {
        case 0: ks = (R - 1) * R + (R - 4); qs = (R - 1) * R + c.INV; break;
        case 1: ks = (R - 4) * R; qs = c.INV * R; break;
        case 2: ks = c.INV; qs = R - 4; break;
        default: ks = c.INV * R + (R - 1); qs = (R - 4) * R + (R - 1); break;
      }
      if (from == ks) rights &= (uint8_t)~1u;
      if (from == qs) rights &= (uint8_t)~2u;
    }
  }
  const uint8_t rook_piece = rook_from != FPC_NO_SQ ? b->sq[rook_from] : (uint8_t)0;
  // RemovePiece(from) + SetPiece(to, piece)
  int n = wave_list_erase_append(b->pl[pc], b->plen[pc], from, to, &found);
  if (rook_from != FPC_NO_SQ) {   // RemovePiece(rook_from) + SetPiece(rook_to): the rook's entry follows the king's
    const int n2 = wave_list_erase_append(b->pl[pc], n, rook_from, rook_to, &found);
    if (!found) { if (lane == 0 && n > 0) b->pl[pc][n - 1] = (uint8_t)rook_to; } else n = n2;
  }
  if (lane == 0) {
    b->plen[pc] = (uint8_t)n;
    b->sq[from] = 0;
    b->sq[to] = piece;
    if (type_of(piece) == KING) b->king[pc] = (uint8_t)to;
    if (c.rules & FPC_RULES_FULL_MOVES) b->castle[pc] = rights;
    if (rook_from != FPC_NO_SQ) { b->sq[rook_to] = rook_piece; b->sq[rook_from] = 0; }
    b->turn = (uint8_t)((b->turn + 1) & 3);  // GetNextPlayer, engine/board.cpp:1299-1313
  }
  __syncthreads();
  return true;
}

// IsAttackedByTeam(team, ksq) on the position obtained from `b` by moving the piece on `from` to
// `to` -- and, for castling, the rook on `from2` to `to2` -- (virtual make; FPC_NO_SQ squares -> the
// position itself).  engine/board.cpp:606-787.
// The function has no side effects, so the reference's probe ORDER is not observable; what costs time
// on a single wave is the LDS round trip of every dependent probe (~100 cycles each).  All 20 leaper
// probes (8 knight, 4 pawn, 8 king squares) and the first ATT_PRE squares of the 8 rays are therefore
// loaded back to back (out-of-range probes read the king's own square and are ignored), evaluated from
// registers, and only a ray still open after ATT_PRE empty squares continues with dependent loads.
constexpr int ATT_PRE = 3;
__device__ __attribute__((noinline)) bool attacked_virtual(const fpc_board *b, const DevCfg &c, int from, int to, uint8_t mover,
                                        int from2, int to2, uint8_t mover2, int ksq, int team) {
  const int R = c.R;
  const int kr = row_of(c, ksq), kc = ksq - kr * R;
  // content of square q after the virtual move: a chain of plain selects (lowest priority first), no branches
  auto vsq = [&](int q, uint32_t raw) -> uint8_t {
    uint32_t v = raw;
    v = q == to2 ? (uint32_t)mover2 : v;
    v = q == to ? (uint32_t)mover : v;
    v = ((q == from) | (q == from2)) ? 0u : v;
    return (uint8_t)v;
  };
#define FPC_VSQ(q, raw) vsq((q), (raw))
  // a piece byte is 1 c c t t t 0 0 (present, colour, type): present + team + type in one masked compare
  const uint8_t tkey = (uint8_t)(0x80 | (team << 5));
  int lq[20];
  uint8_t lraw[20];
  // knights: all 8 offsets regardless of board size (:676-694)
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    const int dr = (k & 4) ? ((k & 2) ? 1 : -1) : ((k & 2) ? 2 : -2);
    const int dc = (k & 4) ? ((k & 1) ? 2 : -2) : ((k & 1) ? 1 : -1);
    const int r = kr + dr, cc = kc + dc;
    lq[k] = legal_loc(c, r, cc) ? r * R + cc : -1;
  }
  // pawns (:697-750): array bounds only
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int r = (k >> 1) ? kr + 1 : kr - 1, cc = (k & 1) ? kc + 1 : kc - 1;
    lq[8 + k] = in_array(c, r, cc) ? r * R + cc : -1;
  }
  // kings (:753-772)
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    const int kk = k < 4 ? k : k + 1;
    const int r = kr + kk / 3 - 1, cc = kc + kk % 3 - 1;
    lq[12 + k] = legal_loc(c, r, cc) ? r * R + cc : -1;
  }
  // rays: rooks & queens end at the ARRAY edge, not at the cut corners (:632);
  // bishops & queens are bounded by IsLegalLocation (:658)
  int rq[8][ATT_PRE];
  uint8_t rraw[8][ATT_PRE];
#pragma unroll
  for (int d = 0; d < 8; ++d) {
    const int ri = d < 4 ? (d == 0 ? -1 : d == 1 ? 1 : 0) : ((d & 2) ? 1 : -1);
    const int ci = d < 4 ? (d == 2 ? -1 : d == 3 ? 1 : 0) : ((d & 1) ? 1 : -1);
#pragma unroll
    for (int k = 0; k < ATT_PRE; ++k) {
      const int r = kr + ri * (k + 1), cc = kc + ci * (k + 1);
      const bool in = d < 4 ? in_array(c, r, cc) : legal_loc(c, r, cc);
      rq[d][k] = in ? r * R + cc : -1;
    }
  }
#pragma unroll
  for (int k = 0; k < 20; ++k) lraw[k] = b->sq[lq[k] < 0 ? ksq : lq[k]];
#pragma unroll
  for (int d = 0; d < 8; ++d)
#pragma unroll
    for (int k = 0; k < ATT_PRE; ++k) rraw[d][k] = b->sq[rq[d][k] < 0 ? ksq : rq[d][k]];
  bool hit = false;
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    const uint8_t p = FPC_VSQ(lq[k], lraw[k]);
    hit |= (lq[k] >= 0) & ((p & 0xBC) == (tkey | (KNIGHT << 2)));
  }
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const uint8_t p = FPC_VSQ(lq[8 + k], lraw[8 + k]);
    // the pawn of colour `col` attacks diagonally forward: red (0) upwards, so it sits one row below (pr = 1), ...
    const int pr = k >> 1, pc = k & 1, col = colour_of(p);
    const bool att = ((col == 0) & (pr != 0)) | ((col == 1) & (pc == 0)) | ((col == 2) & (pr == 0)) | ((col == 3) & (pc != 0));
    hit |= (lq[8 + k] >= 0) & ((p & 0xBC) == (tkey | (PAWN << 2))) & att;
  }
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    const uint8_t p = FPC_VSQ(lq[12 + k], lraw[12 + k]);
    hit |= (lq[12 + k] >= 0) & ((p & 0xBC) == (tkey | (KING << 2)));
  }
  unsigned open_rays = 0;     // bit d: ray d saw ATT_PRE empty in-range squares
#pragma unroll
  for (int d = 0; d < 8; ++d) {
    const uint8_t slider = (uint8_t)(tkey | ((d < 4 ? ROOK : BISHOP) << 2)), queen = (uint8_t)(tkey | (QUEEN << 2));
    bool open = true;
#pragma unroll
    for (int k = 0; k < ATT_PRE; ++k) {
      const uint8_t p = FPC_VSQ(rq[d][k], rraw[d][k]);
      const bool in = rq[d][k] >= 0, occ = present(p);
      hit |= open & in & (((p & 0xBC) == slider) | ((p & 0xBC) == queen));
      open = open & in & !occ;
    }
    open_rays |= open ? 1u << d : 0u;
  }
  if (open_rays && !hit) {   // more than ATT_PRE empty squares in some direction: walk on with dependent loads
    for (int d = 0; d < 8; ++d) {
      if (!((open_rays >> d) & 1u)) continue;
      const int slider = d < 4 ? ROOK : BISHOP;
      const int ri = d < 4 ? (d == 0 ? -1 : d == 1 ? 1 : 0) : ((d & 2) ? 1 : -1);
      const int ci = d < 4 ? (d == 2 ? -1 : d == 3 ? 1 : 0) : ((d & 1) ? 1 : -1);
      int r = kr + ri * (ATT_PRE + 1), cc = kc + ci * (ATT_PRE + 1);
      while (d < 4 ? in_array(c, r, cc) : legal_loc(c, r, cc)) {
        const int q = r * R + cc;
        const uint8_t p = FPC_VSQ(q, b->sq[q]);
        if (present(p)) {
          hit |= team_of(p) == team && (type_of(p) == slider || type_of(p) == QUEEN);
          break;
        }
        r += ri; cc += ci;
      }
    }
  }
#undef FPC_VSQ
  return hit;
}

// ---- king-safety tables: IsKingSafeAfterMove (board.cpp:59-68) for ALL pseudo-legal moves of a position at once ----
// attacked_virtual above answers "is square K attacked after this move" from scratch: 44 probes and ~1 000 VALU
// instructions per move, on every lane.  But for the moves of one position almost everything is shared: the king
// stands on the same square K for every move that is not a king move, and such a move changes the board on two squares
// only.  So the wave looks at K ONCE:
//   * the enemy leapers (knight / pawn / king, IsAttackedByTeam's probe squares, engine/board.cpp:676-772) that attack K
//     now: their number and, if it is one, its square -- a move of another piece removes such an attack only by
//     capturing that piece;
//   * per ray d from K (rook-type rays end at the ARRAY edge, bishop-type rays at the first illegal location, exactly
//     as in engine/board.cpp:632 / :658): the distance of the first and of the second piece on it and whether each is an
//     enemy slider of the ray's type -- a move changes what K sees along a ray only by interposing on / capturing along
//     that ray (the mover becomes the first piece: the mover's side never attacks its own king) or by taking the FIRST
//     piece off it (the second one becomes visible).
// A lane then decides its move with a few compares (ks_move_leaves_king_attacked).  King moves -- K itself changes --
// are decided by eight lanes each, one per ray / leaper offset (ks_king_moves).  Castling (never generated through the
// reference's Python boundary) and positions judged for a player of the other team than the mover keep the
// generic test.  Every decision equals attacked_virtual's: same squares, same bounds, same piece tests.
__device__ __forceinline__ void ray_dir(int d, int *ri, int *ci) {            // attacked_virtual's ray numbering
  *ri = d < 4 ? (d == 0 ? -1 : d == 1 ? 1 : 0) : ((d & 2) ? 1 : -1);
  *ci = d < 4 ? (d == 2 ? -1 : d == 3 ? 1 : 0) : ((d & 1) ? 1 : -1);
}
// ray (0..7, or -1) and distance of square (r, c) as seen from (kr, kc); branch-free
__device__ __forceinline__ int ray_of(int kr, int kc, int r, int c, int *dist) {
  const int dr = r - kr, dc = c - kc;
  const int ar = dr < 0 ? -dr : dr, ac = dc < 0 ? -dc : dc;
  int d = -1;
  d = ((dc == 0) & (dr != 0)) ? (dr < 0 ? 0 : 1) : d;
  d = ((dr == 0) & (dc != 0)) ? (dc < 0 ? 2 : 3) : d;
  d = ((ar == ac) & (ar != 0)) ? 4 + (dr > 0 ? 2 : 0) + (dc > 0 ? 1 : 0) : d;
  *dist = ar > ac ? ar : ac;
  return d;
}
__device__ __forceinline__ bool enemy_slider(uint8_t p, int d, int team) {
  const uint8_t tkey = (uint8_t)(0x80 | (team << 5));
  return ((p & 0xBC) == (uint8_t)(tkey | ((d < 4 ? ROOK : BISHOP) << 2))) | ((p & 0xBC) == (uint8_t)(tkey | (QUEEN << 2)));
}
// leaper probe k (0..7 knight, 8..11 pawn, 12..19 king) of square (kr, kc): the probed square or -1, as attacked_virtual
__device__ __forceinline__ int leaper_square(const DevCfg &c, int kr, int kc, int k) {
  int r, cc;
  bool in;
  if (k < 8) {
    const int dr = (k & 4) ? ((k & 2) ? 1 : -1) : ((k & 2) ? 2 : -2);
    const int dc = (k & 4) ? ((k & 1) ? 2 : -2) : ((k & 1) ? 1 : -1);
    r = kr + dr; cc = kc + dc; in = legal_loc(c, r, cc);
  } else if (k < 12) {
    const int j = k - 8;
    r = (j >> 1) ? kr + 1 : kr - 1; cc = (j & 1) ? kc + 1 : kc - 1; in = in_array(c, r, cc);
  } else {
    const int j = k - 12, kk = j < 4 ? j : j + 1;
    r = kr + kk / 3 - 1; cc = kc + kk % 3 - 1; in = legal_loc(c, r, cc);
  }
  return in ? r * c.R + cc : -1;
}
// does piece byte p on leaper probe k attack the probed-from square for `team`?  (engine/board.cpp:676-772)
__device__ __forceinline__ bool leaper_attacks(uint8_t p, int k, int team) {
  const uint8_t tkey = (uint8_t)(0x80 | (team << 5));
  if (k < 8) return (p & 0xBC) == (uint8_t)(tkey | (KNIGHT << 2));
  if (k >= 12) return (p & 0xBC) == (uint8_t)(tkey | (KING << 2));
  const int j = k - 8, pr = j >> 1, pc = j & 1, col = colour_of(p);
  const bool att = ((col == 0) & (pr != 0)) | ((col == 1) & (pc == 0)) | ((col == 2) & (pr == 0)) | ((col == 3) & (pc != 0));
  return ((p & 0xBC) == (uint8_t)(tkey | (PAWN << 2))) & att;
}
struct KingSafety {
  int kr, kc;          // the king's square K
  uint32_t ray;        // THIS lane's copy of ray (lane & 7): d1 | d2 << 4 | len << 8 | a1 << 12 | a2 << 13  (fetch another ray's with __shfl)
  int abase;           // bit d: the first piece on ray d is an enemy slider of that ray's type (wave-uniform)
  int nla, sqla;       // enemy leapers attacking K now; the square of the only one when nla == 1 (wave-uniform)
};
// All 64 lanes call.  K must be a square of the board.
__device__ __forceinline__ KingSafety ks_build(const fpc_board *b, const DevCfg &c, int K, int team) {
  const int lane = lane_id(), R = c.R;
  KingSafety ks;
  ks.kr = row_of(c, K); ks.kc = K - ks.kr * R;
  // rays: lane (d, k) looks at distances k + 1 and k + 9 of ray d
  {
    const int d = lane >> 3, k = lane & 7;
    int ri, ci;
    ray_dir(d, &ri, &ci);
    const int r1 = ks.kr + ri * (k + 1), c1 = ks.kc + ci * (k + 1), r2 = ks.kr + ri * (k + 9), c2 = ks.kc + ci * (k + 9);
    const bool in1 = d < 4 ? in_array(c, r1, c1) : legal_loc(c, r1, c1);
    const bool in2 = (k < 5) & (d < 4 ? in_array(c, r2, c2) : legal_loc(c, r2, c2));
    const uint8_t p1 = b->sq[in1 ? r1 * R + c1 : K], p2 = b->sq[in2 ? r2 * R + c2 : K];
    const unsigned long long Bin1 = __ballot(in1), Bin2 = __ballot(in2);
    const unsigned long long Boc1 = __ballot(in1 & present(p1)), Boc2 = __ballot(in2 & present(p2));
    // every lane assembles ray dd = lane & 7 (the eight copies are identical; lane dd < 8 is the one others fetch)
    const int dd = lane & 7;
    const uint32_t in13 = (uint32_t)((Bin1 >> (8 * dd)) & 0xFFull) | ((uint32_t)((Bin2 >> (8 * dd)) & 0x1Full) << 8);
    const uint32_t oc13 = (uint32_t)((Boc1 >> (8 * dd)) & 0xFFull) | ((uint32_t)((Boc2 >> (8 * dd)) & 0x1Full) << 8);
    const int len = __builtin_ctz(~in13);                       // squares up to the first one that is out of range (<= 13)
    const uint32_t oc = oc13 & ((1u << len) - 1u);
    const int d1 = oc ? __builtin_ctz(oc) + 1 : 0;
    const uint32_t oc2 = oc & (oc - 1u);
    const int d2 = oc2 ? __builtin_ctz(oc2) + 1 : 0;
    int rdi, cdi;
    ray_dir(dd, &rdi, &cdi);
    const uint8_t q1 = b->sq[d1 ? (ks.kr + rdi * d1) * R + ks.kc + cdi * d1 : K];
    const uint8_t q2 = b->sq[d2 ? (ks.kr + rdi * d2) * R + ks.kc + cdi * d2 : K];
    const bool a1 = (d1 != 0) & enemy_slider(q1, dd, team), a2 = (d2 != 0) & enemy_slider(q2, dd, team);
    ks.ray = (uint32_t)d1 | ((uint32_t)d2 << 4) | ((uint32_t)len << 8) | (a1 ? 1u << 12 : 0u) | (a2 ? 1u << 13 : 0u);
    ks.abase = (int)(__ballot(a1) & 0xFFull);                   // lanes 0..7 hold rays 0..7
  }
  // leapers: lane k < 20 owns probe k
  {
    const int q = lane < 20 ? leaper_square(c, ks.kr, ks.kc, lane) : -1;
    const uint8_t p = b->sq[q < 0 ? K : q];
    const bool att = (q >= 0) && leaper_attacks(p, lane, team);
    const unsigned long long B = __ballot(att);
    ks.nla = __popcll(B);
    ks.sqla = wave_read(q, B ? (int)__ffsll((long long)B) - 1 : 0);
  }
  return ks;
}
// Is K attacked after the move f -> t of a piece of K's own side that is not K itself (no rook hop)?  All lanes call
// (the ray records travel by __shfl); lanes without a move pass any squares and ignore the answer.
__device__ __forceinline__ bool ks_move_leaves_king_attacked(const KingSafety &ks, const DevCfg &c, int f, int t) {
  const int R = c.R;
  const int fr = row_of(c, f), fc = f - fr * R, tr = row_of(c, t), tc = t - tr * R;
  int dt, df;
  const int rt = ray_of(ks.kr, ks.kc, tr, tc, &dt), rf = ray_of(ks.kr, ks.kc, fr, fc, &df);
  const uint32_t pt = __shfl(ks.ray, rt < 0 ? 0 : rt), pf = __shfl(ks.ray, rf < 0 ? 0 : rf);
  int att = ks.abase;
  {   // the mover lands on ray rt in front of (or on) its first piece: it is the first piece now
    const int d1 = (int)(pt & 15u), len = (int)((pt >> 8) & 15u);
    const bool blocks = (rt >= 0) & (dt <= len) & ((d1 == 0) | (dt <= d1));
    att = blocks ? att & ~(1 << (rt < 0 ? 0 : rt)) : att;
  }
  {   // the mover WAS the first piece of ray rf and leaves the ray: the second piece shows
    const int d1 = (int)(pf & 15u);
    const bool opens = (rf >= 0) & (d1 != 0) & (df == d1) & (rt != rf);
    att = (opens & (((pf >> 13) & 1u) != 0u)) ? att | (1 << (rf < 0 ? 0 : rf)) : att;
  }
  const bool leaper = (ks.nla >= 2) | ((ks.nla == 1) & (t != ks.sqla));
  return (att != 0) | leaper;
}
// Up to eight king moves f -> T_j at once: lane (j, d) walks ray d from T_j (with f emptied) and probes leaper offsets
// d of the knight / king patterns and d < 4 of the pawn pattern.  tsq: T_j of slot j = lane >> 3, or -1 (empty slot).
// Returns the ballot of "attacks T_j" over all lanes: slot j's answer is bits 8 j .. 8 j + 7 != 0.  All lanes call.
__device__ __forceinline__ unsigned long long ks_king_moves(const fpc_board *b, const DevCfg &c, int f, int tsq, int team) {
  const int lane = lane_id(), R = c.R, d = lane & 7;
  bool hit = false;
  if (tsq >= 0) {
    const int tr = row_of(c, tsq), tc = tsq - tr * R;
    // leapers: three independent probes
    const int qn = leaper_square(c, tr, tc, d), qk = leaper_square(c, tr, tc, 12 + d), qp = d < 4 ? leaper_square(c, tr, tc, 8 + d) : -1;
    const uint8_t pn = b->sq[qn < 0 ? tsq : qn], pk = b->sq[qk < 0 ? tsq : qk], pp = b->sq[qp < 0 ? tsq : qp];
    hit |= (qn >= 0) & (qn != f) && leaper_attacks(pn, d, team);
    hit |= (qk >= 0) & (qk != f) && leaper_attacks(pk, 12 + d, team);
    hit |= (qp >= 0) & (qp != f) && leaper_attacks(pp, 8 + (d & 3), team);
    // the ray: first piece on the board with f emptied (the king now stands on tsq itself)
    int ri, ci;
    ray_dir(d, &ri, &ci);
    int r = tr + ri, cc = tc + ci;
    while (d < 4 ? in_array(c, r, cc) : legal_loc(c, r, cc)) {
      const int q = r * R + cc;
      const uint8_t p = q == f ? (uint8_t)0 : b->sq[q];
      if (present(p)) { hit |= enemy_slider(p, d, team); break; }
      r += ri; cc += ci;
    }
  }
  return __ballot(hit);
}

// Generator slot `d` (0..7) of a piece, as data: a start square, a step and what a target square may
// hold.  The reference's generators -- pawn {fwd1, fwd2, capture-, capture+} (engine/board.cpp:97-177),
// knight (:179-207, loop bound invalid_area = quirk Q8), bishop (:240-254), rook (:256-302), queen =
// bishop then rook (:304-311), king 8 steps (:313-341) -- all reduce to "step (ir,ic) up to n times".
enum { GEN_QUIET = 1, GEN_CAPT = 2, GEN_PUSH2 = 4, GEN_PAWN = 8 };
struct GenSlot {
  int ir, ic;   // step
  int n;        // steps left (0: the slot is finished / does not exist)
  int mode;     // GEN_QUIET: empty targets are moves; GEN_CAPT: an enemy-occupied target is a move;
                // GEN_PUSH2: pawn double step (the 1st square must be a legal, empty location and is not a
                // move; the 2nd is only checked against the array bounds, Q15); GEN_PAWN: promotion line
};
__device__ __forceinline__ GenSlot gen_slot(const DevCfg &c, int type, int colour, int fr, int fc, int d) {
  GenSlot g{0, 0, 0, 0};
  const int R = c.R;
  if (type == PAWN) {
    if (d >= 4) return g;
    int dr = 0, dc = 0;
    bool not_moved;
    switch (colour) {
      case 0: dr = -1; not_moved = fr == R - 2; break;
      case 1: dc = 1; not_moved = fc == 1; break;
      case 2: dr = 1; not_moved = fr == 1; break;
      default: dc = -1; not_moved = fc == R - 2; break;
    }
    g.ir = dr; g.ic = dc;
    if (d == 0) { g.n = 1; g.mode = GEN_QUIET | GEN_PAWN; }
    else if (d == 1) { if (not_moved) { g.n = 2; g.mode = GEN_QUIET | GEN_PUSH2 | GEN_PAWN; } }
    else {
      const int sd = d == 2 ? -1 : 1;
      if ((colour & 1) == 0) g.ic += sd; else g.ir += sd;
      g.n = 1; g.mode = GEN_CAPT | GEN_PAWN;
    }
  } else if (type == KNIGHT) {
    const int per = 2 * (c.INV - 1);           // 0, 2 or 4 (invalid_area 1..3)
    if (d >= 2 * per) return g;
    const int sh = per == 4 ? 2 : 1;
    const int prs = d >> sh, rem = d & (per - 1), adr = 1 + (rem >> 1), pcs = rem & 1;
    const int adc = adr == 1 ? 2 : 1;
    g.ir = prs ? adr : -adr; g.ic = pcs ? adc : -adc;
    g.n = 1; g.mode = GEN_QUIET | GEN_CAPT;
  } else if (type == KING) {
    const int k = d < 4 ? d : d + 1;
    g.ir = k / 3 - 1; g.ic = k % 3 - 1;
    g.n = 1; g.mode = GEN_QUIET | GEN_CAPT;
  } else if (type == BISHOP || type == ROOK || type == QUEEN) {   // AddMovesFromIncrMovement2, engine/board.cpp:209-238
    const bool diag = type == BISHOP || (type == QUEEN && d < 4);
    const int rd = type == QUEEN ? d - 4 : d;
    if (diag) {
      if (d >= 4) return g;
      g.ir = (d & 2) ? 1 : -1; g.ic = (d & 1) ? 1 : -1;
    } else {
      // rook generator order (:291-301): (0,-1), (-1,0), (0,+1), (+1,0)
      if (rd < 0 || rd >= 4) return g;
      const int incr = (rd & 2) ? 1 : -1;
      if (rd & 1) { g.ir = incr; g.ic = 0; } else { g.ir = 0; g.ic = incr; }
    }
    g.n = R; g.mode = GEN_QUIET | GEN_CAPT;
  }
  return g;
}
// Castling (engine/board.cpp:343-465), generated after the king's eight steps, queenside first:
// rights bit set, a same-team rook on the expected square, empty squares between, and neither the
// king's square nor the first square it crosses attacked.  emit(to, rook_from).  The move travels as
// a plain two-square king move through the tree (Move(flat) drops the rook hop); only
// GetLegalMoves/GetGameResult execute the hop (virtually, for the legality test) and reorder lists.
template <class F>
__device__ inline void walk_castle(const fpc_board *b, const DevCfg &c, int from, F &&emit) {
  const uint8_t king = b->sq[from];
  const int colour = colour_of(king), team = team_of(king);
  const uint8_t cur = b->castle[colour];
  if (!(cur & 3)) return;
  const int R = c.R, fr = from / R, fc = from % R;
  for (int is_k = 0; is_k < 2; ++is_k) {
    if (!(is_k ? (cur & 1) : (cur & 2))) continue;
    int ur = 0, uc = 0;
    switch (colour) {
      case 0: uc = is_k ? 1 : -1; break;
      case 1: ur = is_k ? 1 : -1; break;
      case 2: uc = is_k ? -1 : 1; break;
      default: ur = is_k ? -1 : 1; break;
    }
    const int nb = is_k ? 2 : 3;
    const int rr = fr + ur * (nb + 1), rc = fc + uc * (nb + 1);
    if (!in_array(c, rr, rc)) continue;                 // reference reads out of bounds here
    const uint8_t rook = b->sq[rr * R + rc];
    if (!present(rook) || type_of(rook) != ROOK || team_of(rook) != team) continue;
    bool blocked = false;
    for (int k = 1; k <= nb; ++k) blocked |= present(b->sq[(fr + ur * k) * R + fc + uc * k]);
    if (blocked) continue;
    const int b0 = (fr + ur) * R + fc + uc;
    if (attacked_virtual(b, c, FPC_NO_SQ, FPC_NO_SQ, 0, FPC_NO_SQ, FPC_NO_SQ, 0, b0, team ^ 1)) continue;
    if (attacked_virtual(b, c, FPC_NO_SQ, FPC_NO_SQ, 0, FPC_NO_SQ, FPC_NO_SQ, 0, from, team ^ 1)) continue;
    emit((fr + 2 * ur) * R + fc + 2 * uc, rr * R + rc);
  }
}

// Wave-cooperative movegen + legality + (optionally) GetGameResult / GetLegalMoves side effects.
//   do_result: run Board::GetGameResult(player) (engine/board.cpp:891-939) -> s->result, and apply
//              the piece-list reordering of its make/undo loop (stops at the first legal move).
//   do_legal : run fpchess::Board::GetLegalMoves (board.cpp:94-118) -> s->lflat/lidx/lsorted,
//              s->nlegal, and apply the reordering of its full make/undo loop.  Skipped when
//              do_result found a terminal position (ChooseLeaf returns before the mask is built).
// `player` < 0 -> side to move.  All lanes of the wave must call this (uniform control flow).
// INSTANCE: see make_move_wave (0 the one-leaf kernels and k_board_ops, 1 the leaf-parallel selection, 3 k_play_ply, 4 / 5 first-play urgency)
template <int INSTANCE = 0>
__device__ inline void wave_position_ops(WaveLds *s, const DevCfg &c, bool do_result, bool do_legal, int player) {
  const int lane = lane_id();
  fpc_board *b = &s->b;
  const int turn = b->turn;
  if (player < 0) player = turn;
  const int nown = b->plen[turn];
  const bool gen = b->king[turn] != FPC_NO_SQ;   // GetPseudoLegalMoves2 returns 0 without own king (:852-856)
  const bool player_has_king = b->king[player] != FPC_NO_SQ;

  // ---- generation, one walk: lane = (piece p, generator slots d0, d0+1).  Both slots advance in the same
  //      loop (two independent LDS round trips per iteration) and park their targets in the lane's scratch
  //      rows; the wave scan of the counts then gives every lane its place in the reference's generation order.
  const int p = lane >> 2, d0 = (lane & 3) * 2;
  int cnt0 = 0, cnt1 = 0;
  int from = FPC_NO_SQ;
  uint32_t *scr0 = s->scr[lane][0], *scr1 = s->scr[lane][1];
  if (gen && p < nown) {
    from = b->pl[turn][p];
    const uint8_t piece = b->sq[from];
    const int type = type_of(piece), colour = colour_of(piece), team = team_of(piece);
    const int R = c.R, fr = row_of(c, from), fc = from - fr * R;
    GenSlot g0 = gen_slot(c, type, colour, fr, fc, d0), g1 = gen_slot(c, type, colour, fr, fc, d0 + 1);
    int r0 = fr, c0 = fc, r1 = fr, c1 = fc;
    auto step = [&](GenSlot &g, int &tr, int &tc, uint32_t *scr, int &cnt) {
      if (g.n <= 0) return;
      tr += g.ir; tc += g.ic;
      const bool second = (g.mode & GEN_PUSH2) && g.n == 1;
      if (!(second ? in_array(c, tr, tc) : legal_loc(c, tr, tc))) { g.n = 0; return; }
      const int to = tr * R + tc;
      const uint8_t cap = b->sq[to];
      bool emit;
      if (!present(cap)) {
        emit = (g.mode & GEN_QUIET) && !((g.mode & GEN_PUSH2) && g.n == 2);
        g.n = (g.mode & GEN_QUIET) ? g.n - 1 : 0;
      } else {
        emit = (g.mode & GEN_CAPT) && team_of(cap) != team;
        g.n = 0;
      }
      if (emit && cnt < GEN_SCR) {
        const bool promo = (g.mode & GEN_PAWN) && promotes(c, colour, tr, tc);
        scr[cnt++] = (uint32_t)to | ((uint32_t)cap << 8) | (promo ? 1u << 17 : 0u) | ((uint32_t)FPC_NO_SQ << 24);
      }
    };
    while (g0.n > 0 || g1.n > 0) {
      step(g0, r0, c0, scr0, cnt0);
      step(g1, r1, c1, scr1, cnt1);
    }
    if (d0 == 6 && type == KING)
      walk_castle(b, c, from, [&](int to, int rook_from) {
        if (cnt1 < GEN_SCR) scr1[cnt1++] = (uint32_t)to | ((uint32_t)rook_from << 24);
      });
  }
  FPC_TS(7);
  // exclusive wave scan of (cnt0+cnt1) in lane order == reference generation order
  int incl = cnt0 + cnt1;
  for (int off = 1; off < 64; off <<= 1) {
    const int v = __shfl_up(incl, off);
    if (lane >= off) incl += v;
  }
  const int total = wave_read(incl, 63);
  const int base = incl - (cnt0 + cnt1);
  if ((lane & 3) == 0 && p <= FPC_MAX_PL - 1) s->poff[p] = (uint16_t)(base < FPC_MAX_MOVES ? base : FPC_MAX_MOVES);
  if (lane == 0) {
    s->poff[FPC_MAX_PL] = (uint16_t)(total < FPC_MAX_MOVES ? total : FPC_MAX_MOVES);
    s->errbits = total > FPC_MAX_MOVES ? ERR_CAP_MOVES : 0;
    if (nown > FPC_MAX_PL) s->errbits |= ERR_CAP_MOVES;
  }
  const int M = total < FPC_MAX_MOVES ? total : FPC_MAX_MOVES;
  {  // scratch rows -> the dense move list
    const uint32_t tag = (uint32_t)p << 20;
    const int kmax = cnt0 > cnt1 ? cnt0 : cnt1;
    for (int k = 0; k < kmax; ++k) {
      if (k < cnt0 && base + k < FPC_MAX_MOVES) { s->mw[base + k] = scr0[k] | tag; s->mfrom[base + k] = (uint8_t)from; }
      if (k < cnt1 && base + cnt0 + k < FPC_MAX_MOVES) { s->mw[base + cnt0 + k] = scr1[k] | tag; s->mfrom[base + cnt0 + k] = (uint8_t)from; }
    }
  }
  // square -> list entry map and the "last move touching this entry" slots of the reordering below
  if (lane < 50) reinterpret_cast<uint32_t *>(s->ent)[lane] = 0xFFFFFFFFu;
  if (lane < 48) { s->lk[0][lane] = -1; s->lk[1][lane] = -1; }
  __syncthreads();

  // ---- legality (IsKingSafeAfterMove, board.cpp:59-68): lane i decides move i.  The player's king square is looked
  //      at once for the whole position (ks_build); a move of another piece is then a few compares, king moves take
  //      eight lanes each (ks_king_moves); castling and "judged for the other team" keep attacked_virtual.
  FPC_TS(8);
  const int enemy = team_of_colour(player) ^ 1;
  const int K0 = b->king[player];
  const bool tables = (K0 != FPC_NO_SQ) & (team_of_colour(turn) == team_of_colour(player));   // wave-uniform
  KingSafety ks{};
  if (tables) ks = ks_build(b, c, K0, enemy);
  FPC_TS(9);
  int nlegal = 0, first = -1;
  for (int base_i = 0; base_i < M; base_i += 64) {
    const int i = base_i + lane;
    bool legal = false;
    int f = 0, t = 0;
    bool king_move = false, generic = false;
    uint32_t w = 0;
    uint8_t mover = 0;
    if (i < M) {
      w = s->mw[i];
      f = s->mfrom[i]; t = mv_to(w);
      mover = b->sq[f];
      king_move = (type_of(mover) == KING) & (colour_of(mover) == player);
      generic = !tables | (mv_rook(w) != FPC_NO_SQ);
      if (K0 == FPC_NO_SQ) { legal = true; generic = false; king_move = false; }   // no king to protect (the reference's ksq test never runs)
    }
    if (tables) {
      // moves of the other pieces: the tables
      const bool att = ks_move_leaves_king_attacked(ks, c, f, t);
      if (i < M && !king_move && !generic) legal = !att;
      // king moves (without the rook hop): slot j = rank among this chunk's king moves, eight lanes per slot
      const unsigned long long kb = __ballot(i < M && king_move && !generic);
      if (kb) {                                                  // wave-uniform
        const int myslot = __popcll(kb & ((1ull << lane) - 1ull));
        if ((kb >> lane) & 1ull) { if (myslot < 8) s->lk[0][myslot] = t | (f << 8); }   // lk is cleared again below
        __syncthreads();
        const int j = lane >> 3, nk = __popcll(kb);
        const int ent = j < nk && j < 8 ? s->lk[0][j] : -1;
        const unsigned long long hb = ks_king_moves(b, c, ent < 0 ? 0 : (ent >> 8), ent < 0 ? -1 : (ent & 255), enemy);
        __syncthreads();
        if ((kb >> lane) & 1ull) {
          if (myslot < 8) legal = ((hb >> (8 * myslot)) & 0xFFull) == 0ull;
          else generic = true;                                   // more than eight king moves in one chunk: cannot happen (8 steps), kept total
        }
        if (lane < 8) s->lk[0][lane] = -1;
        __syncthreads();
      }
    }
    if (__ballot(generic)) {                                     // wave-uniform guard around the out-of-line generic test
      if (generic) {
        int ksq = K0;
        if (king_move) ksq = t;
        else if (ksq == t) ksq = FPC_NO_SQ;                      // the player's king itself was captured
        const int rf = mv_rook(w);                               // castling: the rook hops next to the king
        const int rt = rf == FPC_NO_SQ ? FPC_NO_SQ : f + (t - f) / 2;
        legal = ksq == FPC_NO_SQ ? true : !attacked_virtual(b, c, f, t, mover, rf, rt, rf == FPC_NO_SQ ? (uint8_t)0 : b->sq[rf], ksq, enemy);
      }
    }
    const unsigned long long bal = __ballot(legal);
    if (legal) {
      const int k = nlegal + __popcll(bal & ((1ull << lane) - 1ull));
      s->lidx[k] = (uint8_t)i;
      s->lflat[k] = (uint16_t)(move_plane(c, f, t) * c.RR + f);
    }
    if (first < 0 && bal) first = base_i + (int)__ffsll((long long)bal) - 1;
    nlegal += __popcll(bal);
  }
  __syncthreads();

  FPC_TS(10);
  // ---- GetGameResult (engine/board.cpp:891-939)
  int result = FPC_IN_PROGRESS;
  if (do_result) {
    if (!player_has_king) {
      result = team_of_colour(player) == 0 ? FPC_WIN_BG : FPC_WIN_RY;
    } else if (nlegal > 0) {
      const uint8_t cap = mv_cap(s->mw[first]);          // only the FIRST legal move is inspected (Q13)
      if (present(cap) && type_of(cap) == KING) result = team_of(cap) == 0 ? FPC_WIN_BG : FPC_WIN_RY;
    } else {
      const bool chk = attacked_virtual(b, c, FPC_NO_SQ, FPC_NO_SQ, 0, FPC_NO_SQ, FPC_NO_SQ, 0, b->king[player], enemy);
      result = !chk ? FPC_STALEMATE : (team_of_colour(player) == 0 ? FPC_WIN_BG : FPC_WIN_RY);
    }
  }
  const bool run_legal = do_legal && result == FPC_IN_PROGRESS;

  // ---- piece-list reorderings caused by the reference's make/undo loops, in closed form.
  // Every make/undo pair moves the mover's entry -- then, for castling, the rook's entry -- and the
  // captured piece's entry to the END of their lists (engine/board.cpp:977-1014,1028-1160).
  // GetGameResult does that for moves 0..upto (it returns at the first legal move), GetLegalMoves
  // afterwards for ALL pseudo-legal moves, regenerated in the then-current list order.  Net effect on
  // every list: entries no move touches keep their order in front; touched entries follow, ordered by
  // the LAST move that touches them (key = position of that move in the loop's generation order).
  // Lanes 0-15 own the side-to-move entries, lanes 16-31 / 32-47 the entries of the two enemy colours.
  {
    const bool phase1 = do_result && player_has_king;
    const int upto = nlegal > 0 ? first : M - 1;
    const unsigned long long lower = (1ull << lane) - 1ull;
    const int grp = lane >> 4, e = lane & 15;                  // grp 0: own list; 1, 2: enemy colours turn+1, turn+3
    const int lcol = grp == 0 ? turn : (grp == 1 ? ((turn + 1) & 3) : ((turn + 3) & 3));
    const bool my_lane = grp <= 2 && e < b->plen[lcol] && e < FPC_MAX_PL;
    const int mysq = my_lane ? b->pl[lcol][e] : -1;
    const unsigned long long gmask = 0xFFFFull << (grp * 16);
    auto rank_in_group = [&](int key, bool touched) {          // touched entries of my list with a smaller key
      int rank = 0;
      for (int k = 0; k < 16; ++k) {
        const int ok = __shfl(key, (lane & 48) + k);
        rank += (touched && ok >= 0 && ok < key) ? 1 : 0;
      }
      return rank;
    };
    // Which entry a move touches is looked up through the square -> entry map, and every move posts its
    // key to the entries it touches with an LDS atomic max (keys grow along the loop, so the maximum is
    // the LAST move touching the entry): one step per move instead of every entry scanning all moves.
    if (my_lane) s->ent[mysq] = (uint8_t)lane;
    __syncthreads();
    auto post = [&](int *lk, int i, uint32_t w, int key) {
      atomicMax(&lk[mv_piece(w)], key);                          // the mover
      const int rook = mv_rook(w);
      if (rook != FPC_NO_SQ) {                                   // the rook is re-appended AFTER the king
        const int en = s->ent[rook];
        if (en < 16) atomicMax(&lk[en], key + 1);
      }
      if (present(mv_cap(w))) {                                  // the captured piece (always an enemy entry)
        const int en = s->ent[mv_to(w)];
        if (en >= 16 && en < 48) atomicMax(&lk[en], key);
      }
    };
    // GetGameResult's loop: key = move index
    if (phase1)
      for (int i = lane; i <= upto; i += 64) post(s->lk[0], i, s->mw[i], 2 * i);
    __syncthreads();
    const int lk1 = (phase1 && my_lane) ? s->lk[0][lane] : -1;
    const bool t1 = my_lane && lk1 >= 0;
    const unsigned long long T1 = __ballot(t1), L = __ballot(my_lane);
    const int r1 = rank_in_group(lk1, t1);
    const unsigned long long U1 = L & ~T1 & gmask;
    const int pos1 = t1 ? __popcll(U1) + r1 : __popcll(U1 & lower);
    if (grp == 0 && my_lane) s->l1pos[e] = (uint8_t)(phase1 ? pos1 : e);
    __syncthreads();
    // GetLegalMoves' loop: key = (post-GetGameResult position of the mover, its per-piece move index)
    if (run_legal)
      for (int i = lane; i < M; i += 64) {
        const uint32_t w = s->mw[i];
        const int pc = mv_piece(w);
        post(s->lk[1], i, w, 2 * ((int)s->l1pos[pc] * 256 + (i - (int)s->poff[pc])));
      }
    __syncthreads();
    const int lk2 = (run_legal && my_lane) ? s->lk[1][lane] : -1;
    const bool t2 = my_lane && lk2 >= 0;
    const unsigned long long T2 = __ballot(t2);
    const int r2 = rank_in_group(lk2, t2);
    const unsigned long long U2 = L & ~T2 & gmask;
    const int pos2 = t2 ? __popcll(U2) + r2 : __popcll(U2 & lower);
    const int newpos = run_legal ? pos2 : pos1;
    if ((run_legal || phase1) && my_lane) s->newlist[grp][newpos] = (uint8_t)mysq;
    __syncthreads();
    if ((run_legal || phase1) && my_lane) b->pl[lcol][e] = s->newlist[grp][e];
    if (lane == 0) { s->M = M; s->nlegal = run_legal ? nlegal : 0; s->first_legal = first; s->result = result; }
  }
  __syncthreads();

  FPC_TS(11);
  // ---- ascending flat order of the legal set (children are created in torch.nonzero order,
  //      mcts.py:84-87): rank sort, promotions are already collapsed to one entry
  if (run_legal) {
    for (int j = lane; j < nlegal; j += 64) {
      const uint16_t v = s->lflat[j];
      int rank = 0;
      for (int k = 0; k < nlegal; ++k) rank += s->lflat[k] < v;
      s->lsorted[rank] = v;
    }
  }
  __syncthreads();
}

// ================================================================================================
// k_board_ops: the batched Board API (one wave per position)
// ================================================================================================
enum { OP_LEGAL = 1, OP_RESULT = 2, OP_TAKE = 4 };

__global__ void __launch_bounds__(64) k_board_ops(DevCfg c, fpc_board *boards, int n, int ops, const int *player,
                                                  const int *flat, fpc_move *moves, int *counts, int *results,
                                                  int *err) {
  __shared__ WaveLds s;
  const int g = blockIdx.x;
  if (g >= n) return;
  const int lane = lane_id();
  lds_load_board(&s, &boards[g]);
  int e = 0;
  if (ops & OP_TAKE) {
    int from;
    const int to = flat_to(c, flat[g], &from);
    if (!make_move_wave(&s.b, from, to, c)) e |= ERR_MOVE;
  }
  if (ops & (OP_LEGAL | OP_RESULT)) {
    wave_position_ops(&s, c, (ops & OP_RESULT) != 0, (ops & OP_LEGAL) != 0, player ? player[g] : -1);
    e |= s.errbits;
    if (ops & OP_RESULT) { if (lane == 0) results[g] = s.result; }
    if (ops & OP_LEGAL) {
      const int nl = s.nlegal;
      if (lane == 0) counts[g] = nl;
      for (int k = lane; k < nl; k += 64) {
        const int i = s.lidx[k];
        fpc_move m;
        const uint32_t w = s.mw[i];
        m.from = s.mfrom[i]; m.to = (uint8_t)mv_to(w); m.capture = mv_cap(w); m.promo = (uint8_t)mv_promo(w);
        m.flat = s.lflat[k]; m.pad = 0;
        moves[(size_t)g * FPC_MAX_MOVES + k] = m;
      }
    }
  }
  lds_store_board(&s, &boards[g]);
  if (lane == 0) err[g] = e;
}

// ================================================================================================
// k_attack_maps: the attacked-square queries of the binding surface (wrapper.cpp:201-206), one wave per position:
//   maps 0..3  fpchess::Board::IsAttackedByPlayer(location, colour) (src/cpp/board.cpp:142-210) -- its OWN probe set, not
//              the engine's: pawns / knights / kings on the array (BoardLocation::Present(), engine/board.h:194-201), and
//              eight rays that end at the ARRAY edge, i.e. run through the cut corners; the first piece on a ray attacks
//              if it is a bishop (diagonals), rook (lines) or queen -- of whichever colour it is, which is the colour's bit;
//   maps 4..5  chess::Board::IsAttackedByTeam(team, location) (engine/board.cpp:606-787) = attacked_virtual on the position.
// Every row x column of the array is a location, cut corners included (the double loops of board.cpp:120-140, :212-232).
// out: [n][6][RR] bytes, 1 = attacked.
// ================================================================================================
__device__ inline uint32_t attacked_by_players(const fpc_board *b, const DevCfg &c, int sq) {
  const int R = c.R, lr = row_of(c, sq), lc = sq - lr * R;
  uint32_t m = 0;
  for (int k = 0; k < 8; ++k) {                       // the eight neighbours: pawns (:152-161) and kings (:200-207)
    const int kk = k < 4 ? k : k + 1;
    const int dr = kk / 3 - 1, dc = kk % 3 - 1;
    const int r = lr + dr, cc = lc + dc;
    if (!in_array(c, r, cc)) continue;
    const uint8_t p = b->sq[r * R + cc];
    if (!present(p)) continue;
    const int col = colour_of(p), t = type_of(p);
    if (t == KING) m |= 1u << col;
    // PawnAttacks(pawn, colour, location), engine/board.cpp:583-604: (row_diff, col_diff) = location - pawn = (-dr, -dc)
    const bool patt = (col == 0 && dr == 1 && dc != 0) || (col == 1 && dc == -1 && dr != 0) || (col == 2 && dr == -1 && dc != 0) ||
                      (col == 3 && dc == 1 && dr != 0);
    if (t == PAWN && patt) m |= 1u << col;
  }
  for (int k = 0; k < 8; ++k) {                       // knights (:164-171)
    const int dr = (k & 4) ? ((k & 2) ? 1 : -1) : ((k & 2) ? 2 : -2);
    const int dc = (k & 4) ? ((k & 1) ? 2 : -2) : ((k & 1) ? 1 : -1);
    const int r = lr + dr, cc = lc + dc;
    if (!in_array(c, r, cc)) continue;
    const uint8_t p = b->sq[r * R + cc];
    if (present(p) && type_of(p) == KNIGHT) m |= 1u << colour_of(p);
  }
  for (int k = 0; k < 8; ++k) {                       // sliders (:174-197): the first piece on each ray
    const int kk = k < 4 ? k : k + 1;
    const int dr = kk / 3 - 1, dc = kk % 3 - 1;
    const bool diag = dr != 0 && dc != 0;
    int r = lr + dr, cc = lc + dc;
    while (in_array(c, r, cc)) {
      const uint8_t p = b->sq[r * R + cc];
      if (present(p)) {
        const int t = type_of(p);
        if (t == QUEEN || (t == BISHOP && diag) || (t == ROOK && !diag)) m |= 1u << colour_of(p);
        break;
      }
      r += dr; cc += dc;
    }
  }
  return m;
}

__global__ void __launch_bounds__(64) k_attack_maps(DevCfg c, const fpc_board *boards, int n, uint8_t *out) {
  __shared__ WaveLds s;
  const int g = blockIdx.x;
  if (g >= n) return;
  lds_load_board(&s, &boards[g]);
  uint8_t *o = out + (size_t)g * 6 * c.RR;
  for (int sq = lane_id(); sq < c.RR; sq += 64) {
    const uint32_t pm = attacked_by_players(&s.b, c, sq);
    for (int col = 0; col < 4; ++col) o[col * c.RR + sq] = (uint8_t)((pm >> col) & 1u);
    for (int team = 0; team < 2; ++team)
      o[(4 + team) * c.RR + sq] = attacked_virtual(&s.b, c, FPC_NO_SQ, FPC_NO_SQ, 0, FPC_NO_SQ, FPC_NO_SQ, 0, sq, team) ? 1 : 0;
  }
}

// ================================================================================================
// k_encode: Board::GetEncodedStates (board.cpp:305-356).  plane = 6*((colour-turn)&3) + type - 1,
// -1 wrapping to 23 (Q7); whole batch rotated by the turn of the FIRST leaf (Q6).
// mode 0: f32 NCHW [G,24,R,R]   (reference layout; external evaluators, parity tests)
// mode 1: 16-bit NHWC on the zero-bordered (R+2)x(R+2) grid, 32 channels (24 + 8 zero) -- the
//         input image of the internal MFMA conv stack.  one16 = bit pattern of 1.0 in the NN dtype.
// ================================================================================================
__device__ __forceinline__ int first_leaf_turn(const int *leaf_node, const int *leaf_turn, int G) {
  const int lane = lane_id();
  int found = -1;
  for (int base = 0; base < G && found < 0; base += 64) {
    const int g = base + lane;
    const bool has = g < G && leaf_node[g] >= 0;
    const unsigned long long bal = __ballot(has);
    if (bal) found = base + (int)__ffsll((long long)bal) - 1;
  }
  return found < 0 ? 0 : leaf_turn[found];
}

__global__ void __launch_bounds__(64) k_encode(DevCfg c, const fpc_board *boards, int board_stride,
                                               const int *slot_of, const int *leaf_turn, int G, int mode,
                                               float *out_f32, uint16_t *out_nhwc, uint16_t one16,
                                               int fixed_rot /* <0: rotation from first live leaf */) {
  const int g = blockIdx.x;
  if (g >= G) return;
  const int lane = lane_id();
  const int slot = slot_of ? slot_of[g] : 0;   // for the search: leaf board slot (or -1 dead)
  const int R = c.R, RR = c.RR;
  const bool live = slot >= 0;
  const fpc_board *b = live ? &boards[(size_t)g * board_stride + slot] : nullptr;
  const int turn = live ? b->turn : 0;
  // batch-wide rotation by the first state's turn (Q6); FPC_RULES_ROTATION: every sample by its own turn
  const int k = (c.rules & FPC_RULES_ROTATION) ? turn : (fixed_rot >= 0 ? fixed_rot : first_leaf_turn(slot_of, leaf_turn, G));
  if (mode == 0) {
    float *o = out_f32 + (size_t)g * 24 * RR;
    for (int pos = lane; pos < RR; pos += 64) {
      int plane = -1;
      if (live) {
        const uint8_t p = b->sq[rot90_src(R, k, pos / R, pos % R)];
        if (present(p)) plane = piece_plane(p, turn, c.rules);
      }
      for (int pl = 0; pl < 24; ++pl) o[(size_t)pl * RR + pos] = pl == plane ? 1.0f : 0.0f;
    }
  } else {
    const int P = R + 2;
    uint16_t *o = out_nhwc + (size_t)g * P * P * 32;
    for (int pos = lane; pos < RR; pos += 64) {
      int plane = -1;
      const int i = pos / R, j = pos % R;
      if (live) {
        const uint8_t p = b->sq[rot90_src(R, k, i, j)];
        if (present(p)) plane = piece_plane(p, turn, c.rules);
      }
      uint32_t *row = reinterpret_cast<uint32_t *>(o + ((size_t)(i + 1) * P + (j + 1)) * 32);
      for (int w = 0; w < 16; ++w) {
        uint32_t v = 0;
        if (plane == 2 * w) v = one16; else if (plane == 2 * w + 1) v = (uint32_t)one16 << 16;
        row[w] = v;
      }
    }
  }
}

// legal-move mask (four_player_chess_board.py:36-56): dense 0/1 [n,A_ch,R,R] f32 in absolute coords
__global__ void __launch_bounds__(64) k_mask_from_moves(DevCfg c, const fpc_move *moves, const int *counts, int n,
                                                         float *out) {
  const int g = blockIdx.x;
  if (g >= n) return;
  const int lane = lane_id();
  float *o = out + (size_t)g * c.A;
  for (int i = lane; i < c.A; i += 64) o[i] = 0.f;
  __syncthreads();
  for (int k = lane; k < counts[g]; k += 64) o[moves[(size_t)g * FPC_MAX_MOVES + k].flat] = 1.0f;
}

// ================================================================================================
// k_search_init: fresh root per game (mcts.py:29-32: Node(C, game, visit_count=1); Tree::born)
// ================================================================================================
__global__ void __launch_bounds__(64) k_search_init(Tree t, int G, const fpc_board *roots) {
  const int g = blockIdx.x;
  if (g >= G) return;
  const int lane = lane_id();
  {  // root state -> board-pool slot 0 of this game
    const uint32_t *src = reinterpret_cast<const uint32_t *>(&roots[g]);
    uint32_t *dst = reinterpret_cast<uint32_t *>(&t.boards[(size_t)g * t.board_cap]);
    dst[lane] = src[lane];
    if (lane < 8) dst[64 + lane] = src[64 + lane];
  }
  if (lane != 0) return;
  const size_t nb = (size_t)g * t.node_cap;
  t.N[nb] = t.born; t.W[nb] = 0.0; t.P[nb] = 0.f; t.mv[nb] = 0xffff; t.parent[nb] = -1; t.child0[nb] = -1; t.nch[nb] = 0;
  t.bslot[nb] = 0;
  t.nnodes[g] = 1; t.nboards[g] = 1; t.alive[g] = 1; t.sims_done[g] = 0; t.err[g] = 0;
  t.leaf_node[g] = -1; t.leaf_slot[g] = -1; t.leaf_turn[g] = 0; t.nlegal[g] = 0;
}

// root read-back (alphazero.py:104-110 reads GetChildren / GetFlatIndex / GetVisitCount)
__global__ void __launch_bounds__(64) k_root_children(Tree t, int G, int maxc, int *flat, int *visits, float *prior,
                                                      double *wsum, int *meta, fpc_board *roots_out) {
  const int g = blockIdx.x;
  if (g >= G) return;
  const int lane = lane_id();
  const size_t nb = (size_t)g * t.node_cap;
  const int c0 = t.child0[nb], nc = c0 < 0 ? 0 : (int)t.nch[nb];
  for (int k = lane; k < nc && k < maxc; k += 64) {
    const size_t o = (size_t)g * maxc + k;
    flat[o] = t.mv[nb + c0 + k]; visits[o] = t.N[nb + c0 + k]; prior[o] = t.P[nb + c0 + k]; wsum[o] = t.W[nb + c0 + k];
  }
  {
    const uint32_t *src = reinterpret_cast<const uint32_t *>(&t.boards[(size_t)g * t.board_cap]);
    uint32_t *dst = reinterpret_cast<uint32_t *>(&roots_out[g]);
    dst[lane] = src[lane];
    if (lane < 8) dst[64 + lane] = src[64 + lane];
  }
  if (lane == 0) { meta[g * 3 + 0] = t.N[nb]; meta[g * 3 + 1] = nc; meta[g * 3 + 2] = t.sims_done[g]; }
}

// fpc_search_proofs: the statuses of each root and of its children in the tree's child order
__global__ void __launch_bounds__(64) k_root_proofs(Tree t, int G, int maxc, uint8_t *root_proof, uint8_t *child_proof) {
  const int g = blockIdx.x;
  if (g >= G) return;
  const int lane = lane_id();
  const size_t nb = (size_t)g * t.node_cap;
  const int c0 = t.child0[nb], nc = c0 < 0 ? 0 : (int)t.nch[nb];
  for (int k = lane; k < maxc; k += 64) child_proof[(size_t)g * maxc + k] = k < nc ? t.S[nb + c0 + k] : (uint8_t)FPC_PROOF_UNKNOWN;
  if (lane == 0) root_proof[g] = t.S[nb];
}

// Policy target pruning (fpc_search_set_forced; the numeric spec is in include/fpc_engine.h and DESIGN 5.11): the pruned
// visit counts T_k of the children c0 .. c0 + nc - 1 of game nb's root, from the STORED statistics, f64 as written.  All 64
// lanes call; sink(k, T_k) is called once for every k < nc by the lane that owns child k (k % 64).  b, the first child with
// the largest N, is the only thing found across lanes (a ballot per pass of 64 and a scalar lane read); each lane then
// walks its own child's count down, at most sqrt(factor * max_sims) trips.  Reads the tree and writes nothing into it.
template <class Sink>
__device__ __forceinline__ void root_targets(const Tree &t, size_t nb, int c0, int nc, double Cpuct, Sink &&sink) {
  const int lane = lane_id();
  int b = -1, Nb = 0;
  for (int base = 0; base < nc; base += 64) {
    const int k = base + lane;
    const int Nk = k < nc ? t.N[nb + c0 + k] : -1;
    int cur = 0, top = wave_read(Nk, 0);       // lane 0 of a pass always owns a child
    for (;;) {                                 // the first lane with the pass's largest N, select_game's way
      const unsigned long long gt = __ballot(Nk > top);
      if (!gt) break;
      cur = (int)__ffsll((long long)gt) - 1;
      top = wave_read(Nk, cur);
    }
    if (b < 0 || top > Nb) { b = base + cur; Nb = top; }
  }
  if (b < 0) return;                           // no children
  const int Np = t.N[nb];
  const double sq = sqrt((double)Np);
  double ub = 0.0;
  if (Nb > 0) ub = -(t.W[nb + c0 + b] / (double)Nb) + Cpuct * (double)t.P[nb + c0 + b] * sq / (double)(1 + Nb);
  for (int k = lane; k < nc; k += 64) {
    const int Nk = t.N[nb + c0 + k];
    int T = Nk;
    if (Nb > 0 && k != b && Nk > 0) {
      const double Pk = (double)t.P[nb + c0 + k];
      const int F = (int)sqrt(t.forced * Pk * (double)Np);
      const double q = -(t.W[nb + c0 + k] / (double)Nk), a = Cpuct * Pk * sq;
      for (int f = 0; f < F; ++f) {
        if (T == 0 || q + a / (double)T >= ub) break;
        T = T - 1;
      }
      if (T < Nk && T <= 1) T = 0;             // a child reduced to a single playout is pruned outright
    }
    sink(k, T);
  }
}

// fpc_search_targets: the pruned visit counts of each root's children in the tree's child order (prune == 0, forcing not
// in effect: the stored counts), entries past a root's children 0
__global__ void __launch_bounds__(64) k_root_targets(Tree t, int G, int maxc, double Cpuct, int prune, int *target) {
  const int g = blockIdx.x;
  if (g >= G) return;
  const int lane = lane_id();
  const size_t nb = (size_t)g * t.node_cap;
  const int c0 = t.child0[nb], nc = c0 < 0 ? 0 : (int)t.nch[nb];
  int *out = target + (size_t)g * maxc;
  for (int k = lane; k < maxc; k += 64) out[k] = k < nc ? t.N[nb + c0 + k] : 0;
  if (t.fast != nullptr && t.fast[g]) prune = 0;     // a fast search's target is not pruned (fpc_search_set_fast_rows)
  // the same lane owns child k in both loops: its second store follows its first
  if (prune) root_targets(t, nb, c0, nc, Cpuct, [&](int k, int T) { if (k < maxc) out[k] = T; });
}

// training tuples (alphazero.py:104-112): root mailbox + side to move + sparse pi of a finished search.
// prune != 0 (forced playouts are in effect): the pruned counts T_k stand where the visit counts N_k stand.
__global__ void __launch_bounds__(64) k_collect_tuples(Tree t, int G, const int *game_id, int ply, double Cpuct, int prune, fpc_tuple *out) {
  const int g = blockIdx.x;
  if (g >= G) return;
  const int lane = lane_id();
  fpc_tuple *rec = out + g;
  const fpc_board *root = &t.boards[(size_t)g * t.board_cap];
  const size_t nb = (size_t)g * t.node_cap;
  const int c0 = t.child0[nb], nc = c0 < 0 ? 0 : (int)t.nch[nb];
  for (int i = lane; i < FPC_MAX_SQ; i += 64) rec->sq[i] = root->sq[i];
  for (int k = lane; k < FPC_TUPLE_MAXC; k += 64) {
    const bool in = k < nc;
    rec->flat[k] = in ? t.mv[nb + c0 + k] : (uint16_t)0;
    rec->visits[k] = in ? (uint16_t)t.N[nb + c0 + k] : (uint16_t)0;
  }
  // a fast search (fpc_search_set_fast_rows): the stored counts stay, and the record says so
  const int fast = t.fast != nullptr && t.fast[g] ? 1 : 0;
  if (fast) prune = 0;
  // the same lane owns child k in both loops: its second store follows its first
  if (prune) root_targets(t, nb, c0, nc, Cpuct, [&](int k, int T) { if (k < FPC_TUPLE_MAXC) rec->visits[k] = (uint16_t)T; });
  if (lane < 44) rec->pad1[lane] = 0;
  if (lane == 0) {
    rec->turn = root->turn; rec->flags = (uint8_t)(fast ? FPC_TUPLE_FAST : 0);
    rec->n = (uint16_t)(nc < FPC_TUPLE_MAXC ? nc : FPC_TUPLE_MAXC);
    rec->z = 0.f; rec->game = game_id ? game_id[g] : g; rec->ply = ply;
  }
}

// z by (game, team of the side to move): alphazero.py:128-137 / :161-175
__global__ void __launch_bounds__(256) k_tuples_set_z(fpc_tuple *recs, int count, const int *game_id, const float *z0, const float *z1, int n) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= count) return;
  const int game = recs[i].game;
  for (int k = 0; k < n; ++k)
    if (game_id[k] == game) { recs[i].z = (recs[i].turn & 1) ? z1[k] : z0[k]; return; }
}

// ================================================================================================
// k_play_ply (fpc_search_play, opt-in; the numeric spec is in include/fpc_engine.h and DESIGN 5.4): one wave per game
// of a FINISHED search picks the move to play from the root's children, makes it on a copy of the root state (board
// slot 0) and runs GetGameResult for the side to move -- k_board_ops' OP_TAKE then OP_RESULT on that state.  Reads the
// tree and writes nothing into it.
//   argmax == 0: weight of child k = powtab[N_k] (pow(N, 1/temperature), tabulated by the host libm); all lanes fetch
//                the weights into LDS in passes of 64, then ONE lane adds them strictly left to right in f64 -- the
//                order is the spec (a wave scan rounds differently off temperature 1) -- takes x = uniform * S and
//                walks the same sums again to the first c_k > x (the last child if there is none); S == 0 (no child has a
//                visit: FPC_RULES_VISITS only) picks child min(nc - 1, (int)(uniform * nc));
//   argmax != 0: the first child with the largest N.
// A game with a search error or a childless root gets flat = result = -1 and its root state.  A move that cannot be made
// sets ERR_MOVE in err[] (the call's own array, not t.err) and skips GetGameResult.
// ================================================================================================
// solve != 0 (the solver is in effect): a root proven WIN plays its first child with status LOSS, a root proven DRAW its
// first child with status DRAW, at every temperature; a root proven LOSS or unknown takes the draw above.
// prune != 0 (forced playouts are in effect): the draw is from the pruned counts T_k (root_targets) instead of N_k.
__global__ void __launch_bounds__(64) k_play_ply(DevCfg c, Tree t, int G, const double *powtab, int powtab_n, int argmax,
                                                 const double *uniform, int solve, double Cpuct, int prune, int *flat, int *result,
                                                 fpc_board *next, int *err) {
  __shared__ WaveLds s;
  __shared__ double wt[FPC_MAX_MOVES];
  const int g = blockIdx.x;
  if (g >= G) return;
  const int lane = lane_id();
  const size_t nb = (size_t)g * t.node_cap;
  const int c0 = t.child0[nb], gerr = t.err[g];
  int nc = c0 < 0 ? 0 : (int)t.nch[nb];
  if (nc > FPC_MAX_MOVES) nc = FPC_MAX_MOVES;
  const double u = uniform[g];
  const int rootS = solve ? (int)t.S[nb] : FPC_PROOF_UNKNOWN;
  lds_load_board(&s, &t.boards[(size_t)g * t.board_cap]);
  if (gerr != 0 || nc == 0) {
    lds_store_board(&s, &next[g]);
    if (lane == 0) { flat[g] = -1; result[g] = -1; err[g] = 0; }
    return;
  }
  if (t.fast != nullptr && t.fast[g]) prune = 0;     // a fast search draws from the stored counts (fpc_search_set_fast_rows)
  if (prune) {                                       // wave-uniform; T_k <= N_k, the clamp as below
    root_targets(t, nb, c0, nc, Cpuct, [&](int k, int n) { wt[k] = argmax ? (double)n : powtab[n < 0 ? 0 : n < powtab_n ? n : powtab_n - 1]; });
  } else
  for (int base = 0; base < nc; base += 64) {
    const int k = base + lane;
    if (k < nc) {
      const int n = t.N[nb + c0 + k];
      // a visit count is at most 1 + max_sims and the table holds max_sims + 16 entries: the clamp only keeps a
      // corrupted count from reading outside it
      wt[k] = argmax ? (double)n : powtab[n < 0 ? 0 : n < powtab_n ? n : powtab_n - 1];
    }
  }
  // the solver's pick: the first child with the status a proven root asks for (-1: none, the draw decides)
  int forced = -1;
  if (rootS == FPC_PROOF_WIN || rootS == FPC_PROOF_DRAW) {       // wave-uniform
    const int want = rootS == FPC_PROOF_WIN ? FPC_PROOF_LOSS : FPC_PROOF_DRAW;
    for (int base = 0; base < nc && forced < 0; base += 64) {
      const int k = base + lane;
      const unsigned long long hit = __ballot(k < nc && (int)t.S[nb + c0 + k] == want);
      if (hit) forced = base + (int)__ffsll((long long)hit) - 1;
    }
  }
  __syncthreads();
  if (lane == 0) {
    int pick = 0;
    if (forced >= 0) {
      pick = forced;
    } else if (argmax) {
      double best = wt[0];
      for (int k = 1; k < nc; ++k)
        if (wt[k] > best) { best = wt[k]; pick = k; }
    } else {
      double S = 0.0;
      for (int k = 0; k < nc; ++k) S = S + wt[k];
      if (S == 0.0) {                                // no child has a visit (FPC_RULES_VISITS only): uniform over the children
        pick = (int)(u * nc);
        if (pick > nc - 1) pick = nc - 1;
      } else {
        const double x = u * S;
        double ck = 0.0;
        pick = nc - 1;
        for (int k = 0; k < nc; ++k) {
          ck = ck + wt[k];
          if (ck > x) { pick = k; break; }
        }
      }
    }
    s.first_legal = (int)t.mv[nb + c0 + pick];     // broadcast through LDS
  }
  __syncthreads();
  const int fl = s.first_legal;
  __syncthreads();
  int from;
  const int to = flat_to(c, fl, &from);
  int e = make_move_wave<3>(&s.b, from, to, c) ? 0 : ERR_MOVE;
  int res = -1;
  if (!e) {
    wave_position_ops<3>(&s, c, true, false, -1);
    e = s.errbits;
    res = s.result;
  }
  lds_store_board(&s, &next[g]);
  if (lane == 0) { flat[g] = fl; result[g] = res; err[g] = e; }
}

// ================================================================================================
// device-resident replay (fpc_replay_*): the rings hold fpc_tuple records; a minibatch is decoded in one launch
// ================================================================================================
struct alignas(16) Vec16 { uint32_t w[4]; };      // one 16-byte access per lane (global_load/store_dwordx4)
static_assert(sizeof(fpc_tuple) == 80 * sizeof(Vec16), "k_replay_store copies a record as 64 + 16 16-byte pieces");

// m whole records src[src_idx[j]] -> ring slot dst_idx[j], one wave per record.  Destination index space: ring 0's slots,
// then ring 1's (d >= cap0: slot d - cap0 of ring 1).  The host guarantees that no two entries name the same destination.
__global__ void __launch_bounds__(64) k_replay_store(const fpc_tuple *src, const int *src_idx, fpc_tuple *ring0, fpc_tuple *ring1,
                                                     int cap0, const int *dst_idx, int m) {
  const int j = blockIdx.x;
  if (j >= m) return;
  const int lane = lane_id();
  const int d = dst_idx[j];
  const Vec16 *s = reinterpret_cast<const Vec16 *>(src + src_idx[j]);
  Vec16 *o = reinterpret_cast<Vec16 *>(d < cap0 ? ring0 + d : ring1 + (d - cap0));
  o[lane] = s[lane];
  if (lane < 16) o[64 + lane] = s[64 + lane];
}

// One training sample per workgroup: record ring[slot[i]] -> the trainer's dense row (alphazero.py:71-73, :104-110)
//   enc[i] [24,R,R]  what k_encode mode 0 writes for a board with this record's sq and turn, rotated by that turn
//                    (GetEncodedState per tuple: the sample's own rotation), under the engine's current rule set;
//   pi[i]  [A]       zero but pi[flat[k]] = (float)visits[k] / (float)S for k < n, S = sum of the visits as an integer;
//                    one IEEE f32 division, so the row has the bits of tuples.dense_pi (S <= 256 * 65535 < 2^24: torch's
//                    f32 sum is exact in any order).  n == 0 gives an all-zero row, and so does S == 0 (a root none of whose
//                    children has a visit, FPC_RULES_VISITS), as in dense_pi.  A flat >= A (never made by a search) is dropped;
//   z[i]             rec.z;
//   w[i]             (w not null: fpc_replay_batch_w) 0.0f for a record with FPC_TUPLE_FAST, else 1.0f.
// Thread k owns child k (RD_THREADS == FPC_TUPLE_MAXC).  Both rows leave as 16-byte stores, lane after lane (enc and pi
// rows start on 16-byte boundaries: 24*RR and A = 8(R+1)RR are multiples of 4 floats).  The at most 256 nonzeros of pi
// are 4-byte stores into the row this workgroup has just zeroed, ordered behind the zero fill by the barrier
// (k_mask_from_moves' idiom); they merge in L2 with the lines the fill left there.
constexpr int RD_THREADS = 256;
static_assert(RD_THREADS == FPC_TUPLE_MAXC && RD_THREADS >= FPC_MAX_SQ, "k_replay_decode: one thread per child, one per square");
__global__ void __launch_bounds__(RD_THREADS) k_replay_decode(DevCfg c, const fpc_tuple *ring, const int *slot, int n,
                                                              float *enc, float *pi, float *z, float *w) {
  __shared__ int8_t s_plane[FPC_MAX_SQ];           // input plane of the piece on each square of the rotated board, -1 empty
  __shared__ int s_sum[RD_THREADS / 64];
  const int i = blockIdx.x;
  if (i >= n) return;
  const int tid = (int)threadIdx.x;
  const fpc_tuple *rec = ring + slot[i];
  const int R = c.R, RR = c.RR, turn = rec->turn & 3;
  if (tid < RR) {
    const int row = row_of(c, tid);
    const uint8_t p = rec->sq[rot90_src(R, turn, row, tid - row * R)];
    s_plane[tid] = (int8_t)(present(p) ? piece_plane(p, turn, c.rules) : -1);
  }
  const int nc = rec->n < FPC_TUPLE_MAXC ? (int)rec->n : FPC_TUPLE_MAXC;
  const int flat = tid < nc ? (int)rec->flat[tid] : 0;
  const int vis = tid < nc ? (int)rec->visits[tid] : 0;
  int s = vis;
  for (int m = 32; m; m >>= 1) s += __shfl_xor(s, m);
  if ((tid & 63) == 0) s_sum[tid >> 6] = s;
  __syncthreads();
  const int S = s_sum[0] + s_sum[1] + s_sum[2] + s_sum[3];
  if (tid == 0) {
    z[i] = rec->z;
    if (w != nullptr) w[i] = (rec->flags & FPC_TUPLE_FAST) ? 0.0f : 1.0f;     // fpc_replay_batch_w: the policy-loss weight
  }
  float4 *e4 = reinterpret_cast<float4 *>(enc + (size_t)i * 24 * RR);
  // (plane, square) of a piece's first float, carried from piece to piece: one division per thread, none per piece
  const int dplane = (4 * RD_THREADS) / RR, dpos = 4 * RD_THREADS - dplane * RR;
  int plane0 = (4 * tid) / RR, pos0 = 4 * tid - plane0 * RR;
  for (int q = tid; q < 6 * RR; q += RD_THREADS) {
    int plane = plane0, pos = pos0;                         // a 16-byte piece may straddle two planes (RR odd)
    float o[4];
    for (int j = 0; j < 4; ++j) {
      o[j] = s_plane[pos] == plane ? 1.0f : 0.0f;
      if (++pos == RR) { pos = 0; ++plane; }
    }
    float4 v;
    v.x = o[0]; v.y = o[1]; v.z = o[2]; v.w = o[3];
    e4[q] = v;
    plane0 += dplane;
    pos0 += dpos;
    if (pos0 >= RR) { pos0 -= RR; ++plane0; }
  }
  float *prow = pi + (size_t)i * c.A;
  float4 *p4 = reinterpret_cast<float4 *>(prow);
  float4 zero;
  zero.x = zero.y = zero.z = zero.w = 0.0f;
  const bool has = tid < nc && flat < c.A;
  const float val = S > 0 ? (float)vis / (float)S : 0.0f;      // visits that sum to 0 (FPC_RULES_VISITS): a zero row
  for (int q = tid; q < (c.A >> 2); q += RD_THREADS) p4[q] = zero;
  __syncthreads();
  if (has) prow[flat] = val;
}

// ================================================================================================
// k_select: get_expandable_leaves / Node::ChooseLeaf (mcts.py:18-26, node.cpp:19-78)
// ================================================================================================
// Node::Backpropagate (node.cpp:133-142): value_sum += (double)v ; visit_count += 1 ; v = -v (f32)
__device__ __forceinline__ void backprop_lane0(const Tree &t, size_t nb, int n, float v) {
  while (n >= 0) {
    t.W[nb + n] += (double)v;
    t.N[nb + n] += 1;
    v = -v;
    n = t.parent[nb + n];
  }
}

// BackpropagateNodes (node.cpp:118-126) along the descent path k_select recorded: path[len-1] is the
// leaf (+v), its parent gets -v, ... -- every node of the path is touched once, so the lanes of one
// wave update them independently instead of one lane chasing parent pointers.
__device__ __forceinline__ void backprop_path(const Tree &t, size_t nb, int g, float v, int len, int node_of_lane) {
  // len = path_len[g] and node_of_lane = path[lane] (lane < len, first 64 entries) were fetched by the caller together
  // with everything else whose address needs no other load
  const int *path = t.path + (size_t)g * t.path_cap;
  for (int k = lane_id(); k < len; k += 64) {
    const int node = k < 64 ? node_of_lane : path[k];
    const float sv = ((len - 1 - k) & 1) ? -v : v;
    t.W[nb + node] += (double)sv;
    t.N[nb + node] += 1;
  }
}

// The MCTS solver (fpc_search_set_solver).  pv: the value a proven node backs up, from its own side to move.
__device__ __forceinline__ float proof_value(int st) { return st == FPC_PROOF_WIN ? 1.0f : st == FPC_PROOF_LOSS ? -1.0f : 0.0f; }

// Node `cn` has just been proven `cs` (all 64 lanes call with the same arguments): store it and carry the proof towards
// the root.  With c the node just proven and p its parent: stop without a parent or at a p that is proven already; c LOSS
// makes p WIN; otherwise p's children are read 64 per pass (at most FPC_MAX_MOVES / 64 passes) and combined with ballots --
// one unknown child stops the walk, all WIN make p LOSS, anything else DRAW.  The status just given to c is taken from
// the register, not read back: lane 0's store need not be visible to the other lanes.  A status never changes once set.
__device__ __forceinline__ void prove_upward(const Tree &t, size_t nb, int cn, int cs) {
  const int lane = lane_id();
  for (;;) {
    if (lane == 0) t.S[nb + cn] = (uint8_t)cs;
    const int p = t.parent[nb + cn];
    if (p < 0) return;
    // p's status as LANE 0 sees it, for every lane: lane 0 is the only writer, and nothing orders its stores against
    // the other lanes' loads -- a lane that read S[p] after lane 0 had gone on to prove p would leave the walk alone
    const int pS = wave_read((int)t.S[nb + p], 0), pc0 = t.child0[nb + p], pnc = t.nch[nb + p];
    if (pS != FPC_PROOF_UNKNOWN) return;
    int ps = FPC_PROOF_WIN;
    if (cs != FPC_PROOF_LOSS) {
      bool all_win = true;
      for (int base = 0; base < pnc; base += 64) {
        const int i = base + lane;
        int st = FPC_PROOF_WIN;                // lanes past the children: neutral
        if (i < pnc) st = pc0 + i == cn ? cs : (int)t.S[nb + pc0 + i];
        if (__ballot(st == FPC_PROOF_UNKNOWN)) return;
        if (__ballot(st != FPC_PROOF_WIN)) all_win = false;
      }
      ps = all_win ? FPC_PROOF_LOSS : FPC_PROOF_DRAW;
    }
    cn = p;
    cs = ps;
  }
}

// Leaf-parallel search (fpc_search_set_leaves, K leaves per game per step): row r = k*G + g holds the k-th leaf game g
// selected in this step.  VL [G][node_cap] counts the pending visits of a node (0 outside a step); the descent sees
// N' = N + VL and W' = W -+ vl*VL (lower Q on pending paths), a descent that ends on a pending leaf is a collision.
struct LeafPar {
  int *VL;
  double vl;
};
struct OneLeaf { int k, G; };   // select_game's context for one leaf per game (never dereferenced: that instance is the one-leaf selection)
struct LeafRow {         // ... and for descent k of a leaf-parallel step
  LeafPar lp;
  int k, G;
  bool live;             // out: the row is live
  int leaf_vl, best_vl, cvl;   // the descent's pending-visit counts: node it stands on, best child so far, this lane's child
};

// One game's selection step, executed by one wave (all 64 lanes call; `s` is the wave's LDS image).
// The chosen leaf goes to leaf_node/leaf_slot/leaf_turn, or to their _nx twins when `to_next`, at index g.
// MULTI (leaf-parallel, descent k of G games): the per-leaf outputs go to row k*G + g; effective statistics, collision
// check, leaf_slot holds the GLOBAL pool index g*board_cap + slot, VL += 1 along the path of a live row.
// M: OneLeaf (m null), or LeafRow (leaf-parallel; m->live is set when the row is live).
// FPU: first-play urgency is on (fpc_search_set_fpu, FPC_FPU_PARENT).  A separate instance in kernels of its own -- every
// selecting kernel exists as <false> and <true>, and the host launches the one t.fpu_mode asks for -- so that the kernels
// without it are instruction for instruction what they were: a lone wave per game pays for every instruction it fetches
// (both instances in one kernel cost 1 us per step, the extra scalar registers of one shared instance 0.3 us).
// SOLVE: the MCTS solver is in effect (fpc_search_set_solver under FPC_RULES_PUCT | FPC_RULES_TERMINAL), for
// the same reason a second switch of the same kind: every selecting kernel exists as <FPU, SOLVE> in four instances, and the
// <*, false> ones neither load nor store a status.  t.S is not null in a SOLVE instance (the host launches one only then).
//   1. a root with children and a status: a dead row, nothing is written (the status rides with the root's other fields);
//   2. a child with status WIN is no candidate of the argmax (its status rides with its N / W / P / child0);
//   3. a chosen child with a status ends the descent: pv(status) is backed up from it, sims_done += 1, a dead row that
//      ends the game's selection of the step -- before the collision check;
//   4. an unknown leaf whose game is over: the terminal backup, then the leaf's status from the value backed up and the
//      proof's way up (prove_upward).
// FORCE: forced playouts are in effect (fpc_search_set_forced under FPC_RULES_PUCT | FPC_RULES_VISITS), a third
// switch of the same kind: every selecting kernel exists as <FPU, SOLVE, FORCE> in eight instances, and the <*, *, false>
// ones neither load the factor nor test for the root level.  At the root level (n == 0) a child with 0 < N' < sqrt(factor *
// P * N'_root) gets u = +infinity; the argmax, the solver's exclusion and everything after the choice are unchanged.
template <class M, bool FPU, bool SOLVE, bool FORCE, bool MULTI = !std::is_same<M, OneLeaf>::value>
__device__ inline void select_game(WaveLds &s, const DevCfg &c, const Tree &t, int g, double Cpuct, const double *logtab, bool to_next, M *m) {
#define FPC_ROW (MULTI ? m->k * m->G + g : g)     // the leaf's row (folded to g for one leaf per game)
  const int lane = lane_id();
  int *const leaf_node = to_next ? t.leaf_node_nx : t.leaf_node;
  int *const leaf_slot = to_next ? t.leaf_slot_nx : t.leaf_slot;
  int *const leaf_turn = to_next ? t.leaf_turn_nx : t.leaf_turn;
  const size_t nb = (size_t)g * t.node_cap;
  // Everything whose address depends on no other load goes out FIRST, in one round trip (a lone wave per CU pays the
  // full memory latency for every dependent load: the chain of round trips, not the arithmetic, is this function's
  // floor): the liveness flag, the root's fields, the board-pool fill level the leaf materialisation will need.
  const int is_alive = t.alive[g];
  int c0 = t.child0[nb], nc = t.nch[nb], Nn = t.N[nb];
  int slot = t.bslot[nb], parent_slot = -1;        // board-pool slot of node n / of its parent
  const int nboards0 = t.nboards[g];
  // Per-game budget (fpc_search_set_budget): descent k of a step is made only while sims_done + k < budget.  The two loads
  // go out with the batch above -- no dependent round trip -- and without budgets (null) none is issued.  sims_done is
  // the count at the start of the step's selection: a descent changes it only at a terminal leaf, which ends the step.
  int room = 1;
  if (t.budget != nullptr) room = t.budget[g] - t.sims_done[g] - (MULTI ? m->k : 0);
  // First-play urgency (fpc_search_set_fpu): the STORED W and N of the node the descent stands on.  The root's W goes out
  // with the batch above, and at every deeper level the chosen child's W rides along with best_c0 and the rest -- no
  // dependent round trip; the instance without it issues neither the load nor the lane read.
  double Wst = 0.0;
  if constexpr (FPU) Wst = t.W[nb];
  int Nst = Nn;
  int rootS = 0;                             // the solver: the root's status, with the batch above
  if constexpr (SOLVE) rootS = t.S[nb];
  // Playout cap (fpc_search_set_fast_rows): a fast game's root level is not forced.  The game's byte goes out with the batch
  // above, as the aligned word that holds it (the array is padded to whole words and zeroed when it is allocated): gfx950
  // has no scalar byte load, and the word is a scalar load issued beside the one of t.alive[g] and waited for with it.
  // With no mask the game's liveness word stands in and is ignored.  Wave-uniform; an instance without FORCE issues no load.
  bool force_here = FORCE;
  if constexpr (FORCE) {
    uint32_t word;
#ifdef FPC_EMUL
    const void *fw = t.fast != nullptr ? (const void *)(t.fast + (g & ~3)) : (const void *)(t.alive + g);
    __builtin_memcpy(&word, fw, sizeof word);      // host build: no access through a pointer of another type
#else
    const uint32_t *fw = t.fast != nullptr ? reinterpret_cast<const uint32_t *>(t.fast) + (g >> 2) : reinterpret_cast<const uint32_t *>(t.alive + g);
    word = *fw;
#endif
    force_here = t.fast == nullptr || ((word >> ((g & 3) * 8)) & 0xffu) == 0;
  }
  if constexpr (MULTI) { m->leaf_vl = m->lp.VL[nb]; Nn += m->leaf_vl; }
  if (!is_alive || room <= 0) {             // root already removed from the search (Q5), or the game is at its budget: a dead row
    if (lane == 0) { leaf_node[FPC_ROW] = -1; leaf_slot[FPC_ROW] = -1; }
    return;
  }
  if constexpr (SOLVE) {
    if (c0 >= 0 && rootS != FPC_PROOF_UNKNOWN) {     // a proven root with children: idle like a game at its budget
      if (lane == 0) { leaf_node[FPC_ROW] = -1; leaf_slot[FPC_ROW] = -1; }
      return;
    }
  }
  // ---- descent: SelectChild (node.cpp:49-78)
  //   ucb_i = W_i/N_i + C * sqrt( log(sqrt(N_parent)) / (1 + N_i) ) * P_i      (fp64, no contraction)
  //   strict '>' from -inf => lowest index wins ties, NaN never wins
  //   FPC_RULES_PUCT: -W_i/N_i + C P_i sqrt(N_parent) / (1 + N_i); a child with N_i' == 0 has q = 0, or under
  //   FPC_FPU_PARENT q = W_p/N_p - reduction from the parent's stored statistics (f64, as written)
  // Every level costs ONE dependent global round trip: the lanes that fetch the children's N/W/P also
  // fetch each child's (first child, child count, board-pool slot, move), so the chosen child's own children can
  // be requested as soon as the argmax is known, and at the leaf its slot, its parent's and its move are at hand.
  int n = 0, depth = 0, leaf_mv = 0xffff;
  bool fail = false;
  int proven = FPC_PROOF_UNKNOWN;            // the solver: the status of the proven child the descent ended on
  int *path = t.path + (size_t)FPC_ROW * t.path_cap;
  for (;;) {
    if (lane == 0 && depth < t.path_cap) path[depth] = n;
    ++depth;
    if (c0 < 0) break;
    // logtab[0] = log(sqrt(0)) is never read: a node with children has been backed up through at least once (its own
    // expansion), so N >= 1 here under FPC_RULES_VISITS too, where nodes are born with N = 0
    const double L = logtab[Nn];
    const double sqrtNp = sqrt((double)Nn);
    const double q0 = FPU ? Wst / (double)Nst - t.fpu_red : 0.0;     // the q of a child with N' == 0 (PUCT branch)
    double best = 0.0, best_W = 0.0;
    int besti = -1, best_c0 = -1, best_nc = 0, best_N = 0, best_slot = -1, best_mv = 0xffff;
    int best_S = FPC_PROOF_UNKNOWN;
    if constexpr (MULTI) m->best_vl = 0;
    for (int base = 0; base < nc; base += 64) {
      const int i = base + lane;
      double u = 0.0;
      bool valid = false;
      int Nc = 0, cc0 = -1, cnc = 0, cslot = -1, cmv = 0xffff;
      double Wraw = 0.0;                             // the child's stored W (no virtual loss)
      int cS = FPC_PROOF_UNKNOWN;                    // the child's status
      if constexpr (MULTI) m->cvl = 0;
      if (i < nc) {
        if constexpr (SOLVE) cS = t.S[nb + c0 + i];
        Nc = t.N[nb + c0 + i];
        double Wc = t.W[nb + c0 + i];
        double Pc = (double)t.P[nb + c0 + i];
        Wraw = Wc;
        if constexpr (MULTI) {                     // N' = N + VL;  W' = W - vl*VL (strict) / W + vl*VL (PUCT: Q = -W/N)
          m->cvl = m->lp.VL[nb + c0 + i];
          Nc += m->cvl;
          Wc = (c.rules & FPC_RULES_PUCT) ? Wc + m->lp.vl * (double)m->cvl : Wc - m->lp.vl * (double)m->cvl;
        }
        cc0 = t.child0[nb + c0 + i];
        cnc = t.nch[nb + c0 + i];
        cslot = t.bslot[nb + c0 + i];
        cmv = t.mv[nb + c0 + i];
        if (c.rules & FPC_RULES_PUCT) {
          // AlphaZero PUCT, the child's value seen from the parent: -W/N + C P sqrt(N_parent) / (1 + N)
          const double q = Nc > 0 ? -(Wc / (double)Nc) : q0;
          u = q + Cpuct * Pc * sqrtNp / (double)(1 + Nc);
          if constexpr (FORCE) {                     // in effect only under FPC_RULES_PUCT: this branch
            if (n == 0 && force_here && Nc > 0 && (double)Nc < sqrt(t.forced * Pc * (double)Nn)) u = __builtin_inf();
          }
        } else {
          const double q = Nc > 0 ? Wc / (double)Nc : 0.0;
          const double e = Cpuct * sqrt(L / (double)(1 + Nc));
          u = q + e * Pc;
        }
        valid = u > -__builtin_inf();
        if constexpr (SOLVE) valid = valid & (cS != FPC_PROOF_WIN);      // the move that loses is no candidate
      }
      // argmax with the reference's rule (strict '>': the FIRST maximum wins): start at the lowest valid lane and jump
      // to the lowest lane that beats the current one until none does -- about ln(children) rounds of two scalar lane
      // reads, a compare and a ballot, instead of six butterfly rounds of three LDS-crossbar shuffles each
      const unsigned long long live = __ballot(valid);
      int idx = 0x7fffffff, cur = 0;
      double ubest = -__builtin_inf();
      if (live) {                                  // wave-uniform
        cur = (int)__ffsll((long long)live) - 1;
        for (;;) {
          ubest = wave_read(u, cur);
          const unsigned long long gt = __ballot(valid && u > ubest);
          if (!gt) break;
          cur = (int)__ffsll((long long)gt) - 1;
        }
        idx = base + cur;
      }
      const int w_c0 = wave_read(cc0, cur), w_nc = wave_read(cnc, cur), w_N = wave_read(Nc, cur), w_slot = wave_read(cslot, cur), w_mv = wave_read(cmv, cur);
      if constexpr (MULTI) {
        const int w_vl = wave_read(m->cvl, cur);
        if (idx != 0x7fffffff && (besti < 0 || ubest > best)) m->best_vl = w_vl;
      }
      if constexpr (FPU) {
        const double w_W = wave_read(Wraw, cur);
        if (idx != 0x7fffffff && (besti < 0 || ubest > best)) best_W = w_W;
      }
      if constexpr (SOLVE) {
        const int w_S = wave_read(cS, cur);
        if (idx != 0x7fffffff && (besti < 0 || ubest > best)) best_S = w_S;
      }
      if (idx != 0x7fffffff && (besti < 0 || ubest > best)) { best = ubest; besti = idx; best_c0 = w_c0; best_nc = w_nc; best_N = w_N; best_slot = w_slot; best_mv = w_mv; }
    }
    if (besti < 0) { fail = true; break; }
    n = c0 + besti;
    c0 = best_c0; nc = best_nc; Nn = best_N;
    parent_slot = slot; slot = best_slot; leaf_mv = best_mv;
    if constexpr (MULTI) m->leaf_vl = m->best_vl;
    if constexpr (FPU) {
      Wst = best_W; Nst = best_N;
      if constexpr (MULTI) Nst -= m->best_vl;                  // best_N is the effective count N + VL
    }
    if constexpr (SOLVE) {
      if (best_S != FPC_PROOF_UNKNOWN) { proven = best_S; break; }   // the descent ends on a proven child
    }
  }
  FPC_TS(5);
  if (fail) {                                // node.cpp:72-75 throws
    if (lane == 0) { t.err[g] |= ERR_SELECT; t.alive[g] = 0; leaf_node[FPC_ROW] = -1; leaf_slot[FPC_ROW] = -1; }
    return;
  }
  if constexpr (SOLVE) {
    if (proven != FPC_PROOF_UNKNOWN) {       // the bookkeeping of a terminal backup: no board, no GetGameResult, no move generation
      if (lane == 0) {
        backprop_lane0(t, nb, n, proof_value(proven));
        t.sims_done[g] += 1;
        leaf_node[FPC_ROW] = -1;
        leaf_slot[FPC_ROW] = -1;
      }
      return;
    }
  }
  if constexpr (MULTI) {
    if (m->leaf_vl > 0) {                    // collision: a leaf already taken in this step; nothing is touched
      if (lane == 0) { leaf_node[FPC_ROW] = -1; leaf_slot[FPC_ROW] = -1; }
      return;
    }
  }
  // ---- leaf state: the reference copies + MakeMoves a Board for every child at expansion time
  //      (node.cpp:90-91); here it is materialised the first time the node is reached.
  const fpc_board *pool = t.boards + (size_t)g * t.board_cap;
  if (slot < 0) {
    lds_load_board(&s, &pool[parent_slot]);
    int from;
    const int to = flat_to(c, leaf_mv, &from);
    const bool moved = make_move_wave<MULTI + (FPU ? 4 : 0) + (SOLVE ? 8 : 0) + (FORCE ? 16 : 0)>(&s.b, from, to, c);
    if (lane == 0) {
      int e = moved ? 0 : ERR_MOVE;
      int ns = nboards0;                     // fetched with the root's fields; only this block ever changes it
      if (ns >= t.board_cap) { e |= ERR_CAP_BOARDS; ns = -1; } else { t.nboards[g] = ns + 1; t.bslot[nb + n] = ns; }
      s.first_legal = ns;                    // broadcast through LDS
      if (e) t.err[g] |= e;
    }
    __syncthreads();
    slot = s.first_legal;
    __syncthreads();
    if (slot < 0) {                          // board pool exhausted: the game leaves the search, nothing is overwritten
      if (lane == 0) { t.alive[g] = 0; leaf_node[FPC_ROW] = -1; leaf_slot[FPC_ROW] = -1; }
      return;
    }
  } else {
    lds_load_board(&s, &pool[slot]);
  }
  FPC_TS(6);
  // ---- GetGameResult (node.cpp:28-29) then, if in progress, GetLegalMoves
  //      (four_player_chess_board.py:38) on the same state, with their list reorderings
  wave_position_ops<MULTI + (FPU ? 4 : 0) + (SOLVE ? 8 : 0) + (FORCE ? 16 : 0)>(&s, c, true, true, -1);
  FPC_TS(12);
  lds_store_board(&s, &t.boards[(size_t)g * t.board_cap + slot]);
  const int res = s.result;
  if (lane == 0 && s.errbits) t.err[g] |= s.errbits;
  if (res != FPC_IN_PROGRESS) {              // node.cpp:31-42: back up 0 / -1, drop the root (Q5)
    if (lane == 0) {
      float v = res == FPC_STALEMATE ? 0.0f : -1.0f;
      bool leaves = true;
      if (c.rules & FPC_RULES_TERMINAL) {    // value by result, seen from the leaf's side to move; only a terminal ROOT leaves the search
        if (res != FPC_STALEMATE) v = (res == FPC_WIN_BG ? 1 : 0) == (s.b.turn & 1) ? 1.0f : -1.0f;
        leaves = n == 0;
      }
      backprop_lane0(t, nb, n, v);
      t.sims_done[g] += 1;
      if (leaves) t.alive[g] = 0;
      leaf_node[FPC_ROW] = -1;
      leaf_slot[FPC_ROW] = -1;
    }
    if constexpr (SOLVE) {                   // the leaf's status from the value just backed up (FPC_RULES_TERMINAL's: the solver
                                             // is in effect only under it), recomputed by every lane: the branch is wave-uniform
      const int st = res == FPC_STALEMATE ? FPC_PROOF_DRAW : (res == FPC_WIN_BG ? 1 : 0) == (s.b.turn & 1) ? FPC_PROOF_WIN : FPC_PROOF_LOSS;
      prove_upward(t, nb, n, st);
    }
    return;
  }
  const int nl = s.nlegal;
  uint16_t *lg = t.legal + (size_t)FPC_ROW * FPC_MAX_MOVES;
  for (int k = lane; k < nl; k += 64) lg[k] = s.lsorted[k];
  if (lane == 0) {
    leaf_node[FPC_ROW] = n; leaf_slot[FPC_ROW] = slot; leaf_turn[FPC_ROW] = s.b.turn;
    t.nlegal[FPC_ROW] = nl; t.path_len[FPC_ROW] = depth;
  }
  if constexpr (MULTI) {                     // the row is pending: VL += 1 on every node of its path, root through leaf
    __syncthreads();                         // lane 0's path stores are visible
    const int len = depth < t.path_cap ? depth : t.path_cap;
    for (int k = lane; k < len; k += 64) m->lp.VL[nb + path[k]] += 1;
    if (lane == 0) leaf_slot[FPC_ROW] = g * t.board_cap + slot;
    m->live = true;
  }
  FPC_TS(13);
#undef FPC_ROW
}
constexpr OneLeaf *ONE_LEAF = nullptr;

// K descents of one game in one step (leaf-parallel search): row k*G + g for k = 0, 1, ...  The first row that is not
// live (collision, terminal leaf, dead game, the game's budget reached) ends the game's selection for this step; its
// remaining rows are dead.  With the solver a proven root and a backup from a proven child end it the same way.
template <bool FPU, bool SOLVE, bool FORCE>
__device__ inline void select_game_multi(WaveLds &s, const DevCfg &c, const Tree &t, int G, int g, int K, double Cpuct,
                                         const double *logtab, bool to_next, const LeafPar &lp) {
  int k = 0;
  while (k < K) {
    LeafRow r{lp, k, G, false, 0, 0, 0};
    select_game<LeafRow, FPU, SOLVE, FORCE>(s, c, t, g, Cpuct, logtab, to_next, &r);
    ++k;
    if (!r.live) break;
    __syncthreads();                         // this descent's tree stores (VL, bslot, nboards, board) precede the next one
  }
  int *const leaf_node = to_next ? t.leaf_node_nx : t.leaf_node;
  int *const leaf_slot = to_next ? t.leaf_slot_nx : t.leaf_slot;
  if (lane_id() == 0)
    for (; k < K; ++k) { leaf_node[k * G + g] = -1; leaf_slot[k * G + g] = -1; }
}

template <bool FPU, bool SOLVE, bool FORCE>
__global__ void __launch_bounds__(64) k_select(DevCfg c, Tree t, int G, double Cpuct, const double *logtab) {
  __shared__ WaveLds s;
  const int g = blockIdx.x;
  if (g >= G) return;
  select_game<OneLeaf, FPU, SOLVE, FORCE>(s, c, t, g, Cpuct, logtab, false, ONE_LEAF);
}

template <bool FPU, bool SOLVE, bool FORCE>
__global__ void __launch_bounds__(64) k_select_multi(DevCfg c, Tree t, int G, int K, double Cpuct, const double *logtab, LeafPar lp) {
  __shared__ WaveLds s;
  const int g = blockIdx.x;
  if (g >= G) return;
  select_game_multi<FPU, SOLVE, FORCE>(s, c, t, G, g, K, Cpuct, logtab, false, lp);
}

// pending-visit counters of the roots (node storage, and with it VL, is reused across searches; children are zeroed
// where they are created)
__global__ void __launch_bounds__(64) k_vl_roots(int *VL, int node_cap, int G) {
  const int g = blockIdx.x * 64 + lane_id();
  if (g < G) VL[(size_t)g * node_cap] = 0;
}

// ================================================================================================
// k_live_rows (fpc_search_set_live_rows, opt-in): the live rows of the pending selection numbered densely in ascending
// row order, so that everything between selection and expansion works on n_live rows instead of `rows`.
//   live_row[j] = r, inv[r] = j for the j-th live row r (leaf_node[r] >= 0); inv[r] = -1 for a dead row;
//   c_slot[j] = the GLOBAL board-pool index of row r's leaf state, c_turn[j] = its side to move: what the encoders read
//   with board stride 0; c_slot[j] = -1, c_turn[j] = 0 for n_live <= j < rows (the tower's and k_encode's dead rows);
//   *n_live = the count.
// slot_stride: 0 when leaf_slot already holds the global index (a leaf-parallel selection), else board_cap (a one-leaf
// selection stores the slot within game r % G's pool).
// ONE block of LIVE_THREADS, chunks of LIVE_THREADS rows: every wave ballots its 64 rows, a lane's place is the popcount
// of the lower lanes + the lower waves' counts of the chunk (LDS) + the offset carried over from the chunks before.  No
// atomics: the numbering is a function of leaf_node alone.
// ================================================================================================
constexpr int LIVE_THREADS = 256;
__global__ void __launch_bounds__(LIVE_THREADS) k_live_rows(const int *leaf_node, const int *leaf_slot, const int *leaf_turn, int rows,
                                                            int G, int slot_stride, int *live_row, int *inv, int *c_slot, int *c_turn,
                                                            int *n_live) {
  __shared__ int wcount[2][LIVE_THREADS / 64];      // per chunk parity: one barrier per chunk is enough
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  int carried = 0;
  for (int base = 0, par = 0; base < rows; base += LIVE_THREADS, par ^= 1) {
    const int r = base + tid;
    const bool in = r < rows;
    const int node = in ? leaf_node[r] : -1;
    const int slot = in ? leaf_slot[r] : -1;
    const int turn = in ? leaf_turn[r] : 0;
    const bool live = node >= 0;
    const unsigned long long bal = __ballot(live);
    if (lane == 0) wcount[par][wave] = __popcll(bal);
    __syncthreads();
    int below = 0, total = 0;
    for (int w = 0; w < LIVE_THREADS / 64; ++w) {
      const int cw = wcount[par][w];
      below += w < wave ? cw : 0;
      total += cw;
    }
    if (live) {
      const int j = carried + below + __popcll(bal & ((1ull << lane) - 1ull));
      live_row[j] = r;
      inv[r] = j;
      c_slot[j] = (r % G) * slot_stride + slot;
      c_turn[j] = turn;
    } else if (in) {
      inv[r] = -1;
    }
    carried += total;
  }
  for (int j = carried + tid; j < rows; j += LIVE_THREADS) { c_slot[j] = -1; c_turn[j] = 0; }
  if (tid == 0) *n_live = carried;
}

// ================================================================================================
// deterministic f32 exp shared (as a numeric SPEC, DESIGN.md "fpc_expf") with the test oracle:
// k = rint(x*log2e); r = x - k*ln2 (two fma steps); degree-7 Horner in fma; scale by 2^k.
// ================================================================================================
__device__ __forceinline__ float fpc_expf(float x) {
  if (x != x) return x;
  if (x < -86.0f) return 0.0f;
  if (x > 88.0f) return __builtin_inff();
  const float k = __builtin_rintf(x * 0x1.715476p+0f);
  float r = __builtin_fmaf(k, -0x1.62e4p-1f, x);
  r = __builtin_fmaf(k, -0x1.7f7d1cp-20f, r);
  float p = 0x1.a01a02p-13f;
  p = __builtin_fmaf(p, r, 0x1.6c16c2p-10f);
  p = __builtin_fmaf(p, r, 0x1.111112p-7f);
  p = __builtin_fmaf(p, r, 0x1.555556p-5f);
  p = __builtin_fmaf(p, r, 0x1.555556p-3f);
  p = __builtin_fmaf(p, r, 0.5f);
  p = __builtin_fmaf(p, r, 1.0f);
  p = __builtin_fmaf(p, r, 1.0f);
  const int ki = (int)k;
  const uint32_t bits = (uint32_t)(ki + 127) << 23;
  float sc;
  __builtin_memcpy(&sc, &bits, 4);
  return p * sc;
}

__device__ __forceinline__ float fdiv_rn(float a, float b) {
#ifdef FPC_EMUL
  return a / b;
#else
  return __fdiv_rn(a, b);
#endif
}

// Shared end of both expand kernels (one wave): s.pri[0..nl) = unnormalised legal probabilities in
// ascending flat order, s.lsorted the flat indices.  Legal mass (sequential ascending f32 sum),
// policy error, BackpropagateNodes (mcts.py:78) before ExpandNodes (mcts.py:79), children appended.
// Where the network left a step row's outputs (value, softmax records, logits): at the row itself, or, under the
// live-row numbering (t.inv, k_live_rows), at inv[row] -- one dependent load, requested with the up-front batch, on which
// only the addresses of those outputs wait.  A dead row gets -1 there and must not use it as an index.
__device__ __forceinline__ int live_net_row(const Tree &t, int row) { return t.inv != nullptr ? t.inv[row] : row; }
struct ExpandPre {     // what expand_game / expand_legal_game fetch up front for expand_finish (one round trip with their own loads)
  float v;             // value[g]
  int path_len, path_node, nnodes;
};
// crow: the row of the network's outputs that holds this leaf (live_net_row; < 0: a dead row under the live-row numbering)
__device__ __forceinline__ ExpandPre expand_prefetch(const Tree &t, int g, int row, int crow, const float *value) {
  ExpandPre e;
  const int lane = lane_id();
  e.v = crow >= 0 ? value[crow] : 0.f;
  e.path_len = t.path_len[row];
  e.path_node = lane < t.path_cap ? t.path[(size_t)row * t.path_cap + lane] : 0;
  e.nnodes = t.nnodes[g];
  return e;
}
// MULTI (leaf-parallel): `row` is the leaf's row (k*G + g); the backup also takes the row's pending visit off its path
// (VL -= 1) and the new children start with VL = 0.  Returns false on a policy error.
template <bool MULTI>
__device__ __forceinline__ bool expand_finish(WaveLds &s, const Tree &t, int g, int row, size_t nb, int n, int nl, bool nan, const ExpandPre &pre,
                                              int *VL) {
  const int lane = lane_id();
  if (lane == 0) {
    float T = 0.f;
    for (int j = 0; j < nl; ++j) T = T + s.pri[j];
    s.errbits = (nan || !(T > 0.f)) ? ERR_POLICY : 0;
    s.scal_f = T;
  }
  __syncthreads();
  if (s.errbits) {                          // the reference would expand all A indices and throw
    if (lane == 0) { t.err[g] |= ERR_POLICY; t.alive[g] = 0; }
    return false;
  }
  const float T = s.scal_f;
  // root Dirichlet noise (N4): prior' = (1 - eps) prior + eps g_j / sum g over the root's legal moves,
  // g = caller-supplied Gamma(alpha) draws; sequential ascending f32 sum, IEEE division
  const bool noisy = n == 0 && t.noise != nullptr;
  if (noisy) {
    const float *gm = t.noise + (size_t)g * FPC_MAX_MOVES;
    __syncthreads();
    if (lane == 0) {
      float sg = 0.f;
      for (int j = 0; j < nl; ++j) sg = sg + gm[j];
      s.scal_f = sg;
    }
    __syncthreads();
  }
  const float SG = s.scal_f;
  const bool add_noise = noisy && SG > 0.f;      // rows without positive mass (never uploaded, all-zero draws) leave the priors alone
  // BackpropagateNodes (mcts.py:78) before ExpandNodes (mcts.py:79)
  backprop_path(t, nb, row, pre.v, pre.path_len, pre.path_node);
  if constexpr (MULTI) {
    const int *path = t.path + (size_t)row * t.path_cap;
    for (int k = lane; k < pre.path_len; k += 64) VL[nb + (k < 64 ? pre.path_node : path[k])] -= 1;
  }
  if (lane == 0) t.sims_done[g] += 1;
  // children: ascending flat order, entries with prior == 0 dropped (torch.nonzero, mcts.py:84)
  const int base_node = pre.nnodes;
  int created = 0;
  for (int b0 = 0; b0 < nl; b0 += 64) {
    const int j = b0 + lane;
    float pr = 0.f;
    bool nz = false;
    if (j < nl) {
      pr = fdiv_rn(s.pri[j], T);
      if (add_noise) pr = (1.0f - t.noise_eps) * pr + t.noise_eps * fdiv_rn(t.noise[(size_t)g * FPC_MAX_MOVES + j], SG);
      nz = pr != 0.f;
    }
    const unsigned long long bal = __ballot(nz);
    if (nz) {
      const int k = base_node + created + __popcll(bal & ((1ull << lane) - 1ull));
      if (k < t.node_cap) {
        t.N[nb + k] = t.born; t.W[nb + k] = 0.0; t.P[nb + k] = pr; t.mv[nb + k] = s.lsorted[j];
        t.parent[nb + k] = n; t.child0[nb + k] = -1; t.nch[nb + k] = 0; t.bslot[nb + k] = -1;
        if constexpr (MULTI) VL[nb + k] = 0;
      }
    }
    created += __popcll(bal);
  }
  if (lane == 0) {
    if (base_node + created > t.node_cap) { t.err[g] |= ERR_CAP_NODES; t.alive[g] = 0; }
    else if (created > 0) {
      t.child0[nb + n] = base_node; t.nch[nb + n] = (uint16_t)created; t.nnodes[g] = base_node + created;
    }
  }
  return true;
}

// ================================================================================================
// Softmax statistics of a logits row, by chunks of 1024 logits (= 256 threads x float4) -- the first half
// of the numeric spec of mcts.py:67.  Chunk c of a row: m_c = its maximum,
// s_c = sum of fpc_expf(x - m_c) in the order "thread t owns float4 group t of the chunk, adds x,y,z,w
// ascending; xor butterfly 32..1 inside each 64-lane wave; ((w0+w1)+w2)+w3", flag = a NaN was seen.
// The policy Linear's k_fc_reduce produces the records while it still holds the logits in registers
// (fpc_fc.h); k_softmax_partials produces the same records for logits handed in by an external evaluator.
// ================================================================================================
constexpr int SM_THREADS = 256;
constexpr int SM_REC = 4;              // floats per chunk record: max, sum, NaN flag, pad
constexpr int SM_MAXCH = 32;           // records per row (A <= 32768; 23 at 14x14)
// all SM_THREADS threads call; `red`: 8 floats of shared memory
__device__ __forceinline__ void softmax_chunk_stats(float4 v, bool valid, float *red, float *rec) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  float m = -__builtin_inff();
  bool nan = false;
  if (valid) {
    nan = (v.x != v.x) | (v.y != v.y) | (v.z != v.z) | (v.w != v.w);
    m = v.x > m ? v.x : m; m = v.y > m ? v.y : m; m = v.z > m ? v.z : m; m = v.w > m ? v.w : m;
  }
  for (int off = 32; off >= 1; off >>= 1) { const float o = __shfl_xor(m, off); m = o > m ? o : m; }
  const bool wnan = __ballot(nan) != 0ull;
  if (lane == 0) { red[wave] = m; red[4 + wave] = wnan ? 1.f : 0.f; }
  __syncthreads();
  m = red[0];
  m = red[1] > m ? red[1] : m; m = red[2] > m ? red[2] : m; m = red[3] > m ? red[3] : m;
  const float nf = ((red[4] != 0.f) | (red[5] != 0.f) | (red[6] != 0.f) | (red[7] != 0.f)) ? 1.f : 0.f;
  __syncthreads();
  float part = 0.f;
  if (valid && m > -__builtin_inff()) {
    part = part + fpc_expf(v.x - m);
    part = part + fpc_expf(v.y - m);
    part = part + fpc_expf(v.z - m);
    part = part + fpc_expf(v.w - m);
  }
  for (int off = 32; off >= 1; off >>= 1) part = part + __shfl_xor(part, off);
  if (lane == 0) red[wave] = part;
  __syncthreads();
  if (tid == 0) { rec[0] = m; rec[1] = ((red[0] + red[1]) + red[2]) + red[3]; rec[2] = nf; rec[3] = 0.f; }
}

// grid = G * nchunks blocks: block b -> (row b / nchunks, chunk b % nchunks)
__global__ void __launch_bounds__(SM_THREADS) k_softmax_partials(const float *logits, int A, int G, int nchunks, float *stats) {
  __shared__ float red[8];
  const int g = (int)blockIdx.x / nchunks, ch = (int)blockIdx.x % nchunks;
  if (g >= G) return;
  const int q = ch * SM_THREADS + (int)threadIdx.x;
  const bool valid = q * 4 < A;
  const float4 v = valid ? *reinterpret_cast<const float4 *>(logits + (size_t)g * A + 4 * q) : float4{0.f, 0.f, 0.f, 0.f};
  softmax_chunk_stats(v, valid, red, stats + ((size_t)g * SM_MAXCH + ch) * SM_REC);
}

// ================================================================================================
// k_expand: mcts.py:67-89 for one leaf per wave.
//   p = softmax(logits) over all A entries;  policy_abs[pl][r][c] = p[pl][rot90 by -turn0]  (Q6);
//   prior_j = p_src(j) / sum_legal p  for the ascending legal list; exact zeros get no child;
//   BackpropagateNodes(value) first (Q4), then children appended with N=1 (Q1), W=0.
// Numeric spec, second half: m = max_c m_c; S = sequential ascending sum over the
// chunks of s_c * fpc_expf(m_c - m) (a chunk of -inf only contributes 0); p_i = fpc_expf(l_i - m) * (1/S);
// the legal mass is a sequential ascending f32 sum.  The row itself is only touched at the legal moves.
// ================================================================================================
constexpr int EXPAND_THREADS = 64;
// Where a leaf's logits come from.  `dense` != null: a [G][A] f32 matrix (external evaluators; fpc_nn_forward).
// Else: the policy Linear's split-K partial sums as k_fc16 / k_fcw left them -- `part` [slab][Mtot][gw] f32 and the bias --
// which the fused search never combines into a dense matrix: the softmax records come from k_fc_reduce, and the
// expansion adds up the slabs of a column itself at the leaf's ~40 legal moves, in k_fc_reduce's order
// (bias, then the group's slabs ascending: the same f32 additions, the same bits).
constexpr int LOGIT_MAX_SLABS = 8;
struct LogitSrc {
  const float *dense;
  const float *part, *bias;
  int G1, s1, s2, Mtot;      // column groups [0, G1) own s1 slabs each, the rest s2 (plan_fc)
  int gw;                    // columns per group: 256 (k_fc / k_fc16) or 384 (k_fcw)
};
__device__ __forceinline__ float logit_at(const LogitSrc &L, int g, int A, int idx) {
  if (L.dense) return L.dense[(size_t)g * A + idx];
  const int j = L.gw == 256 ? idx >> 8 : idx / L.gw, col = idx - j * L.gw;   // column group (fpc_fc.h)
  const int base = j < L.G1 ? j * L.s1 : L.G1 * L.s1 + (j - L.G1) * L.s2, cnt = j < L.G1 ? L.s1 : L.s2;
  // all of a column's slabs are requested before the first is added (one round trip, not `cnt`): a group has at most
  // LOGIT_MAX_SLABS = 2 * FC_SPLITK of them (plan_fc)
  float p[LOGIT_MAX_SLABS];
#pragma unroll
  for (int k = 0; k < LOGIT_MAX_SLABS; ++k) p[k] = k < cnt ? L.part[((size_t)(base + k) * L.Mtot + g) * L.gw + col] : 0.f;
  float v = L.bias[idx];
#pragma unroll
  for (int k = 0; k < LOGIT_MAX_SLABS; ++k) v = k < cnt ? v + p[k] : v;
  return v;
}
// G: rows of the step (games when one leaf per game); g the game, row the leaf's row (== g unless MULTI)
template <bool MULTI>
__device__ inline bool expand_game(WaveLds &s, const DevCfg &c, const Tree &t, int G, int g, int row, const LogitSrc &logits,
                                   const float *stats, const float *value, int *VL) {
  const int lane = lane_id();
  const size_t nb = (size_t)g * t.node_cap;
  const int nchunks = (c.A / 4 + SM_THREADS - 1) / SM_THREADS;     // A = (8R+8)*R*R is a multiple of 4 for even R
  const uint16_t *legal = t.legal + (size_t)row * FPC_MAX_MOVES;
  // ONE round trip for everything whose address depends on no other load (a lone wave per CU pays the full memory
  // latency per dependent load): the leaf, its legal list (first 64 entries), the chunk records, the leaf turns of the
  // first 64 games (the batch's first live leaf is almost always among them), value / path / node count.
  const int crow = live_net_row(t, row);
  const int n = t.leaf_node[row];
  const int nl = t.nlegal[row];
  const int own_turn = t.leaf_turn[row];
  const int scan_node = lane < G ? t.leaf_node[lane] : -1;
  const int scan_turn = lane < G ? t.leaf_turn[lane] : 0;
  const int fl0 = legal[lane];                                    // lane < 64 <= FPC_MAX_MOVES: always in bounds
  float mc = -__builtin_inff(), sc = 0.f;
  bool nan = false;
  const float *st = stats + (size_t)(crow >= 0 ? crow : 0) * SM_MAXCH * SM_REC;
  if (lane < nchunks && crow >= 0) { mc = st[lane * SM_REC]; sc = st[lane * SM_REC + 1]; nan = st[lane * SM_REC + 2] != 0.f; }
  const ExpandPre pre = expand_prefetch(t, g, row, crow, value);
  int turn0;
  if (c.rules & FPC_RULES_ROTATION) turn0 = own_turn;
  else {                                                          // the batch's FIRST live leaf (Q6)
    const unsigned long long bal = __ballot(scan_node >= 0);
    turn0 = bal ? wave_read(scan_turn, (int)__ffsll((long long)bal) - 1) : (G > 64 ? first_leaf_turn(t.leaf_node, t.leaf_turn, G) : 0);
  }
  if (n < 0) return true;
  FPC_TS(1);
  float m = mc;
  for (int off = 32; off >= 1; off >>= 1) { const float o = __shfl_xor(m, off); m = o > m ? o : m; }
  nan = __ballot(nan) != 0ull;
  const float term = (lane < nchunks && mc > -__builtin_inff()) ? sc * fpc_expf(mc - m) : 0.f;
  float S = 0.f;
  for (int k = 0; k < nchunks; ++k) S = S + wave_read(term, k);      // sequential ascending sum (numeric spec); k is wave-uniform
  const float inv = fdiv_rn(1.0f, S);
  FPC_TS(2);
  for (int j = lane; j < nl; j += 64) {
    const int fl = j < 64 ? fl0 : (int)legal[j];
    const int plane = fl / c.RR, pos = fl % c.RR;
    const int src = plane * c.RR + rot90_src(c.R, -turn0, pos / c.R, pos % c.R);
    s.pri[j] = fpc_expf(logit_at(logits, crow, c.A, src) - m) * inv;
    s.lsorted[j] = (uint16_t)fl;
  }
  __syncthreads();
  FPC_TS(3);
  return expand_finish<MULTI>(s, t, g, row, nb, n, nl, nan, pre, VL);
}

__global__ void __launch_bounds__(EXPAND_THREADS) k_expand(DevCfg c, Tree t, int G, LogitSrc logits, const float *stats, const float *value) {
  __shared__ WaveLds s;
  const int g = blockIdx.x;
  if (g >= G) return;
  (void)expand_game<false>(s, c, t, G, g, g, logits, stats, value, nullptr);
}

// k_expand of simulation step s followed, for the same game, by k_select of step s+1 (one launch and one
// dependent-kernel gap less per step).  Other blocks may still be expanding step s when this block's
// selection publishes its leaf, and strict mode reads the turn of the batch's FIRST live leaf across games
// (Q6), so the selection writes the _nx leaf arrays; the host swaps them in after the launch.
template <bool FPU, bool SOLVE, bool FORCE>
__global__ void __launch_bounds__(EXPAND_THREADS) k_expand_select(DevCfg c, Tree t, int G, LogitSrc logits, const float *stats,
                                                                  const float *value, double Cpuct, const double *logtab) {
  __shared__ WaveLds s;
  const int g = blockIdx.x;
  if (g >= G) return;
  FPC_TS(0);
  (void)expand_game<false>(s, c, t, G, g, g, logits, stats, value, nullptr);
  __syncthreads();                           // the new children (global stores of other lanes) are visible to the descent
  FPC_TS(4);
  select_game<OneLeaf, FPU, SOLVE, FORCE>(s, c, t, g, Cpuct, logtab, true, ONE_LEAF);
}


// ================================================================================================
// k_expand_legal: the same step for the LEGAL-ONLY policy head (opt-in, fpc_set_policy_mode): the
// network evaluated the policy Linear only at the leaf's legal moves (k_policy_gemv, fpc_nn.h), so
// ll[g][j] is the logit of legal move j (ascending flat order, already taken through the inverse
// rotation).  prior_j = exp(l_j - max_legal) / sum_legal exp(l_k - max_legal): the full softmax's
// denominator cancels in mask-multiply + renormalise (mcts.py:67-76), so this equals the reference's
// priors up to f32 rounding -- except where a legal logit lies more than ~87 below the GLOBAL
// maximum, which the full softmax would flush to zero (child dropped / policy error) and this form
// cannot see.  One wave per game.
// ================================================================================================
template <bool MULTI>
__device__ inline bool expand_legal_game(WaveLds &s, const DevCfg &c, const Tree &t, int g, int row, const float *ll, const float *value, int *VL) {
  const int lane = lane_id();
  const int n = t.leaf_node[row];
  const ExpandPre pre = expand_prefetch(t, g, row, live_net_row(t, row), value);
  if (n < 0) return true;
  const size_t nb = (size_t)g * t.node_cap;
  const int nl = t.nlegal[row];
  const uint16_t *legal = t.legal + (size_t)row * FPC_MAX_MOVES;
  const float *lg = ll + (size_t)row * FPC_MAX_MOVES;
  float m = -__builtin_inff();
  bool nan = false;
  for (int j = lane; j < nl; j += 64) { const float v = lg[j]; nan |= v != v; m = v > m ? v : m; }
  for (int off = 32; off >= 1; off >>= 1) { const float o = __shfl_xor(m, off); m = o > m ? o : m; }
  nan = __ballot(nan) != 0ull;
  for (int j = lane; j < nl; j += 64) {
    s.pri[j] = m == -__builtin_inff() ? 0.f : fpc_expf(lg[j] - m);     // every legal logit -inf: mass 0 -> policy error
    s.lsorted[j] = legal[j];
  }
  __syncthreads();
  return expand_finish<MULTI>(s, t, g, row, nb, n, nl, nan, pre, VL);
}

__global__ void __launch_bounds__(64) k_expand_legal(DevCfg c, Tree t, int G, const float *ll, const float *value) {
  __shared__ WaveLds s;
  const int g = blockIdx.x;
  if (g >= G) return;
  (void)expand_legal_game<false>(s, c, t, g, g, ll, value, nullptr);
}

// the legal-only head's counterpart of k_expand_select
template <bool FPU, bool SOLVE, bool FORCE>
__global__ void __launch_bounds__(64) k_expand_legal_select(DevCfg c, Tree t, int G, const float *ll, const float *value, double Cpuct,
                                                            const double *logtab) {
  __shared__ WaveLds s;
  const int g = blockIdx.x;
  if (g >= G) return;
  (void)expand_legal_game<false>(s, c, t, g, g, ll, value, nullptr);
  __syncthreads();
  select_game<OneLeaf, FPU, SOLVE, FORCE>(s, c, t, g, Cpuct, logtab, true, ONE_LEAF);
}

// ================================================================================================
// Leaf-parallel search (fpc_search_set_leaves): the expansion of a step of `kexp` leaves per game, one block per game
// walking the game's live rows k*G + g in ascending k (that order fixes the f64 sums of the backups), each with the
// arithmetic of k_expand / k_expand_legal from ITS row's logits, statistics and value; the _select twins then select the
// next step's `ksel` leaves of the game (rows written to the _nx leaf arrays, as k_expand_select does).
// ================================================================================================
template <bool LEGAL>
__device__ inline void expand_game_multi(WaveLds &s, const DevCfg &c, const Tree &t, int G, int g, int kexp, const LogitSrc &logits,
                                         const float *ll, const float *stats, const float *value, int *VL) {
  for (int k = 0; k < kexp; ++k) {
    const int row = k * G + g;
    bool ok;
    if constexpr (LEGAL) ok = expand_legal_game<true>(s, c, t, g, row, ll, value, VL);
    else ok = expand_game<true>(s, c, t, kexp * G, g, row, logits, stats, value, VL);
    __syncthreads();                         // this row's tree stores (N, W, VL, children, nnodes) precede the next row
    if (!ok) break;                          // policy error: the game has left the search
  }
}

__global__ void __launch_bounds__(EXPAND_THREADS) k_expand_multi(DevCfg c, Tree t, int G, int kexp, LogitSrc logits, const float *stats,
                                                                 const float *value, LeafPar lp) {
  __shared__ WaveLds s;
  const int g = blockIdx.x;
  if (g >= G) return;
  expand_game_multi<false>(s, c, t, G, g, kexp, logits, nullptr, stats, value, lp.VL);
}

template <bool FPU, bool SOLVE, bool FORCE>
__global__ void __launch_bounds__(EXPAND_THREADS) k_expand_select_multi(DevCfg c, Tree t, int G, int kexp, int ksel, LogitSrc logits,
                                                                        const float *stats, const float *value, double Cpuct,
                                                                        const double *logtab, LeafPar lp) {
  __shared__ WaveLds s;
  const int g = blockIdx.x;
  if (g >= G) return;
  expand_game_multi<false>(s, c, t, G, g, kexp, logits, nullptr, stats, value, lp.VL);
  select_game_multi<FPU, SOLVE, FORCE>(s, c, t, G, g, ksel, Cpuct, logtab, true, lp);
}

__global__ void __launch_bounds__(64) k_expand_legal_multi(DevCfg c, Tree t, int G, int kexp, const float *ll, const float *value, LeafPar lp) {
  __shared__ WaveLds s;
  const int g = blockIdx.x;
  if (g >= G) return;
  expand_game_multi<true>(s, c, t, G, g, kexp, LogitSrc{}, ll, nullptr, value, lp.VL);
}

template <bool FPU, bool SOLVE, bool FORCE>
__global__ void __launch_bounds__(64) k_expand_legal_select_multi(DevCfg c, Tree t, int G, int kexp, int ksel, const float *ll,
                                                                  const float *value, double Cpuct, const double *logtab, LeafPar lp) {
  __shared__ WaveLds s;
  const int g = blockIdx.x;
  if (g >= G) return;
  expand_game_multi<true>(s, c, t, G, g, kexp, LogitSrc{}, ll, nullptr, value, lp.VL);
  select_game_multi<FPU, SOLVE, FORCE>(s, c, t, G, g, ksel, Cpuct, logtab, true, lp);
}

// ================================================================================================
// k_tree_advance (fpc_search_advance, opt-in subtree reuse; not reference semantics -- the reference builds a fresh
// tree per ply): new game g continues old game src_game[g] from the root child whose move is flat[g].  That child
// becomes node 0 (parent -1, move 0xffff, N / W kept), its subtree follows with N, W, P, move, the children's order
// and every materialised board; the rest of the old tree is dropped.
//
// OUT OF PLACE: games move to other indices -- lower ones when games are dropped, and, since fpc_search_advance_refill
// puts fresh rows between the kept ones, higher ones as well -- and the blocks run concurrently, so block g would
// overwrite a region that another block is still reading.  `t` is the finished search (read only, apart from the
// per-game scalars, which no block reads), `o` the same Tree with the eight node arrays and the board pool replaced by
// the second set; the host swaps the two sets after the launch.  Neither direction matters to the scheme: block g reads
// only region src_game[g] of `t` and writes only region g of `o` and the scalars of game g.
//
// FRESH ROWS (fpc_search_advance_refill): src_game[g] == -1 starts a new game in region g on fresh[g], in the state
// k_search_init leaves a game in (N = 1 -- 0 under FPC_RULES_VISITS, as everywhere a node is born --, W = 0, no children, board slot 0 = fresh[g], one node, one board, alive, no
// error, no leaf, no pending visit), kept[g] = that N, roots_out[g] = fresh[g]; flat[g] is not read.  A block is one wave
// and src_game[g] is the same in all of its lanes, so the two kinds of row never meet at a barrier: the fresh kind
// returns before the first __syncthreads, as a block with g >= G does.  Root noise reaches such a root when it is
// expanded (n == 0), from row g of the noise.
//
// Breadth-first append, one wave per game: new node j keeps its OLD (child0, nch) until it is processed.  64 queue
// entries at a time: a wave scan of their child counts places every entry's child block at the tail (blocks stay
// contiguous, children keep their order); the blocks are then copied as ONE flat range, 64 nodes per pass with
// coalesced stores, each lane finding its queue entry by bisection of the scanned offsets; the materialised nodes of a
// pass get consecutive new board slots (ballot prefix) and their 288-byte states are copied as one flat range of
// dwords.  No mark array, no atomics, and the node order is a function of the old tree alone.
// The new root's state is board slot 0: the child's board, or -- a child that was never selected (Q1: every child has
// N = 1, so a sampled move can be one; under FPC_RULES_VISITS it has N = 0 and the game is a fresh root's) -- the old root's board with the move made, which is what a selection would
// have done, and no more (no GetGameResult / legal-moves pass).
// Proof statuses (fpc_search_set_solver; t.S null: none): every node that moves takes its status along, into the second
// set's array, which the host zeroed before the launch -- so fresh rows, the root of a failed advance and every node created
// later are unknown.
// Root noise: a new root that is already expanded gets it here, child i (ascending flat order) from gamma[g][i], with
// expand_finish's operations in expand_finish's order; an unexpanded one gets it when it is expanded (n == 0).
// ================================================================================================
__global__ void __launch_bounds__(64) k_tree_advance(DevCfg c, Tree t, Tree o, int G, const int *src_game, const int *flat,
                                                     const fpc_board *fresh, int *VL, int *kept, fpc_board *roots_out) {
  __shared__ WaveLds s;
  __shared__ int q_c0[64], q_ex[64], q_bs[64];
  const int g = blockIdx.x;
  if (g >= G) return;
  const int lane = lane_id();
  const int born = t.born;
  const int sg = src_game ? src_game[g] : g;
  const size_t nb = (size_t)g * t.node_cap;
  fpc_board *npool = o.boards + (size_t)g * t.board_cap;
  if (sg < 0) {                                              // a fresh row (block-uniform): k_search_init's state, no barrier
    const uint32_t *src = reinterpret_cast<const uint32_t *>(&fresh[g]);
    uint32_t *dst = reinterpret_cast<uint32_t *>(&npool[0]), *out = reinterpret_cast<uint32_t *>(&roots_out[g]);
    const uint32_t w0 = src[lane], w1 = lane < 8 ? src[64 + lane] : 0u;
    dst[lane] = w0; out[lane] = w0;
    if (lane < 8) { dst[64 + lane] = w1; out[64 + lane] = w1; }
    if (lane == 0) {
      o.N[nb] = born; o.W[nb] = 0.0; o.P[nb] = 0.f; o.mv[nb] = 0xffff; o.parent[nb] = -1; o.child0[nb] = -1; o.nch[nb] = 0;
      o.bslot[nb] = 0;
      if (VL != nullptr) VL[nb] = 0;
      t.nnodes[g] = 1; t.nboards[g] = 1; t.alive[g] = 1; t.sims_done[g] = 0; t.err[g] = 0;
      t.leaf_node[g] = -1; t.leaf_slot[g] = -1; t.leaf_turn[g] = 0; t.nlegal[g] = 0;
      kept[g] = born;
    }
    return;
  }
  const int fl = flat[g];
  const size_t ob = (size_t)sg * t.node_cap;
  const fpc_board *opool = t.boards + (size_t)sg * t.board_cap;
  // ---- the root child that was played
  const int rc0 = t.child0[ob], rnc = rc0 < 0 ? 0 : (int)t.nch[ob];
  int r = -1;
  for (int base = 0; base < rnc && r < 0; base += 64) {
    const int i = base + lane;
    const unsigned long long hit = __ballot(i < rnc && (int)t.mv[ob + rc0 + i] == fl);
    if (hit) r = rc0 + base + (int)__ffsll((long long)hit) - 1;
  }
  int errbits = r < 0 ? ERR_MOVE : 0;      // not a root child: the game is killed with a childless root on the old root's state
  const int rslot = r < 0 ? 0 : t.bslot[ob + r], rootN = r < 0 ? born : t.N[ob + r];
  if (lane == 0) {
    o.N[nb] = rootN; o.W[nb] = r < 0 ? 0.0 : t.W[ob + r]; o.P[nb] = r < 0 ? 0.f : t.P[ob + r]; o.mv[nb] = 0xffff; o.parent[nb] = -1;
    o.child0[nb] = r < 0 ? -1 : t.child0[ob + r]; o.nch[nb] = r < 0 ? (uint16_t)0 : t.nch[ob + r]; o.bslot[nb] = 0;
    if (t.S != nullptr && r >= 0) o.S[nb] = t.S[ob + r];      // (the host zeroed o.S: a failed advance's root and a fresh row stay 0)
  }
  // ---- its state -> board slot 0 (the root of a tree is always in slot 0)
  if (rslot < 0) {
    lds_load_board(&s, &opool[0]);
    int from;
    const int to = flat_to(c, fl, &from);
    if (!make_move_wave<2>(&s.b, from, to, c)) errbits |= ERR_MOVE;
    lds_store_board(&s, &npool[0]);
  } else {
    const uint32_t *src = reinterpret_cast<const uint32_t *>(&opool[rslot]);
    uint32_t *dst = reinterpret_cast<uint32_t *>(&npool[0]);
    dst[lane] = src[lane];
    if (lane < 8) dst[64 + lane] = src[64 + lane];
  }
  __syncthreads();
  // ---- breadth-first append of the subtree
  int tail = 1, nbo = 1;
  for (int head = 0, end = 1; head < tail && !(errbits & (ERR_CAP_NODES | ERR_CAP_BOARDS)); head = end) {
    end = head + 64 < tail ? head + 64 : tail;              // this batch: queue entries head .. end-1
    const int j = head + lane;
    int oc0 = -1, cnt = 0;
    if (j < end) { oc0 = o.child0[nb + j]; cnt = oc0 < 0 ? 0 : (int)o.nch[nb + j]; }
    int inc = cnt;                                          // inclusive scan of the child counts
    for (int d = 1; d < 64; d <<= 1) {
      const int v = __shfl_up(inc, d);
      if (lane >= d) inc += v;
    }
    const int total = wave_read(inc, 63), ex = inc - cnt;
    if (tail + total > t.node_cap) { errbits |= ERR_CAP_NODES; break; }     // cannot happen: a subtree of a tree that fitted
    if (oc0 >= 0) o.child0[nb + j] = tail + ex;
    q_c0[lane] = oc0; q_ex[lane] = ex;                      // lanes past the batch: ex == total, never found
    __syncthreads();
    for (int p0 = 0; p0 < total; p0 += 64) {
      const int p = p0 + lane;
      const bool in = p < total;
      int bs = -1;
      size_t dn = 0;
      if (in) {
        int en = 0;                                         // the last entry with ex <= p: the one whose block holds p
        for (int step = 32; step; step >>= 1) if (q_ex[en + step] <= p) en += step;
        const size_t so = ob + q_c0[en] + (p - q_ex[en]);
        dn = nb + tail + p;
        o.N[dn] = t.N[so]; o.W[dn] = t.W[so]; o.P[dn] = t.P[so]; o.mv[dn] = t.mv[so]; o.parent[dn] = head + en;
        o.child0[dn] = t.child0[so]; o.nch[dn] = t.nch[so];
        if (t.S != nullptr) o.S[dn] = t.S[so];
        bs = t.bslot[so];
      }
      const unsigned long long mat = __ballot(bs >= 0);
      const int m = __popcll(mat), mi = __popcll(mat & ((1ull << lane) - 1ull));
      if (nbo + m > t.board_cap) { errbits |= ERR_CAP_BOARDS; break; }      // cannot happen either
      if (in) o.bslot[dn] = bs >= 0 ? nbo + mi : -1;
      if (m) {                                              // wave-uniform
        if (bs >= 0) q_bs[mi] = bs;
        __syncthreads();
        for (int q = lane; q < m * 72; q += 64) {           // 72 dwords per state
          const int bi = q / 72, w = q - bi * 72;
          reinterpret_cast<uint32_t *>(&npool[nbo + bi])[w] = reinterpret_cast<const uint32_t *>(&opool[q_bs[bi]])[w];
        }
        nbo += m;
        __syncthreads();
      }
    }
    tail += total;
    __syncthreads();                                        // this batch's stores precede the next batch's loads; q_* are reused
  }
  if (errbits & (ERR_CAP_NODES | ERR_CAP_BOARDS)) {         // leave a childless root rather than a half-built tree
    __syncthreads();
    if (lane == 0) { o.child0[nb] = -1; o.nch[nb] = 0; if (t.S != nullptr) o.S[nb] = FPC_PROOF_UNKNOWN; }
    tail = 1; nbo = 1;
    __syncthreads();
  }
  // ---- root noise on an expanded new root (its children are nodes 1 .. nch)
  const int nc = o.child0[nb] < 0 ? 0 : (int)o.nch[nb];
  if (t.noise != nullptr && nc > 0 && !errbits) {
    const float *gm = t.noise + (size_t)g * FPC_MAX_MOVES;
    const int nn = nc < FPC_MAX_MOVES ? nc : FPC_MAX_MOVES;
    if (lane == 0) {
      float sgm = 0.f;
      for (int k = 0; k < nn; ++k) sgm = sgm + gm[k];
      s.scal_f = sgm;
    }
    __syncthreads();
    const float SG = s.scal_f;
    if (SG > 0.f)
      for (int k = lane; k < nn; k += 64) o.P[nb + 1 + k] = (1.0f - t.noise_eps) * o.P[nb + 1 + k] + t.noise_eps * fdiv_rn(gm[k], SG);
  }
  if (VL != nullptr)                                         // no pending visit survives from the game that lived in this region
    for (int k = lane; k < tail; k += 64) VL[nb + k] = 0;
  {
    const uint32_t *src = reinterpret_cast<const uint32_t *>(&npool[0]);
    uint32_t *dst = reinterpret_cast<uint32_t *>(&roots_out[g]);
    dst[lane] = src[lane];
    if (lane < 8) dst[64 + lane] = src[64 + lane];
  }
  if (lane == 0) {
    t.nnodes[g] = tail; t.nboards[g] = nbo; t.alive[g] = errbits ? 0 : 1; t.sims_done[g] = 0; t.err[g] = errbits;
    t.leaf_node[g] = -1; t.leaf_slot[g] = -1; t.leaf_turn[g] = 0; t.nlegal[g] = 0;
    kept[g] = rootN;
  }
}

}  // namespace fpc
