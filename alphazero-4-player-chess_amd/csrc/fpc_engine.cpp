// fpc_engine.cpp -- host side of the C-ABI declared in include/fpc_engine.h.
//
// Owns every device allocation (tree SoA pools, board pools, staging), launches the kernels of
// fpc_tree_kernels.h / fpc_nn_kernels.h on one HIP stream, and never computes game logic on the
// host: positions are uploaded, processed by one wavefront each, and read back.  Compiled by hipcc
// for gfx950 into libfpc_engine.so (the product).  The same file builds against the wavefront
// emulator (-DFPC_EMUL, tests/emul/) for the CPU test-suite; that build has no NN and is never
// loaded by the product modules.
#include "fpc_tree_kernels.h"
#include "fpc_pack.h"

#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <string>
#include <unordered_map>
#include <vector>

#ifndef FPC_EMUL
#include <dlfcn.h>

#include "fpc_nn.h"
#endif

using namespace fpc;

namespace {
std::string g_create_error;

struct Timer {
  hipEvent_t a = nullptr, b = nullptr;
};
}  // namespace

struct fpc_engine {
  fpc_config cfg{};
  DevCfg dc{};
  std::string err;
  hipStream_t stream = nullptr;
  // ---- batched board-op scratch
  int cap_boards = 0;
  fpc_board *d_boards = nullptr, *d_boards2 = nullptr;
  fpc_move *d_moves = nullptr;
  int *d_counts = nullptr, *d_results = nullptr, *d_err = nullptr, *d_player = nullptr, *d_flat = nullptr;
  float *d_dense = nullptr;       // encode / mask output staging [cap_boards * max(24*RR, A)]
  // ---- search
  Tree t{};
  std::vector<void *> allocs;
  int G = 0;
  double Cpuct = 0;
  bool searching = false;
  double *d_logtab = nullptr;
  float *d_enc_f32 = nullptr;     // [max_games,24,R,R]
  float *d_stats = nullptr;       // [max_games][SM_MAXCH][SM_REC] softmax chunk statistics of external logits
  fpc_board *d_roots = nullptr;   // staging [max_games]
  int *d_rc_i = nullptr;          // root-children gather: [2][rc_cap] flat | visits
  float *d_rc_f = nullptr;
  double *d_rc_d = nullptr;
  int *d_rc_meta = nullptr;       // [max_games][3]
  size_t rc_cap = 0;
  long sims_issued = 0;           // simulation steps since fpc_search_begin (bounded by max_sims: pools + log table)
  // ---- leaf-parallel search (fpc_search_set_leaves)
  int leaves = 1;                 // leaves per game of the NEXT selection
  double vl = 1.0;                // virtual loss per pending visit
  int *d_VL = nullptr;            // [max_games][node_cap] pending visits, allocated on the first leaves > 1
  bool stepping = false;          // between fpc_search_begin and fpc_search_results
  bool multi = false;             // this search runs the leaf-parallel kernels (leaves > 1 at begin, or set during it)
  int rows_k = 1;                 // leaves per game of the selection waiting to be expanded (rows = rows_k * G)
  bool pending_vl = false;        // that selection was made by a leaf-parallel kernel: its paths hold pending visits
  // ---- subtree reuse (fpc_search_advance)
  Tree t2{};                      // the second set of node arrays + board pool (only those nine members): k_tree_advance writes
                                  // the re-rooted trees there and the host swaps the two sets; allocated on the first advance
  int *d_adv = nullptr;           // [2][max_games] src_game | flat of one advance
  fpc_board *d_fresh = nullptr;   // [max_games] start boards of the rows fpc_search_advance_refill refills
  std::vector<fpc_board> fresh_stage;  // their host staging (the entries at kept positions are not read from the caller)
  // ---- per-game simulation budgets (fpc_search_set_budget)
  int *d_budget = nullptr;        // [max_games], allocated on the first call; t.budget points here while budgets are set
  // ---- playout cap randomization (fpc_search_set_fast_rows)
  uint8_t *d_fast = nullptr;      // [max_games] padded to whole words, allocated on the first call; t.fast points here while a mask is set
  std::vector<int> base;          // [G] simulations already through each root: kept_visits - born_visits after an advance, else 0
  bool selected = false;          // a selection has been issued since the last begin / advance
  // ---- live-row numbering (fpc_search_set_live_rows)
  bool live_rows = false;         // the setting; every selection latches it into t.inv (number_live_rows)
  int *d_live = nullptr;          // [4][max_games] live_row | inv | c_slot | c_turn, then n_live; allocated when first switched on
  int live_n = 0;                 // step entry points: the live rows of the pending selection
  // ---- MCTS solver (fpc_search_set_solver)
  bool solver = false;            // the switch; t.S / t2.S (one status byte per node) exist from the first on = 1 and are kept up
                                  // from then on whatever the switch says: cleared by begin, carried by an advance
  uint8_t *d_proof = nullptr;     // fpc_search_proofs' staging: [G] roots | [G][max_children] children
  size_t proof_cap = 0;
  // ---- forced playouts and target pruning (fpc_search_set_forced): the factor is t.forced
  int *d_target = nullptr;        // fpc_search_targets' staging: [G][max_children]
  size_t target_cap = 0;
  // ---- device-side move choice (fpc_search_play); allocated on the first call
  double *d_powtab = nullptr;     // [max_sims + 16] pow(v, 1 / powtab_T) by the host libm
  double powtab_T = -1.0;         // temperature the uploaded table was made for (-1: none yet)
  double *d_play_u = nullptr;     // [max_games] uniforms of one call
  int *d_play_out = nullptr;      // [3][max_games] flat | result | error bits of one call
  fpc_board *d_play_next = nullptr;   // [max_games] next states of one call
  hipEvent_t play_ev[2] = {nullptr, nullptr};   // around k_play_ply while fpc_set_timing is on
  float play_ms = -1.f;
  // ---- training tuples (device resident until the episode ends) and their RCCL exchange
  fpc_tuple *d_tuples = nullptr;
  int tuple_cap = 0, tuple_count = 0;
  int *d_tgame = nullptr;           // [max_games] game ids of one collect / set_z call
  float *d_tz = nullptr;            // [2][max_games]
  float *d_noise = nullptr;         // [max_games][FPC_MAX_MOVES] root-noise gamma draws (N4)
  int noise_n = 0;                  // rows uploaded by fpc_search_set_root_noise: a search must have exactly that many games
  void *comm = nullptr;             // ncclComm_t
  int comm_rank = 0, comm_world = 1;
  fpc_tuple *d_gather = nullptr;    // [world][gather_stride]
  long long *d_gcounts = nullptr;   // [3 * world + 4]: all-gathered (count, capacity, epoch) records | this rank's own record | its status word
  long long comm_epoch = 0;         // exchanges started on this communicator (tags every record and status word)
  int comm_fault = 0;               // fpc_debug_comm_fault
  int gcounts_world = 0;
  int gather_stride = 0;
  size_t gather_cap = 0;            // tuples the receive buffer holds (world x padded count)
  std::vector<int> gather_counts;
  // ---- device-resident replay (fpc_replay_*): the cursors live here, the records on the device
  struct Ring {
    fpc_tuple *d = nullptr;
    int cap = 0, size = 0, next = 0;   // ReplayBuffer's capacity, len(_items), _next
  } ring[FPC_REPLAY_RINGS + 1];     // + FPC_REPLAY_SCRATCH
  int *d_rp_idx = nullptr;          // index staging of one push ([2][rp_idx_cap / 2] source | destination) or one batch (slots)
  size_t rp_idx_cap = 0;
  hipEvent_t rp_ev[2] = {nullptr, nullptr};   // around k_replay_decode while fpc_set_timing is on
  float rp_decode_ms = -1.f;
  // ---- device-side weight pack (fpc_weights_pack / fpc_load_weights_device)
  unsigned char *d_pack_tab = nullptr;   // k_pack_conv's descriptor table [pack_tab_convs] + one float (the value bias on its way to the host)
  int pack_tab_convs = 0;
  hipEvent_t pk_ev[2] = {nullptr, nullptr};   // around the pack kernels while fpc_set_timing is on
  float pack_ms = -1.f;
  int fc_wtype = FPC_FC_W16;             // fpc_set_fc_weight_type: the policy Linear's weight type of the next pack
  float *d_fc8_scale = nullptr;          // k_fc_rowmax's output: [fc8_scale_n] scales + one int (the non-finite flag)
  int fc8_scale_n = 0;
  // ---- stats
  bool timing = false;
  int policy_mode = 0;            // FPC_POLICY_FULL / FPC_POLICY_LEGAL (fpc_search_run only)
  fpc_stats stats{};
  // asynchronous stage timing: events are only RECORDED on the stream during the search and read
  // back in fpc_search_results, so enabling it does not serialise the pipeline.  Five events per
  // simulation step still cost 2.7 % of the step, so only every TIMING_PERIOD-th step carries them
  // and its intervals are scaled by the period.
  static constexpr int TIMING_PERIOD = 16;   // round 3: at 8 the events still cost 0.3-1.3 % of the step (same-box A/B against --no-stage-timing)
  uint64_t tstep = 0;
  bool tsample = false;
  std::vector<hipEvent_t> evpool;
  std::vector<int> evtag;          // 0 step start, 1 tower start, 2 Linear start, 3 expand start, 4 step end
  size_t evused = 0;
#ifndef FPC_EMUL
  fpc::NN nn;
#endif
};

namespace {

int fail(fpc_engine *e, int code, const char *fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof(buf), fmt, ap);
  va_end(ap);
  if (e) e->err = buf; else g_create_error = buf;
  return code;
}

// every entry point re-selects the handle's device: one process may hold engines on several GPUs
#define USE_DEV(e)                                                                             \
  do {                                                                                         \
    if ((e) && hipSetDevice((e)->cfg.device) != hipSuccess) return fail(e, FPC_ENODEVICE, "hipSetDevice(%d) failed", (e)->cfg.device); \
  } while (0)

#define HIPCHK(e, call)                                                                        \
  do {                                                                                         \
    hipError_t _r = (call);                                                                    \
    if (_r != hipSuccess) return fail(e, FPC_ENODEVICE, "%s failed: %s", #call, hipGetErrorString(_r)); \
  } while (0)

template <class T>
int dalloc(fpc_engine *e, T **p, size_t count) {
  void *q = nullptr;
  if (hipMalloc(&q, count * sizeof(T)) != hipSuccess || !q) return fail(e, FPC_ENOMEM, "hipMalloc of %zu bytes failed", count * sizeof(T));
  if (hipMemset(q, 0, count * sizeof(T)) != hipSuccess) return fail(e, FPC_ENODEVICE, "hipMemset failed");
  e->allocs.push_back(q);
  *p = (T *)q;
  return 0;
}

int ensure_board_scratch(fpc_engine *e, int n) {
  if (n <= e->cap_boards) return 0;
  int cap = std::max(n, std::max(64, e->cap_boards * 2));
  auto re = [&](auto **p, size_t count) -> int {
    if (*p) { (void)hipFree(*p); e->allocs.erase(std::find(e->allocs.begin(), e->allocs.end(), (void *)*p)); *p = nullptr; }
    return dalloc(e, p, count);
  };
  int r;
  if ((r = re(&e->d_boards, cap))) return r;
  if ((r = re(&e->d_boards2, cap))) return r;
  if ((r = re(&e->d_moves, (size_t)cap * FPC_MAX_MOVES))) return r;
  if ((r = re(&e->d_counts, cap))) return r;
  if ((r = re(&e->d_results, cap))) return r;
  if ((r = re(&e->d_err, cap))) return r;
  if ((r = re(&e->d_player, cap))) return r;
  if ((r = re(&e->d_flat, cap))) return r;
  if ((r = re(&e->d_dense, (size_t)cap * std::max(24 * e->dc.RR, e->dc.A)))) return r;
  e->cap_boards = cap;
  return 0;
}

int check_boards(fpc_engine *e, const fpc_board *b, int n) {
  for (int i = 0; i < n; ++i) {
    for (int c = 0; c < 4; ++c) {
      if (b[i].castle[c] > 3) return fail(e, FPC_EINVAL, "board %d: bad castling rights", i);
      if (b[i].plen[c] > FPC_MAX_PL) return fail(e, FPC_EINVAL, "board %d: piece list longer than %d", i, FPC_MAX_PL);
    }
    if (b[i].turn > 3) return fail(e, FPC_EINVAL, "board %d: bad turn", i);
  }
  return 0;
}

int err_to_status(fpc_engine *e, const std::vector<int> &errs, const char *what) {
  for (size_t i = 0; i < errs.size(); ++i) {
    const int x = errs[i];
    if (!x) continue;
    if (x & ERR_MOVE) return fail(e, FPC_EMOVE, "%s %zu: piece missing for move (engine/board.cpp:1046-1054)", what, i);
    if (x & ERR_SELECT) return fail(e, FPC_ESELECT, "%s %zu: Failed to select a child. (node.cpp:72-75)", what, i);
    if (x & ERR_POLICY) return fail(e, FPC_EPOLICY, "%s %zu: legal policy mass is zero/NaN (reference expands every index and throws)", what, i);
    return fail(e, FPC_ECAPACITY, "%s %zu: capacity exceeded (bits %d: moves>%d / node pool / board pool)", what, i, x, FPC_MAX_MOVES);
  }
  return 0;
}

int run_board_ops(fpc_engine *e, fpc_board *boards, int n, int ops, const int *player, const int *flat) {
  int r;
  if ((r = ensure_board_scratch(e, n))) return r;
  HIPCHK(e, hipMemcpyAsync(e->d_boards, boards, (size_t)n * sizeof(fpc_board), hipMemcpyHostToDevice, e->stream));
  if (player) HIPCHK(e, hipMemcpyAsync(e->d_player, player, (size_t)n * sizeof(int), hipMemcpyHostToDevice, e->stream));
  if (flat) HIPCHK(e, hipMemcpyAsync(e->d_flat, flat, (size_t)n * sizeof(int), hipMemcpyHostToDevice, e->stream));
  FPC_LAUNCH(k_board_ops, n, 64, e->stream, e->dc, e->d_boards, n, ops, player ? e->d_player : (const int *)nullptr,
             flat ? e->d_flat : (const int *)nullptr, e->d_moves, e->d_counts, e->d_results, e->d_err);
  HIPCHK(e, hipGetLastError());
  return 0;
}

int fetch_errs(fpc_engine *e, int n, const char *what) {
  std::vector<int> errs(n);
  HIPCHK(e, hipMemcpyAsync(errs.data(), e->d_err, (size_t)n * sizeof(int), hipMemcpyDeviceToHost, e->stream));
  HIPCHK(e, hipStreamSynchronize(e->stream));
  return err_to_status(e, errs, what);
}

struct LocHash {   // std::hash<chess::BoardLocation>, engine/board.h:229-237
  int R;
  size_t operator()(uint8_t s) const {
    size_t h = 14479 + 14593 * (size_t)(int8_t)(s / R);
    h += 24439 * (size_t)(int8_t)(s % R);
    return h;
  }
};

void mark(fpc_engine *e, int tag) {
  if (tag == 0) e->tsample = e->timing && (e->tstep++ % fpc_engine::TIMING_PERIOD) == 0;
  if (!e->tsample) return;
  if (e->evused == e->evpool.size()) {
    hipEvent_t ev = nullptr;
    if (hipEventCreate(&ev) != hipSuccess) return;
    e->evpool.push_back(ev);
    e->evtag.push_back(0);
  }
  e->evtag[e->evused] = tag;
  (void)hipEventRecord(e->evpool[e->evused], e->stream);
  e->evused++;
}
// call after the stream has been synchronised
void resolve_marks(fpc_engine *e) {
  for (size_t i = 0; i + 1 < e->evused; ++i) {
    const int a = e->evtag[i], b = e->evtag[i + 1];
    if (b != a + 1) continue;
    float ms = 0.f;
    if (hipEventElapsedTime(&ms, e->evpool[i], e->evpool[i + 1]) != hipSuccess) continue;
    ms *= (float)fpc_engine::TIMING_PERIOD;
    if (a == 0) e->stats.ms_select += ms; else if (a == 1) e->stats.ms_tower += ms; else if (a == 2) e->stats.ms_fc += ms; else e->stats.ms_expand += ms;
  }
  e->evused = 0;
}

}  // namespace

extern "C" {

int fpc_abi_version(void) { return 7; }

const char *fpc_last_error(const fpc_engine *e) { return e ? e->err.c_str() : g_create_error.c_str(); }

int fpc_num_action_channels(int R) { return 8 * R + 8; }
int fpc_action_space_size(int R) { return (8 * R + 8) * R * R; }
int fpc_is_legal_location(int R, int INV, int row, int col) {
  const int mx = R - 1;
  if (row < 0 || row > mx || col < 0 || col > mx) return 0;
  const bool cc = col < INV || col > mx - INV;
  return !(cc && (row < INV || row > mx - INV));
}
int fpc_move_flat_index(int R, int from, int to) {
  if (from < 0 || to < 0 || from >= R * R || to >= R * R || from == to) return -1;
  const int dy = to / R - from / R, dx = to % R - from % R;
  const int ay = std::abs(dy), ax = std::abs(dx);
  const bool queen = dx == 0 || dy == 0 || ax == ay;
  const bool knight = (ax == 1 && ay == 2) || (ax == 2 && ay == 1);
  if (!queen && !knight) return -1;
  DevCfg c = make_devcfg(R, 0, 0);
  return move_plane(c, from, to) * R * R + from;
}
int fpc_flat_to_move(int R, int flat, int *from, int *to) {
  DevCfg c = make_devcfg(R, 0, 0);
  if (flat < 0 || flat >= c.A) return FPC_EINVAL;
  *to = flat_to(c, flat, from);
  return 0;
}

int fpc_board_from_dict(fpc_board *out, int R, int turn, const uint8_t *sq, const uint8_t *piece, int n,
                        const uint8_t *castle4) {
  if (!out || R < 4 || R * R > FPC_MAX_SQ || turn < 0 || turn > 3 || n < 0) return FPC_EINVAL;
  memset(out, 0, sizeof(*out));
  for (int c = 0; c < 4; ++c) out->king[c] = FPC_NO_SQ;
  out->turn = (uint8_t)turn;
  if (castle4) for (int c = 0; c < 4; ++c) out->castle[c] = castle4[c] & 3;
  // Same container, hash and insertion sequence as the reference constructor sees (pybind11's dict
  // -> unordered_map caster reserves, then emplaces in dict order), so iteration order -- which
  // the reference bakes into piece_list_ (engine/board.cpp:1209-1223) -- is reproduced.
  std::unordered_map<uint8_t, uint8_t, LocHash> m(0, LocHash{R});
  m.reserve((size_t)n);
  for (int i = 0; i < n; ++i) {
    if (sq[i] >= R * R || !(piece[i] & 0x80)) return FPC_EINVAL;
    m.emplace(sq[i], piece[i]);
  }
  std::vector<std::pair<uint8_t, uint8_t>> lists[4];
  for (const auto &it : m) {
    out->sq[it.first] = it.second;
    const int col = (it.second >> 5) & 3;
    lists[col].push_back({it.first, it.second});
    if (((it.second >> 2) & 7) == KING) out->king[col] = it.first;
  }
  static const int score[8] = {1, 2, 3, 4, 5, 0, 0, 0};   // piece_move_order_scores, engine/board.cpp:1230-1236
  for (int c = 0; c < 4; ++c) {
    std::sort(lists[c].begin(), lists[c].end(), [](const std::pair<uint8_t, uint8_t> &a, const std::pair<uint8_t, uint8_t> &b) {
      return score[(a.second >> 2) & 7] < score[(b.second >> 2) & 7];
    });
    if (lists[c].size() > FPC_MAX_PL) return FPC_ECAPACITY;
    out->plen[c] = (uint8_t)lists[c].size();
    for (size_t i = 0; i < lists[c].size(); ++i) out->pl[c][i] = lists[c][i].first;
  }
  return 0;
}

int fpc_board_heuristic(const fpc_board *b, int team) {   // engine/board.cpp:1263-1292
  static const int val[8] = {1, 3, 3, 5, 9, 0, 0, 0};
  int h = 0;
  for (int c = 0; c < 4; ++c)
    for (int i = 0; i < b->plen[c] && i < FPC_MAX_PL; ++i) {
      const uint8_t p = b->sq[b->pl[c][i]];
      if (!(p & 0x80)) continue;
      const int ty = (p >> 2) & 7;
      if (ty == KING) continue;
      h += (((p >> 5) & 1) == team) ? val[ty] : -val[ty];
    }
  return h;
}

int fpc_create(const fpc_config *cfg, fpc_engine **out) {
  if (!cfg || !out) return fail(nullptr, FPC_EINVAL, "null argument");
  const int R = cfg->board_size, INV = cfg->invalid_area;
  // geometries the kernels implement: 8 generator slots per piece bound the knight loop (2*2*(INV-1) <= 8,
  // engine/board.cpp:188) and the network kernels tile boards of 8..14 squares a side
  if (R < 8 || R > 14 || INV < 1 || INV > 3 || 2 * INV >= R) return fail(nullptr, FPC_EINVAL, "unsupported board %dx%d/%d (supported: 8..14 a side, cut corners 1..3)", R, R, INV);
  if (cfg->max_games < 1 || cfg->max_sims < 1) return fail(nullptr, FPC_EINVAL, "max_games/max_sims must be positive");
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= cfg->device || cfg->device < 0)
    return fail(nullptr, FPC_ENODEVICE, "no HIP device %d (found %d): this engine has no CPU path", cfg->device, ndev);
  if (hipSetDevice(cfg->device) != hipSuccess) return fail(nullptr, FPC_ENODEVICE, "hipSetDevice(%d) failed", cfg->device);
  fpc_engine *e = new fpc_engine();
  e->cfg = *cfg;
  if (e->cfg.avg_children <= 0) e->cfg.avg_children = 96;
  e->dc = make_devcfg(R, INV, FPC_RULES_STRICT);
  e->t.born = born_visits(FPC_RULES_STRICT);
  int r = 0;
  auto bail = [&](int code) { g_create_error = e->err; fpc_destroy(e); return code; };
  if (hipStreamCreate(&e->stream) != hipSuccess) { e->err = "hipStreamCreate failed"; return bail(FPC_ENODEVICE); }
  const int Gm = cfg->max_games;
  Tree &t = e->t;
  t.node_cap = 1 + cfg->max_sims * e->cfg.avg_children;
  t.board_cap = cfg->max_sims + 2;
  t.path_cap = cfg->max_sims + 2;          // a descent visits at most one node per earlier expansion + the root
  const size_t nn = (size_t)Gm * t.node_cap;
  if ((r = dalloc(e, &t.N, nn)) || (r = dalloc(e, &t.W, nn)) || (r = dalloc(e, &t.P, nn)) || (r = dalloc(e, &t.mv, nn)) ||
      (r = dalloc(e, &t.parent, nn)) || (r = dalloc(e, &t.child0, nn)) || (r = dalloc(e, &t.nch, nn)) ||
      (r = dalloc(e, &t.bslot, nn)) || (r = dalloc(e, &t.boards, (size_t)Gm * t.board_cap)) ||
      (r = dalloc(e, &t.nnodes, Gm)) || (r = dalloc(e, &t.nboards, Gm)) || (r = dalloc(e, &t.alive, Gm)) ||
      (r = dalloc(e, &t.sims_done, Gm)) || (r = dalloc(e, &t.err, Gm)) || (r = dalloc(e, &t.leaf_node, Gm)) || (r = dalloc(e, &t.leaf_node_nx, Gm)) ||
      (r = dalloc(e, &t.leaf_slot_nx, Gm)) || (r = dalloc(e, &t.leaf_turn_nx, Gm)) ||
      (r = dalloc(e, &t.leaf_turn, Gm)) || (r = dalloc(e, &t.nlegal, Gm)) ||
      (r = dalloc(e, &t.path, (size_t)Gm * t.path_cap)) || (r = dalloc(e, &t.path_len, Gm)) ||
      (r = dalloc(e, &t.legal, (size_t)Gm * FPC_MAX_MOVES)) || (r = dalloc(e, &t.leaf_slot, Gm)) ||
      (r = dalloc(e, &e->d_enc_f32, (size_t)Gm * 24 * e->dc.RR)) || (r = dalloc(e, &e->d_stats, (size_t)Gm * SM_MAXCH * SM_REC)) || (r = dalloc(e, &e->d_roots, Gm)) ||
      (r = dalloc(e, &e->d_logtab, (size_t)cfg->max_sims + 16)) ||
      (r = dalloc(e, &e->d_rc_meta, (size_t)Gm * 3)))
    return bail(r);
  e->pack_tab_convs = 2 * 64 + 3;      // networks of up to 64 residual blocks are packed without an allocation
  if ((r = dalloc(e, &e->d_pack_tab, (size_t)e->pack_tab_convs * sizeof(PackConv) + 16))) return bail(r);
  {
    // log(sqrt(N_parent)) (node.cpp:53-54) tabulated with the HOST libm so that the device PUCT
    // sees exactly the bits the reference's std::log produces; +,*,/,sqrt are IEEE on both sides.
    std::vector<double> lt((size_t)cfg->max_sims + 16);
    for (size_t i = 0; i < lt.size(); ++i) lt[i] = i == 0 ? 0.0 : std::log(std::sqrt((double)i));
    if (hipMemcpy(e->d_logtab, lt.data(), lt.size() * sizeof(double), hipMemcpyHostToDevice) != hipSuccess) {
      e->err = "logtab upload failed";
      return bail(FPC_ENODEVICE);
    }
  }
#ifndef FPC_EMUL
  if ((r = e->nn.init(e->dc, Gm, cfg->nn_dtype, e->stream, &e->err))) return bail(r);
#endif
  *out = e;
  return 0;
}

void fpc_destroy(fpc_engine *e) {
  if (!e) return;
  (void)hipSetDevice(e->cfg.device);
  (void)fpc_comm_destroy(e);
#ifndef FPC_EMUL
  e->nn.destroy();
#endif
  for (void *p : e->allocs) (void)hipFree(p);
  for (auto &ev : e->evpool) if (ev) (void)hipEventDestroy(ev);
  for (auto &ev : e->rp_ev) if (ev) (void)hipEventDestroy(ev);
  for (auto &ev : e->play_ev) if (ev) (void)hipEventDestroy(ev);
  for (auto &ev : e->pk_ev) if (ev) (void)hipEventDestroy(ev);
  if (e->stream) (void)hipStreamDestroy(e->stream);
  delete e;
}

// ------------------------------------------------------------------------------------------------
int fpc_boards_legal_moves(fpc_engine *e, fpc_board *boards, int n, fpc_move *moves, int *counts) {
  if (!e || !boards || !moves || !counts || n < 0) return fail(e, FPC_EINVAL, "bad argument");
  USE_DEV(e);
  if (n == 0) return 0;
  int r;
  if ((r = check_boards(e, boards, n))) return r;
  if ((r = run_board_ops(e, boards, n, OP_LEGAL, nullptr, nullptr))) return r;
  HIPCHK(e, hipMemcpyAsync(boards, e->d_boards, (size_t)n * sizeof(fpc_board), hipMemcpyDeviceToHost, e->stream));
  HIPCHK(e, hipMemcpyAsync(counts, e->d_counts, (size_t)n * sizeof(int), hipMemcpyDeviceToHost, e->stream));
  HIPCHK(e, hipMemcpyAsync(moves, e->d_moves, (size_t)n * FPC_MAX_MOVES * sizeof(fpc_move), hipMemcpyDeviceToHost, e->stream));
  return fetch_errs(e, n, "board");
}

int fpc_boards_game_result(fpc_engine *e, fpc_board *boards, int n, const int *player, int *results) {
  if (!e || !boards || !results || n < 0) return fail(e, FPC_EINVAL, "bad argument");
  USE_DEV(e);
  if (n == 0) return 0;
  int r;
  if ((r = check_boards(e, boards, n))) return r;
  if ((r = run_board_ops(e, boards, n, OP_RESULT, player, nullptr))) return r;
  HIPCHK(e, hipMemcpyAsync(boards, e->d_boards, (size_t)n * sizeof(fpc_board), hipMemcpyDeviceToHost, e->stream));
  HIPCHK(e, hipMemcpyAsync(results, e->d_results, (size_t)n * sizeof(int), hipMemcpyDeviceToHost, e->stream));
  return fetch_errs(e, n, "board");
}

int fpc_boards_take_action(fpc_engine *e, const fpc_board *boards, const int *flat, int n, fpc_board *out) {
  if (!e || !boards || !flat || !out || n < 0) return fail(e, FPC_EINVAL, "bad argument");
  USE_DEV(e);
  if (n == 0) return 0;
  int r;
  if ((r = check_boards(e, boards, n))) return r;
  for (int i = 0; i < n; ++i)
    if (flat[i] < 0 || flat[i] >= e->dc.A) return fail(e, FPC_EINVAL, "flat index %d out of range", flat[i]);
  if ((r = run_board_ops(e, const_cast<fpc_board *>(boards), n, OP_TAKE, nullptr, flat))) return r;
  HIPCHK(e, hipMemcpyAsync(out, e->d_boards, (size_t)n * sizeof(fpc_board), hipMemcpyDeviceToHost, e->stream));
  return fetch_errs(e, n, "board");
}

int fpc_boards_attack_maps(fpc_engine *e, const fpc_board *boards, int n, uint8_t *out_host) {
  if (!e || !boards || !out_host || n < 0) return fail(e, FPC_EINVAL, "bad argument");
  USE_DEV(e);
  if (n == 0) return 0;
  int r;
  if ((r = check_boards(e, boards, n))) return r;
  if ((r = ensure_board_scratch(e, n))) return r;
  HIPCHK(e, hipMemcpyAsync(e->d_boards, boards, (size_t)n * sizeof(fpc_board), hipMemcpyHostToDevice, e->stream));
  uint8_t *d_maps = reinterpret_cast<uint8_t *>(e->d_dense);       // [n][24][RR] f32 of scratch: room for [n][6][RR] bytes
  FPC_LAUNCH(k_attack_maps, n, 64, e->stream, e->dc, (const fpc_board *)e->d_boards, n, d_maps);
  HIPCHK(e, hipGetLastError());
  HIPCHK(e, hipMemcpyAsync(out_host, d_maps, (size_t)n * 6 * e->dc.RR, hipMemcpyDeviceToHost, e->stream));
  HIPCHK(e, hipStreamSynchronize(e->stream));
  return 0;
}

int fpc_boards_encode(fpc_engine *e, const fpc_board *boards, int n, float *out_host) {
  if (!e || !boards || !out_host || n < 0) return fail(e, FPC_EINVAL, "bad argument");
  USE_DEV(e);
  if (n == 0) return 0;
  int r;
  if ((r = check_boards(e, boards, n))) return r;
  if ((r = ensure_board_scratch(e, n))) return r;
  HIPCHK(e, hipMemcpyAsync(e->d_boards, boards, (size_t)n * sizeof(fpc_board), hipMemcpyHostToDevice, e->stream));
  FPC_LAUNCH(k_encode, n, 64, e->stream, e->dc, (const fpc_board *)e->d_boards, 1, (const int *)nullptr,
             (const int *)nullptr, n, 0, e->d_dense, (uint16_t *)nullptr, (uint16_t)0, (int)boards[0].turn);
  HIPCHK(e, hipGetLastError());
  HIPCHK(e, hipMemcpyAsync(out_host, e->d_dense, (size_t)n * 24 * e->dc.RR * sizeof(float), hipMemcpyDeviceToHost, e->stream));
  HIPCHK(e, hipStreamSynchronize(e->stream));
  return 0;
}

int fpc_boards_legal_mask(fpc_engine *e, fpc_board *boards, int n, float *out_host) {
  if (!e || !boards || !out_host || n < 0) return fail(e, FPC_EINVAL, "bad argument");
  USE_DEV(e);
  if (n == 0) return 0;
  int r;
  if ((r = check_boards(e, boards, n))) return r;
  if ((r = run_board_ops(e, boards, n, OP_LEGAL, nullptr, nullptr))) return r;
  FPC_LAUNCH(k_mask_from_moves, n, 64, e->stream, e->dc, (const fpc_move *)e->d_moves, (const int *)e->d_counts, n, e->d_dense);
  HIPCHK(e, hipGetLastError());
  HIPCHK(e, hipMemcpyAsync(boards, e->d_boards, (size_t)n * sizeof(fpc_board), hipMemcpyDeviceToHost, e->stream));
  HIPCHK(e, hipMemcpyAsync(out_host, e->d_dense, (size_t)n * e->dc.A * sizeof(float), hipMemcpyDeviceToHost, e->stream));
  return fetch_errs(e, n, "board");
}

// ------------------------------------------------------------------------------------------------
// Search.  A simulation step selects a leaf (or K leaves, fpc_search_set_leaves) per game, stages them for the network,
// evaluates them and expands them; for all but the last step of a call the expansion and the NEXT step's selection are
// one launch (k_expand(_legal)_select(_multi)), so a step is 4 dependent kernels instead of 5.  fpc_search_run drives
// that sequence with the internal network; the step entry points (fpc_search_select / _expand_select / _expand) drive
// it for an external evaluator.  Both go through the same helpers: admit (the checks and the max_sims accounting of a
// call that selects), launch_select, stage_leaves (fpc_search_run) or finish_select (step entry points), and
// launch_expand, which picks the expansion kernel.  The selection waiting to be expanded is described by rows_k and
// pending_vl; only launch_select and launch_expand change them.

// every call that selects checks that the rows fit (the setting may have changed after fpc_search_results)
static int check_rows(fpc_engine *e, int leaves, int G) {
  if ((long)leaves * G > e->cfg.max_games)
    return fail(e, FPC_EINVAL, "%d leaves x %d games = %ld rows > max_games %d (fpc_search_set_leaves)", leaves, G,
                (long)leaves * G, e->cfg.max_games);
  return 0;
}

int fpc_search_begin(fpc_engine *e, const fpc_board *roots, int n_games, double c_puct) {
  if (!e || !roots || n_games < 1) return fail(e, FPC_EINVAL, "bad argument");
  USE_DEV(e);
  if (n_games > e->cfg.max_games) return fail(e, FPC_EINVAL, "n_games %d > max_games %d", n_games, e->cfg.max_games);
  int r;
  if ((r = check_rows(e, e->leaves, n_games))) return r;
  if (e->t.noise && e->noise_n != n_games)
    return fail(e, FPC_EINVAL, "root noise was uploaded for %d games, this search has %d: call fpc_search_set_root_noise again (or with NULL)", e->noise_n, n_games);
  if ((r = check_boards(e, roots, n_games))) return r;
  e->G = n_games;
  e->Cpuct = c_puct;
  HIPCHK(e, hipMemcpyAsync(e->d_roots, roots, (size_t)n_games * sizeof(fpc_board), hipMemcpyHostToDevice, e->stream));
  if (e->t.S)       // the solver's statuses: every node of the new search is unknown (no kernel gives a node a birth status)
    HIPCHK(e, hipMemsetAsync(e->t.S, 0, (size_t)n_games * e->t.node_cap, e->stream));
  FPC_LAUNCH(k_search_init, n_games, 64, e->stream, e->t, n_games, (const fpc_board *)e->d_roots);
  HIPCHK(e, hipGetLastError());
  e->searching = true;
  e->sims_issued = 0;
  e->base.assign((size_t)n_games, 0);
  e->t.budget = nullptr;          // budgets belong to one ply
  e->t.fast = nullptr;            // and so does the fast-row mask
  e->selected = false;
  e->stepping = true;
  e->multi = e->leaves > 1;
  e->rows_k = 1;
  e->pending_vl = false;
  if (e->multi) {     // leaf-parallel from the start: the roots' counters (children are zeroed where they are created)
    FPC_LAUNCH(k_vl_roots, (n_games + 63) / 64, 64, e->stream, e->d_VL, e->t.node_cap, n_games);
    HIPCHK(e, hipGetLastError());
  }
  return 0;
}

static int check_searching(fpc_engine *e) {
  return !e || !e->searching ? fail(e, FPC_ESTATE, "fpc_search_begin has not been called") : 0;
}

// admission of a call that selects, after its own argument checks: the rows of the engine's leaves per game fit, and
// n more simulations stay within max_sims (pools + log table), which they are then counted against.  With per-game
// budgets set (fpc_search_set_budget) every game is bounded by base[g] + budget[g] <= max_sims instead, whatever the
// number of steps: the batch-wide check does not apply.
static int admit(fpc_engine *e, int n) {
  int r;
  if ((r = check_rows(e, e->leaves, e->G))) return r;
  if (!e->t.budget) {
    if (e->sims_issued + n > e->cfg.max_sims) return fail(e, FPC_ECAPACITY, "more than max_sims = %d simulations since fpc_search_begin", e->cfg.max_sims);
    e->sims_issued += n;
  }
  e->selected = true;
  return 0;
}

static LeafPar leafpar(const fpc_engine *e) { return LeafPar{e->d_VL, e->vl}; }

// the solver is in effect: the switch is on and the rule set holds both FPC_RULES_PUCT and FPC_RULES_TERMINAL
static bool solving(const fpc_engine *e) {
  const int need = FPC_RULES_PUCT | FPC_RULES_TERMINAL;
  return e->solver && e->t.S != nullptr && (e->dc.rules & need) == need;
}

// forced playouts and target pruning are in effect: the factor is > 0 and the rule set holds both FPC_RULES_PUCT and
// FPC_RULES_VISITS
static bool forcing(const fpc_engine *e) {
  const int need = FPC_RULES_PUCT | FPC_RULES_VISITS;
  return e->t.forced > 0.0 && (e->dc.rules & need) == need;
}

// every selecting kernel exists without and with first-play urgency (fpc_search_set_fpu), without and with the solver
// (fpc_search_set_solver) and without and with forced playouts (fpc_search_set_forced): the instance the settings ask for.
// With forcing not in effect these are the four <*, *, false> instances, chosen as before.
#define FPC_LAUNCH_SELECT_F(kernel, e, FORCE, ...)                \
  do {                                                            \
    const bool fpu_ = (e)->t.fpu_mode != FPC_FPU_ZERO;            \
    if (solving(e)) {                                             \
      if (fpu_) FPC_LAUNCH((kernel<true, true, FORCE>), __VA_ARGS__);      \
      else FPC_LAUNCH((kernel<false, true, FORCE>), __VA_ARGS__);          \
    } else if (fpu_) FPC_LAUNCH((kernel<true, false, FORCE>), __VA_ARGS__); \
    else FPC_LAUNCH((kernel<false, false, FORCE>), __VA_ARGS__);           \
  } while (0)
#define FPC_LAUNCH_SELECT(kernel, e, ...)                         \
  do {                                                            \
    if (forcing(e)) FPC_LAUNCH_SELECT_F(kernel, e, true, __VA_ARGS__); \
    else FPC_LAUNCH_SELECT_F(kernel, e, false, __VA_ARGS__);      \
  } while (0)

// k leaves per game (k_select_multi), or one (k_select) in a one-leaf search
static void launch_select(fpc_engine *e, int k) {
  if (e->multi)
    FPC_LAUNCH_SELECT(k_select_multi, e, e->G, 64, e->stream, e->dc, e->t, e->G, k, e->Cpuct, (const double *)e->d_logtab, leafpar(e));
  else
    FPC_LAUNCH_SELECT(k_select, e, e->G, 64, e->stream, e->dc, e->t, e->G, e->Cpuct, (const double *)e->d_logtab);
  e->rows_k = k;
  e->pending_vl = e->multi;
}

// after a k_expand_select launch the leaves it selected become the current ones
static void swap_leaf_arrays(fpc_engine *e) {
  std::swap(e->t.leaf_node, e->t.leaf_node_nx);
  std::swap(e->t.leaf_slot, e->t.leaf_slot_nx);
  std::swap(e->t.leaf_turn, e->t.leaf_turn_nx);
}

// The expansion of the pending selection from the full head's logits (src + softmax chunk statistics) or, with `legal`
// set, from the legal-only head's; with ksel > 0 fused with the selection of the next step's ksel leaves per game.
// A one-leaf selection made before fpc_search_set_leaves switched the search to leaf-parallel holds no pending visit:
// it is expanded by the one-leaf kernel, and the next step's leaves are selected by k_select_multi.
static void launch_expand(fpc_engine *e, const LogitSrc &src, const float *stats, const float *legal, const float *value, int ksel) {
  const int G = e->G, kexp = e->rows_k;
  const bool fuse = ksel > 0, fused = fuse && e->pending_vl == e->multi;    // one launch expands and selects
  const double *logtab = e->d_logtab;
  if (e->pending_vl) {
    if (legal && fuse)
      FPC_LAUNCH_SELECT(k_expand_legal_select_multi, e, G, 64, e->stream, e->dc, e->t, G, kexp, ksel, legal, value, e->Cpuct, logtab, leafpar(e));
    else if (legal)
      FPC_LAUNCH(k_expand_legal_multi, G, 64, e->stream, e->dc, e->t, G, kexp, legal, value, leafpar(e));
    else if (fuse)
      FPC_LAUNCH_SELECT(k_expand_select_multi, e, G, EXPAND_THREADS, e->stream, e->dc, e->t, G, kexp, ksel, src, stats, value, e->Cpuct, logtab, leafpar(e));
    else
      FPC_LAUNCH(k_expand_multi, G, EXPAND_THREADS, e->stream, e->dc, e->t, G, kexp, src, stats, value, leafpar(e));
  } else {
    if (legal && fused)
      FPC_LAUNCH_SELECT(k_expand_legal_select, e, G, 64, e->stream, e->dc, e->t, G, legal, value, e->Cpuct, logtab);
    else if (legal)
      FPC_LAUNCH(k_expand_legal, G, 64, e->stream, e->dc, e->t, G, legal, value);
    else if (fused)
      FPC_LAUNCH_SELECT(k_expand_select, e, G, EXPAND_THREADS, e->stream, e->dc, e->t, G, src, stats, value, e->Cpuct, logtab);
    else
      FPC_LAUNCH(k_expand, G, EXPAND_THREADS, e->stream, e->dc, e->t, G, src, stats, value);
  }
  if (fused) swap_leaf_arrays(e);
  else if (fuse) launch_select(e, ksel);
  e->rows_k = fuse ? ksel : 1;
  e->pending_vl = fuse && e->multi;
}

// softmax chunk statistics of logits that did not come from the internal policy Linear (one record set per row; under
// the live-row numbering the caller's buffers hold the n_live live rows only)
static void launch_partials(fpc_engine *e, const float *logits_dev) {
  const int nchunks = (e->dc.A / 4 + SM_THREADS - 1) / SM_THREADS, rows = e->t.inv ? e->live_n : e->rows_k * e->G;
  if (rows == 0) return;
  FPC_LAUNCH(k_softmax_partials, rows * nchunks, SM_THREADS, e->stream, logits_dev, e->dc.A, rows, nchunks, e->d_stats);
}

// the leaf-parallel kernels leave the GLOBAL pool index g*board_cap + slot in leaf_slot: the encoders read it with stride 0
static int leaf_board_stride(const fpc_engine *e) { return e->pending_vl ? 0 : e->t.board_cap; }

// fpc_search_set_live_rows: the four arrays of k_live_rows (live_row | inv | c_slot | c_turn) and its count
static int *live_array(const fpc_engine *e, int i) { return e->d_live + (size_t)i * e->cfg.max_games; }
static int *live_count(const fpc_engine *e) { return live_array(e, 4); }

// After EVERY selection: with the switch on, its live rows are numbered (k_live_rows) and the numbering is latched into
// t.inv, which the expansion of that selection reads; with it off t.inv is null and nothing is launched.
static void number_live_rows(fpc_engine *e) {
  if (!e->live_rows) { e->t.inv = nullptr; return; }
  FPC_LAUNCH(k_live_rows, 1, LIVE_THREADS, e->stream, (const int *)e->t.leaf_node, (const int *)e->t.leaf_slot, (const int *)e->t.leaf_turn,
             e->rows_k * e->G, e->G, leaf_board_stride(e), live_array(e, 0), live_array(e, 1), live_array(e, 2), live_array(e, 3), live_count(e));
  e->t.inv = live_array(e, 1);
}

// the step entry points: the pending leaves encoded in f32 for the external evaluator, and how many are live
static int finish_select(fpc_engine *e, int *n_live, const float **enc_dev) {
  const int rows = e->rows_k * e->G;
  number_live_rows(e);
  const bool compact = e->t.inv != nullptr;     // rows 0..n_live-1 hold the live leaves in ascending row order, the rest are zero
  FPC_LAUNCH(k_encode, rows, 64, e->stream, e->dc, (const fpc_board *)e->t.boards, compact ? 0 : leaf_board_stride(e),
             (const int *)(compact ? live_array(e, 2) : e->t.leaf_slot), (const int *)(compact ? live_array(e, 3) : e->t.leaf_turn), rows, 0,
             e->d_enc_f32, (uint16_t *)nullptr, (uint16_t)0, -1);
  HIPCHK(e, hipGetLastError());
  mark(e, 1);
  e->stats.launches_select++;
  int live = 0;
  if (compact) {
    HIPCHK(e, hipMemcpyAsync(&live, live_count(e), sizeof(int), hipMemcpyDeviceToHost, e->stream));
    HIPCHK(e, hipStreamSynchronize(e->stream));
    e->live_n = live;
  } else {
    std::vector<int> slots(rows);
    HIPCHK(e, hipMemcpyAsync(slots.data(), e->t.leaf_slot, (size_t)rows * sizeof(int), hipMemcpyDeviceToHost, e->stream));
    HIPCHK(e, hipStreamSynchronize(e->stream));
    for (int s : slots) live += s >= 0;
  }
  if (n_live) *n_live = live;
  if (enc_dev) *enc_dev = e->d_enc_f32;
  return 0;
}

int fpc_search_select(fpc_engine *e, int *n_live, const float **enc_dev) {
  int r;
  if ((r = check_searching(e))) return r;
  USE_DEV(e);
  if ((r = admit(e, e->leaves))) return r;
  mark(e, 0);
  launch_select(e, e->leaves);
  return finish_select(e, n_live, enc_dev);
}

int fpc_search_expand_select(fpc_engine *e, const float *logits_dev, const float *value_dev, int *n_live, const float **enc_dev) {
  int r;
  if ((r = check_searching(e))) return r;
  USE_DEV(e);
  if (!logits_dev || !value_dev) return fail(e, FPC_EINVAL, "null logits/value");
  if ((r = admit(e, e->leaves))) return r;
  mark(e, 3);
  launch_partials(e, logits_dev);
  launch_expand(e, LogitSrc{logits_dev, nullptr, nullptr, 0, 0, 0, 0, 256}, e->d_stats, nullptr, value_dev, e->leaves);
  HIPCHK(e, hipGetLastError());
  mark(e, 4);
  e->stats.launches_expand++;
  mark(e, 0);
  return finish_select(e, n_live, enc_dev);
}

int fpc_search_expand(fpc_engine *e, const float *logits_dev, const float *value_dev) {
  int r;
  if ((r = check_searching(e))) return r;
  USE_DEV(e);
  if (!logits_dev || !value_dev) return fail(e, FPC_EINVAL, "null logits/value");
  mark(e, 3);
  launch_partials(e, logits_dev);
  launch_expand(e, LogitSrc{logits_dev, nullptr, nullptr, 0, 0, 0, 0, 256}, e->d_stats, nullptr, value_dev, 0);
  HIPCHK(e, hipGetLastError());
  mark(e, 4);
  e->stats.launches_expand++;
  return 0;
}

int fpc_search_set_budget(fpc_engine *e, const int *budget, int n_games) {
  if (!e) return fail(e, FPC_EINVAL, "null engine");
  if (!e->searching)
    return fail(e, FPC_ESTATE, "fpc_search_set_budget needs a search in progress: after fpc_search_begin / fpc_search_advance(_refill)");
  if (e->selected && e->stepping)
    return fail(e, FPC_ESTATE, "fpc_search_set_budget: a selection has been issued since the last fpc_search_begin / fpc_search_advance");
  if (e->selected)      // (results read right after a begin / advance, before any selection, leave the search where it was)
    return fail(e, FPC_ESTATE, "fpc_search_set_budget: the search is finished (fpc_search_results has been read): advance it or begin another");
  if (n_games != e->G) return fail(e, FPC_EINVAL, "fpc_search_set_budget: n_games %d, the search has %d games", n_games, e->G);
  if (!budget) {
    e->t.budget = nullptr;
    return 0;
  }
  for (int g = 0; g < n_games; ++g)
    if (budget[g] < 0) return fail(e, FPC_EINVAL, "fpc_search_set_budget: budget[%d] = %d is negative", g, budget[g]);
  for (int g = 0; g < n_games; ++g)
    if ((long)e->base[g] + budget[g] > e->cfg.max_sims)
      return fail(e, FPC_ECAPACITY, "fpc_search_set_budget: game %d: %d simulations kept + budget %d > max_sims = %d", g, e->base[g],
                  budget[g], e->cfg.max_sims);
  USE_DEV(e);
  int r;
  if (!e->d_budget && (r = dalloc(e, &e->d_budget, (size_t)e->cfg.max_games))) return r;
  // pageable host memory: the copy has left `budget` when the call returns
  HIPCHK(e, hipMemcpyAsync(e->d_budget, budget, (size_t)n_games * sizeof(int), hipMemcpyHostToDevice, e->stream));
  e->t.budget = e->d_budget;
  return 0;
}

int fpc_search_set_fast_rows(fpc_engine *e, const uint8_t *fast, int n_games) {
  if (!e) return fail(e, FPC_EINVAL, "null engine");
  if (!e->searching)
    return fail(e, FPC_ESTATE, "fpc_search_set_fast_rows needs a search in progress: after fpc_search_begin / fpc_search_advance(_refill)");
  if (e->selected && e->stepping)
    return fail(e, FPC_ESTATE, "fpc_search_set_fast_rows: a selection has been issued since the last fpc_search_begin / fpc_search_advance");
  if (e->selected)
    return fail(e, FPC_ESTATE, "fpc_search_set_fast_rows: the search is finished (fpc_search_results has been read): advance it or begin another");
  if (n_games != e->G) return fail(e, FPC_EINVAL, "fpc_search_set_fast_rows: n_games %d, the search has %d games", n_games, e->G);
  if (!fast) {
    e->t.fast = nullptr;
    return 0;
  }
  for (int g = 0; g < n_games; ++g)
    if (fast[g] > 1) return fail(e, FPC_EINVAL, "fpc_search_set_fast_rows: fast[%d] = %d is neither 0 nor 1", g, (int)fast[g]);
  USE_DEV(e);
  int r;
  // whole words: the FORCE instances of select_game read the aligned word that holds a game's byte
  if (!e->d_fast && (r = dalloc(e, &e->d_fast, ((size_t)e->cfg.max_games + 3) & ~(size_t)3))) return r;
  // pageable host memory: the copy has left `fast` when the call returns
  HIPCHK(e, hipMemcpyAsync(e->d_fast, fast, (size_t)n_games, hipMemcpyHostToDevice, e->stream));
  e->t.fast = e->d_fast;
  return 0;
}

int fpc_search_set_leaves(fpc_engine *e, int leaves, double virtual_loss) {
  if (!e) return fail(e, FPC_EINVAL, "null engine");
  if (leaves < 1 || leaves > FPC_MAX_LEAVES) return fail(e, FPC_EINVAL, "leaves %d outside 1..%d", leaves, FPC_MAX_LEAVES);
  if (!std::isfinite(virtual_loss) || virtual_loss < 0.0) return fail(e, FPC_EINVAL, "virtual_loss must be finite and >= 0");
  int r;
  if (e->stepping && (r = check_rows(e, leaves, e->G))) return r;   // a running search; every selection re-checks (admit)
  USE_DEV(e);
  if (leaves > 1 && !e->d_VL) {
    if ((r = dalloc(e, &e->d_VL, (size_t)e->cfg.max_games * e->t.node_cap))) return r;
  }
  if (leaves > 1 && e->searching && !e->multi) {
    // a search that started with one leaf per game: its nodes were created without pending-visit counters (a pending
    // one-leaf selection holds none either: launch_expand expands it with the one-leaf kernel)
    HIPCHK(e, hipMemsetAsync(e->d_VL, 0, (size_t)e->cfg.max_games * e->t.node_cap * sizeof(int), e->stream));
    e->multi = true;
  }
  e->leaves = leaves;
  e->vl = virtual_loss;
  return 0;
}

int fpc_search_set_fpu(fpc_engine *e, int mode, double reduction) {
  if (!e) return fail(e, FPC_EINVAL, "null engine");
  if (mode != FPC_FPU_ZERO && mode != FPC_FPU_PARENT) return fail(e, FPC_EINVAL, "fpc_search_set_fpu: mode %d outside 0..1", mode);
  if (!std::isfinite(reduction)) return fail(e, FPC_EINVAL, "fpc_search_set_fpu: reduction must be finite");
  e->t.fpu_mode = mode;           // read by select_game from the next selection on
  e->t.fpu_red = reduction;
  return 0;
}

int fpc_search_set_live_rows(fpc_engine *e, int on) {
  if (!e) return fail(e, FPC_EINVAL, "null engine");
  if (on < 0 || on > 1) return fail(e, FPC_EINVAL, "fpc_search_set_live_rows: on = %d outside 0..1", on);
  if (e->searching && e->selected && e->stepping)
    return fail(e, FPC_ESTATE, "fpc_search_set_live_rows: a selection has been issued and the search's results have not been read");
  USE_DEV(e);
  int r;
  if (on && !e->d_live && (r = dalloc(e, &e->d_live, (size_t)4 * e->cfg.max_games + 1))) return r;
  e->live_rows = on != 0;
  return 0;
}

int fpc_search_set_solver(fpc_engine *e, int on) {
  if (!e) return fail(e, FPC_EINVAL, "null engine");
  if (on < 0 || on > 1) return fail(e, FPC_EINVAL, "fpc_search_set_solver: on = %d outside 0..1", on);
  if (e->searching && e->selected && e->stepping)
    return fail(e, FPC_ESTATE, "fpc_search_set_solver: a selection has been issued and the search's results have not been read");
  USE_DEV(e);
  int r;
  const size_t nn = (size_t)e->cfg.max_games * e->t.node_cap;
  if (on && !e->t.S) {              // zeroed by dalloc: a search in progress that has selected nothing holds no proof
    uint8_t *s1 = nullptr, *s2 = nullptr;
    if ((r = dalloc(e, &s1, nn))) return r;
    if (e->t2.N && (r = dalloc(e, &s2, nn))) return r;
    e->t.S = s1;
    e->t2.S = s2;
  }
  e->solver = on != 0;
  return 0;
}

int fpc_search_proofs(fpc_engine *e, int max_children, uint8_t *root_proof, uint8_t *child_proof) {
  if (!e || !e->searching) return fail(e, FPC_ESTATE, "fpc_search_begin has not been called");
  if (max_children < 0 || !root_proof) return fail(e, FPC_EINVAL, "fpc_search_proofs: bad max_children or null root_proof");
  USE_DEV(e);
  const int G = e->G;
  const size_t nch = (size_t)G * max_children;
  if (!e->t.S) {                    // the solver was never switched on
    std::fill(root_proof, root_proof + G, (uint8_t)FPC_PROOF_UNKNOWN);
    if (child_proof) std::fill(child_proof, child_proof + nch, (uint8_t)FPC_PROOF_UNKNOWN);
    return 0;
  }
  int r;
  if ((size_t)G + nch > e->proof_cap) {
    if (e->d_proof) {
      (void)hipFree(e->d_proof);
      e->allocs.erase(std::find(e->allocs.begin(), e->allocs.end(), (void *)e->d_proof));
      e->d_proof = nullptr;
    }
    e->proof_cap = 0;
    if ((r = dalloc(e, &e->d_proof, (size_t)G + nch))) return r;
    e->proof_cap = (size_t)G + nch;
  }
  uint8_t *d_out = e->d_proof;
  FPC_LAUNCH(k_root_proofs, G, 64, e->stream, e->t, G, max_children, d_out, d_out + G);
  HIPCHK(e, hipGetLastError());
  HIPCHK(e, hipMemcpyAsync(root_proof, d_out, (size_t)G, hipMemcpyDeviceToHost, e->stream));
  if (child_proof && nch) HIPCHK(e, hipMemcpyAsync(child_proof, d_out + G, nch, hipMemcpyDeviceToHost, e->stream));
  HIPCHK(e, hipStreamSynchronize(e->stream));
  return 0;
}

int fpc_search_set_forced(fpc_engine *e, double factor) {
  if (!e) return fail(e, FPC_EINVAL, "null engine");
  if (!std::isfinite(factor) || factor < 0.0) return fail(e, FPC_EINVAL, "fpc_search_set_forced: factor must be finite and >= 0");
  if (e->searching && e->selected && e->stepping)
    return fail(e, FPC_ESTATE, "fpc_search_set_forced: a selection has been issued and the search's results have not been read");
  e->t.forced = factor;           // read by the FORCE instances and by root_targets; t2 is only ever a set of arrays
  return 0;
}

int fpc_search_targets(fpc_engine *e, int max_children, int *child_target) {
  if (!e || !e->searching) return fail(e, FPC_ESTATE, "fpc_search_begin has not been called");
  if (max_children < 0 || !child_target) return fail(e, FPC_EINVAL, "fpc_search_targets: bad max_children or null child_target");
  USE_DEV(e);
  const int G = e->G;
  const size_t nch = (size_t)G * max_children;
  if (!nch) return 0;
  int r;
  if (nch > e->target_cap) {
    if (e->d_target) {
      (void)hipFree(e->d_target);
      e->allocs.erase(std::find(e->allocs.begin(), e->allocs.end(), (void *)e->d_target));
      e->d_target = nullptr;
    }
    e->target_cap = 0;
    if ((r = dalloc(e, &e->d_target, nch))) return r;
    e->target_cap = nch;
  }
  FPC_LAUNCH(k_root_targets, G, 64, e->stream, e->t, G, max_children, e->Cpuct, forcing(e) ? 1 : 0, e->d_target);
  HIPCHK(e, hipGetLastError());
  HIPCHK(e, hipMemcpyAsync(child_target, e->d_target, nch * sizeof(int), hipMemcpyDeviceToHost, e->stream));
  HIPCHK(e, hipStreamSynchronize(e->stream));
  return 0;
}

#ifndef FPC_EMUL
// the pending leaves as the network's input: the tower megakernels encode them themselves, the other paths take k_encode's.
// Under the live-row numbering the network's row j is the j-th live leaf (k_live_rows' c_slot / c_turn, global pool
// indices: stride 0), rows n_live.. are dead, and beyond one 256-row tile the policy Linear skips the tiles without a
// live row (single-tile shapes pass no count: they run exactly the kernels of the switch off).
static void stage_leaves(fpc_engine *e) {
  const int rows = e->rows_k * e->G;
  const bool compact = e->t.inv != nullptr;
  const int stride = compact ? 0 : leaf_board_stride(e);
  const int *slot = compact ? live_array(e, 2) : e->t.leaf_slot, *turn = compact ? live_array(e, 3) : e->t.leaf_turn;
  e->nn.set_live_count(compact && rows > 256 ? live_count(e) : nullptr);
  if (e->nn.takes_boards())
    e->nn.set_board_input((const fpc_board *)e->t.boards, stride, slot, turn);
  else
    FPC_LAUNCH(k_encode, rows, 64, e->stream, e->dc, (const fpc_board *)e->t.boards, stride, slot, turn, rows, 1, (float *)nullptr,
               e->nn.input16(), e->nn.one16(), -1);
}
#endif

int fpc_search_run(fpc_engine *e, int sims) {
  int r;
  if ((r = check_searching(e))) return r;
  USE_DEV(e);
  if (sims < 0 || sims > e->cfg.max_sims) return fail(e, FPC_EINVAL, "sims %d > max_sims %d", sims, e->cfg.max_sims);
  if ((r = admit(e, sims))) return r;
#ifdef FPC_EMUL
  return fail(e, FPC_EWEIGHTS, "the internal ResNet exists only in the gfx950 build");
#else
  if (!e->nn.loaded) return fail(e, FPC_EWEIGHTS, "fpc_load_weights has not been called");
  // ceil(sims / K) steps of K leaves per game, the last one of the remainder (K = 1 in a one-leaf search)
  const int K = e->leaves, steps = (sims + K - 1) / K;
  auto leaves_of = [&](int s) { return s + 1 < steps ? K : sims - K * (steps - 1); };
  const bool legal = e->policy_mode == FPC_POLICY_LEGAL;
  // developer knob (A/B, with FPC_DEV_KNOBS=1): the dense [rows][A] logits matrix is written as well
  const bool dense = getenv("FPC_DEV_KNOBS") && atoi(getenv("FPC_DEV_KNOBS")) != 0 && getenv("FPC_DENSE_LOGITS") != nullptr;
  for (int s = 0; s < steps; ++s) {
    mark(e, 0);
    if (s == 0) launch_select(e, leaves_of(0));
    number_live_rows(e);
    stage_leaves(e);
    mark(e, 1);
    e->nn.mark_fn = [](void *ctx, int tag) { mark((fpc_engine *)ctx, tag); };
    e->nn.mark_ctx = e;
    const int rows = e->rows_k * e->G;
    r = legal ? e->nn.forward_legal(rows, e->t, &e->err) : e->nn.forward(rows, dense, &e->err);
    e->nn.mark_fn = nullptr;
    if (r) return r;
    mark(e, 3);
    launch_expand(e, e->nn.logit_src(dense), (const float *)e->nn.stats(), legal ? (const float *)e->nn.legal_logits() : nullptr,
                  (const float *)e->nn.value(), s + 1 < steps ? leaves_of(s + 1) : 0);
    mark(e, 4);
    e->stats.launches_select++; e->stats.launches_nn++; e->stats.launches_expand++;
  }
  HIPCHK(e, hipGetLastError());
  return 0;
#endif
}

int fpc_search_results(fpc_engine *e, fpc_board *roots_out, int *root_visits, int *n_children, int *sims_done,
                       int max_children, int *child_flat, int *child_visits, float *child_prior,
                       double *child_value_sum) {
  if (!e || !e->searching) return fail(e, FPC_ESTATE, "fpc_search_begin has not been called");
  USE_DEV(e);
  if (max_children < 0) return fail(e, FPC_EINVAL, "bad max_children");
  const int G = e->G;
  int r;
  const size_t need = (size_t)G * std::max(max_children, 1);
  if (need > e->rc_cap) {
    auto drop = [&](auto **p) {
      if (!*p) return;
      (void)hipFree(*p);
      e->allocs.erase(std::find(e->allocs.begin(), e->allocs.end(), (void *)*p));
      *p = nullptr;
    };
    drop(&e->d_rc_i); drop(&e->d_rc_f); drop(&e->d_rc_d);
    e->rc_cap = 0;
    if ((r = dalloc(e, &e->d_rc_i, need * 2)) || (r = dalloc(e, &e->d_rc_f, need)) || (r = dalloc(e, &e->d_rc_d, need))) return r;
    e->rc_cap = need;
  }
  int *d_flat = e->d_rc_i, *d_vis = e->d_rc_i + need, *d_meta = e->d_rc_meta;
  FPC_LAUNCH(k_root_children, G, 64, e->stream, e->t, G, max_children, d_flat, d_vis, e->d_rc_f, e->d_rc_d, d_meta, e->d_roots);
  HIPCHK(e, hipGetLastError());
  std::vector<int> meta((size_t)G * 3), errs(G);
  HIPCHK(e, hipMemcpyAsync(meta.data(), d_meta, meta.size() * sizeof(int), hipMemcpyDeviceToHost, e->stream));
  HIPCHK(e, hipMemcpyAsync(errs.data(), e->t.err, (size_t)G * sizeof(int), hipMemcpyDeviceToHost, e->stream));
  if (roots_out) HIPCHK(e, hipMemcpyAsync(roots_out, e->d_roots, (size_t)G * sizeof(fpc_board), hipMemcpyDeviceToHost, e->stream));
  if (child_flat) HIPCHK(e, hipMemcpyAsync(child_flat, d_flat, need * sizeof(int), hipMemcpyDeviceToHost, e->stream));
  if (child_visits) HIPCHK(e, hipMemcpyAsync(child_visits, d_vis, need * sizeof(int), hipMemcpyDeviceToHost, e->stream));
  if (child_prior) HIPCHK(e, hipMemcpyAsync(child_prior, e->d_rc_f, need * sizeof(float), hipMemcpyDeviceToHost, e->stream));
  if (child_value_sum) HIPCHK(e, hipMemcpyAsync(child_value_sum, e->d_rc_d, need * sizeof(double), hipMemcpyDeviceToHost, e->stream));
  HIPCHK(e, hipStreamSynchronize(e->stream));
  resolve_marks(e);
  uint64_t sims = 0, nodes = 0;
  for (int g = 0; g < G; ++g) {
    if (root_visits) root_visits[g] = meta[(size_t)g * 3 + 0];
    if (n_children) n_children[g] = meta[(size_t)g * 3 + 1];
    if (sims_done) sims_done[g] = meta[(size_t)g * 3 + 2];
    sims += (uint64_t)meta[(size_t)g * 3 + 2];
  }
  (void)nodes;
  e->stats.sims += sims;
  e->stepping = false;
  return err_to_status(e, errs, "game");
}

int fpc_search_grandchildren(fpc_engine *e, int game, int child_idx, int max_children, int *n, int *flat, int *visits) {
  if (!e || !e->searching || game < 0 || game >= e->G || !n) return fail(e, FPC_EINVAL, "bad argument");
  USE_DEV(e);
  HIPCHK(e, hipStreamSynchronize(e->stream));
  const size_t nb = (size_t)game * e->t.node_cap;
  int c0 = -1;
  uint16_t nc = 0;
  HIPCHK(e, hipMemcpy(&c0, e->t.child0 + nb, sizeof(int), hipMemcpyDeviceToHost));
  HIPCHK(e, hipMemcpy(&nc, e->t.nch + nb, sizeof(uint16_t), hipMemcpyDeviceToHost));
  if (c0 < 0 || child_idx < 0 || child_idx >= nc) return fail(e, FPC_EINVAL, "no such root child");
  const size_t ch = nb + c0 + child_idx;
  int g0 = -1;
  uint16_t gn = 0;
  HIPCHK(e, hipMemcpy(&g0, e->t.child0 + ch, sizeof(int), hipMemcpyDeviceToHost));
  HIPCHK(e, hipMemcpy(&gn, e->t.nch + ch, sizeof(uint16_t), hipMemcpyDeviceToHost));
  if (g0 < 0) { *n = 0; return 0; }
  *n = gn;
  const int k = std::min<int>(gn, max_children);
  std::vector<uint16_t> mv(k);
  HIPCHK(e, hipMemcpy(mv.data(), e->t.mv + nb + g0, (size_t)k * sizeof(uint16_t), hipMemcpyDeviceToHost));
  if (visits) HIPCHK(e, hipMemcpy(visits, e->t.N + nb + g0, (size_t)k * sizeof(int), hipMemcpyDeviceToHost));
  if (flat) for (int i = 0; i < k; ++i) flat[i] = mv[i];
  return 0;
}

// ------------------------------------------------------------------------------------------------
// Subtree reuse: the finished search becomes the start of the next one.  k_tree_advance writes the re-rooted trees into
// the second set of tree arrays (games move to lower indices while other blocks still read the old regions), the host
// swaps the two sets, reads the kept root visit counts back and counts max(kept) - 1 simulations as issued: a node
// created with N = 1 and now at N = n has had n - 1 simulations through it, which is the accounting of a fresh root
// after n - 1 simulations for the log table, the board pool and the node pool, so admit() holds as it is.
// fpc_search_advance_refill is the same launch with fresh rows among the kept ones (src_game[i] == -1): a fresh
// root counts as kept with N = 1, i.e. 0 simulations issued.  Under FPC_RULES_VISITS nodes are born with N = 0 and a root
// at N = n has had n simulations through it: max(kept) count as issued, a fresh root is kept with N = 0.
static int advance_impl(fpc_engine *e, const int *src_game, const int *flat, const fpc_board *fresh, int n_games, fpc_board *roots_out,
                        int *kept_visits) {
  USE_DEV(e);
  int r;
  if ((r = check_rows(e, e->leaves, n_games))) return r;
  if (e->t.noise && e->noise_n != n_games)
    return fail(e, FPC_EINVAL, "root noise was uploaded for %d games, this search has %d: call fpc_search_set_root_noise again (or with NULL)", e->noise_n, n_games);
  Tree &t = e->t, &u = e->t2;
  const size_t nn = (size_t)e->cfg.max_games * t.node_cap;
  if ((!u.N && (r = dalloc(e, &u.N, nn))) || (!u.W && (r = dalloc(e, &u.W, nn))) || (!u.P && (r = dalloc(e, &u.P, nn))) ||
      (!u.mv && (r = dalloc(e, &u.mv, nn))) || (!u.parent && (r = dalloc(e, &u.parent, nn))) || (!u.child0 && (r = dalloc(e, &u.child0, nn))) ||
      (!u.nch && (r = dalloc(e, &u.nch, nn))) || (!u.bslot && (r = dalloc(e, &u.bslot, nn))) ||
      (!u.boards && (r = dalloc(e, &u.boards, (size_t)e->cfg.max_games * t.board_cap))) ||
      (t.S && !u.S && (r = dalloc(e, &u.S, nn))) ||
      (!e->d_adv && (r = dalloc(e, &e->d_adv, (size_t)2 * e->cfg.max_games))) ||
      (fresh && !e->d_fresh && (r = dalloc(e, &e->d_fresh, (size_t)e->cfg.max_games))))
    return r;
  int *d_src = e->d_adv, *d_flat = e->d_adv + e->cfg.max_games;
  if (src_game) HIPCHK(e, hipMemcpyAsync(d_src, src_game, (size_t)n_games * sizeof(int), hipMemcpyHostToDevice, e->stream));
  HIPCHK(e, hipMemcpyAsync(d_flat, flat, (size_t)n_games * sizeof(int), hipMemcpyHostToDevice, e->stream));
  if (fresh) {                      // only the rows that are refilled are read from the caller
    e->fresh_stage.assign((size_t)n_games, fpc_board{});
    for (int i = 0; i < n_games; ++i)
      if (src_game[i] < 0) e->fresh_stage[i] = fresh[i];
    HIPCHK(e, hipMemcpyAsync(e->d_fresh, e->fresh_stage.data(), (size_t)n_games * sizeof(fpc_board), hipMemcpyHostToDevice, e->stream));
  }
  if (t.S)          // the statuses travel with the nodes k_tree_advance moves; everything else in the regions written is unknown
    HIPCHK(e, hipMemsetAsync(u.S, 0, (size_t)n_games * t.node_cap, e->stream));
  Tree o = t;
  o.S = u.S;
  o.N = u.N; o.W = u.W; o.P = u.P; o.mv = u.mv; o.parent = u.parent; o.child0 = u.child0; o.nch = u.nch; o.bslot = u.bslot; o.boards = u.boards;
  FPC_LAUNCH(k_tree_advance, n_games, 64, e->stream, e->dc, t, o, n_games, src_game ? (const int *)d_src : (const int *)nullptr,
             (const int *)d_flat, fresh ? (const fpc_board *)e->d_fresh : (const fpc_board *)nullptr, e->d_VL, e->d_rc_meta, e->d_roots);
  HIPCHK(e, hipGetLastError());
  std::swap(t.N, u.N); std::swap(t.W, u.W); std::swap(t.P, u.P); std::swap(t.mv, u.mv); std::swap(t.parent, u.parent);
  std::swap(t.child0, u.child0); std::swap(t.nch, u.nch); std::swap(t.bslot, u.bslot); std::swap(t.boards, u.boards);
  std::swap(t.S, u.S);
  e->G = n_games;
  e->stepping = true;
  e->multi = e->leaves > 1;
  e->rows_k = 1;
  e->pending_vl = false;
  e->t.budget = nullptr;          // budgets belong to one ply
  e->t.fast = nullptr;            // and so does the fast-row mask
  e->selected = false;
  std::vector<int> kept(n_games), errs(n_games);
  HIPCHK(e, hipMemcpyAsync(kept.data(), e->d_rc_meta, (size_t)n_games * sizeof(int), hipMemcpyDeviceToHost, e->stream));
  HIPCHK(e, hipMemcpyAsync(errs.data(), t.err, (size_t)n_games * sizeof(int), hipMemcpyDeviceToHost, e->stream));
  if (roots_out) HIPCHK(e, hipMemcpyAsync(roots_out, e->d_roots, (size_t)n_games * sizeof(fpc_board), hipMemcpyDeviceToHost, e->stream));
  HIPCHK(e, hipStreamSynchronize(e->stream));
  const int born = born_visits(e->dc.rules);      // FPC_RULES_VISITS: a root's N IS the number of simulations through it
  e->sims_issued = (long)*std::max_element(kept.begin(), kept.end()) - born;
  e->base.resize((size_t)n_games);
  for (int i = 0; i < n_games; ++i) e->base[i] = std::max(kept[i] - born, 0);     // per game, for fpc_search_set_budget
  if (kept_visits) std::copy(kept.begin(), kept.end(), kept_visits);
  return err_to_status(e, errs, "game");
}

int fpc_search_advance(fpc_engine *e, const int *src_game, const int *flat, int n_games, fpc_board *roots_out, int *kept_visits) {
  if (!e || !flat) return fail(e, FPC_EINVAL, "bad argument");
  if (!e->searching || e->stepping) return fail(e, FPC_ESTATE, "fpc_search_advance needs a finished search: fpc_search_results has not been read");
  if (n_games < 1) return fail(e, FPC_EINVAL, "n_games must be positive");
  if (!src_game && n_games > e->G) return fail(e, FPC_EINVAL, "n_games %d > the %d games of the finished search", n_games, e->G);
  for (int i = 0; src_game && i < n_games; ++i)
    if (src_game[i] < 0 || src_game[i] >= e->G || (i > 0 && src_game[i] <= src_game[i - 1]))
      return fail(e, FPC_EINVAL, "src_game must be strictly ascending within 0..%d (entry %d is %d)", e->G - 1, i, src_game[i]);
  return advance_impl(e, src_game, flat, nullptr, n_games, roots_out, kept_visits);
}

int fpc_search_advance_refill(fpc_engine *e, const int *src_game, const int *flat, const fpc_board *fresh, int n_games, fpc_board *roots_out,
                              int *kept_visits) {
  if (!e || !flat) return fail(e, FPC_EINVAL, "bad argument");
  if (!e->searching || e->stepping)
    return fail(e, FPC_ESTATE, "fpc_search_advance_refill needs a finished search: fpc_search_results has not been read");
  if (n_games < 1) return fail(e, FPC_EINVAL, "n_games must be positive");
  if (!src_game && n_games > e->G) return fail(e, FPC_EINVAL, "n_games %d > the %d games of the finished search", n_games, e->G);
  bool any_fresh = false;
  for (int i = 0, last = -1; src_game && i < n_games; ++i) {
    const int sg = src_game[i];
    if (sg == -1) {
      if (!fresh) return fail(e, FPC_EINVAL, "src_game[%d] is -1 (a fresh row) and fresh is NULL", i);
      any_fresh = true;
      continue;
    }
    if (sg < -1 || sg >= e->G || sg <= last)
      return fail(e, FPC_EINVAL, "src_game must be -1 (a fresh row) or strictly ascending within 0..%d (entry %d is %d)", e->G - 1, i, sg);
    last = sg;
  }
  for (int i = 0; any_fresh && i < n_games; ++i) {
    int r;
    if (src_game[i] == -1 && (r = check_boards(e, fresh + i, 1)))
      return fail(e, FPC_EINVAL, "fresh[%d]: not a board fpc_search_begin takes (castling rights, piece-list length or turn)", i);
  }
  return advance_impl(e, src_game, flat, any_fresh ? fresh : nullptr, n_games, roots_out, kept_visits);
}

// ------------------------------------------------------------------------------------------------
// Device-side move choice: what sits between a finished search and fpc_search_advance / the next fpc_search_begin.
// One k_play_ply launch draws every game's move from its root's visit counts, makes it on a copy of the root state and
// runs GetGameResult on the result; the host sees two ints (and, if asked, the next state) per game.  The only
// transcendental of the draw, pow(N, 1/T), is tabulated here with the host libm (as the PUCT log table is in
// fpc_create) and uploaded when the temperature changes.  Nothing in the tree or in the engine's search state changes.
int fpc_search_play(fpc_engine *e, double temperature, const double *uniform, int *flat_out, int *result_out, fpc_board *next_out) {
  if (!e || !uniform || !flat_out || !result_out) return fail(e, FPC_EINVAL, "fpc_search_play: null argument");
  if (!e->searching || e->stepping) return fail(e, FPC_ESTATE, "fpc_search_play needs a finished search: fpc_search_results has not been read");
  if (!std::isfinite(temperature) || temperature < 0.0) return fail(e, FPC_EINVAL, "fpc_search_play: temperature must be finite and >= 0 (0: argmax)");
  const int G = e->G;
  for (int g = 0; g < G; ++g)
    if (!(uniform[g] >= 0.0 && uniform[g] < 1.0)) return fail(e, FPC_EINVAL, "fpc_search_play: uniform[%d] = %g is not in [0, 1)", g, uniform[g]);
  const size_t ntab = (size_t)e->cfg.max_sims + 16;
  const bool argmax = temperature == 0.0;
  if (!argmax && !std::isfinite(std::pow((double)(ntab - 1), 1.0 / temperature)))
    return fail(e, FPC_EINVAL, "fpc_search_play: pow(%zu, 1/%g) is not finite; use temperature 0 for argmax", ntab - 1, temperature);
  USE_DEV(e);
  int r;
  const size_t Gm = (size_t)e->cfg.max_games;
  if ((!e->d_powtab && (r = dalloc(e, &e->d_powtab, ntab))) || (!e->d_play_u && (r = dalloc(e, &e->d_play_u, Gm))) ||
      (!e->d_play_out && (r = dalloc(e, &e->d_play_out, 3 * Gm))) || (!e->d_play_next && (r = dalloc(e, &e->d_play_next, Gm))))
    return r;
  if (!argmax && temperature != e->powtab_T) {
    std::vector<double> tab(ntab);
    for (size_t v = 0; v < ntab; ++v) tab[v] = std::pow((double)v, 1.0 / temperature);
    e->powtab_T = -1.0;
    HIPCHK(e, hipMemcpyAsync(e->d_powtab, tab.data(), ntab * sizeof(double), hipMemcpyHostToDevice, e->stream));
    HIPCHK(e, hipStreamSynchronize(e->stream));     // `tab` goes out of scope
    e->powtab_T = temperature;
  }
  HIPCHK(e, hipMemcpyAsync(e->d_play_u, uniform, (size_t)G * sizeof(double), hipMemcpyHostToDevice, e->stream));
  int *d_flat = e->d_play_out, *d_res = e->d_play_out + Gm, *d_err = e->d_play_out + 2 * Gm;
  const bool timed = e->timing;
  if (timed)
    for (auto &ev : e->play_ev)
      if (!ev) HIPCHK(e, hipEventCreate(&ev));
  if (timed) HIPCHK(e, hipEventRecord(e->play_ev[0], e->stream));
  FPC_LAUNCH(k_play_ply, G, 64, e->stream, e->dc, e->t, G, (const double *)e->d_powtab, (int)ntab, argmax ? 1 : 0,
             (const double *)e->d_play_u, solving(e) ? 1 : 0, e->Cpuct, forcing(e) ? 1 : 0, d_flat, d_res, e->d_play_next, d_err);
  HIPCHK(e, hipGetLastError());
  if (timed) HIPCHK(e, hipEventRecord(e->play_ev[1], e->stream));
  std::vector<int> errs(G);
  HIPCHK(e, hipMemcpyAsync(flat_out, d_flat, (size_t)G * sizeof(int), hipMemcpyDeviceToHost, e->stream));
  HIPCHK(e, hipMemcpyAsync(result_out, d_res, (size_t)G * sizeof(int), hipMemcpyDeviceToHost, e->stream));
  HIPCHK(e, hipMemcpyAsync(errs.data(), d_err, (size_t)G * sizeof(int), hipMemcpyDeviceToHost, e->stream));
  if (next_out) HIPCHK(e, hipMemcpyAsync(next_out, e->d_play_next, (size_t)G * sizeof(fpc_board), hipMemcpyDeviceToHost, e->stream));
  HIPCHK(e, hipStreamSynchronize(e->stream));
  e->play_ms = -1.f;
  if (timed) HIPCHK(e, hipEventElapsedTime(&e->play_ms, e->play_ev[0], e->play_ev[1]));
  return err_to_status(e, errs, "game");
}

// ------------------------------------------------------------------------------------------------
int fpc_load_weights(fpc_engine *e, const void *blob, uint64_t nbytes) {
  if (!e || !blob) return fail(e, FPC_EINVAL, "bad argument");
  USE_DEV(e);
#ifdef FPC_EMUL
  (void)nbytes;
  return fail(e, FPC_EWEIGHTS, "the internal ResNet exists only in the gfx950 build");
#else
  return e->nn.load(blob, nbytes, &e->err);
#endif
}

int fpc_nn_forward(fpc_engine *e, const float *enc_dev, int n, float *logits_dev, float *value_dev) {
  if (!e || !enc_dev || !logits_dev || !value_dev) return fail(e, FPC_EINVAL, "bad argument");
  USE_DEV(e);
#ifdef FPC_EMUL
  (void)n;
  return fail(e, FPC_EWEIGHTS, "the internal ResNet exists only in the gfx950 build");
#else
  if (!e->nn.loaded) return fail(e, FPC_EWEIGHTS, "fpc_load_weights has not been called");
  if (n < 1 || n > e->cfg.max_games) return fail(e, FPC_EINVAL, "n out of range");
  return e->nn.forward_external(enc_dev, n, logits_dev, value_dev, &e->err);
#endif
}

// ------------------------------------------------------------------------------------------------
// training tuples
int fpc_tuples_reserve(fpc_engine *e, int capacity) {
  if (!e || capacity < 0) return fail(e, FPC_EINVAL, "bad argument");
  // fpc_tuple carries a child's visit count (1 + its simulations, Q1) as u16
  if (e->cfg.max_sims > 65534) return fail(e, FPC_EUNSUPPORTED, "training tuples hold visit counts as u16: max_sims %d > 65534", e->cfg.max_sims);
  USE_DEV(e);
  if (e->d_tuples) {
    (void)hipFree(e->d_tuples);
    e->allocs.erase(std::find(e->allocs.begin(), e->allocs.end(), (void *)e->d_tuples));
    e->d_tuples = nullptr;
  }
  e->tuple_cap = e->tuple_count = 0;
  int r;
  if (capacity > 0 && (r = dalloc(e, &e->d_tuples, (size_t)capacity))) return r;
  if (!e->d_tgame && ((r = dalloc(e, &e->d_tgame, (size_t)e->cfg.max_games)) || (r = dalloc(e, &e->d_tz, (size_t)2 * e->cfg.max_games)))) return r;
  e->tuple_cap = capacity;
  return 0;
}

int fpc_tuples_reset(fpc_engine *e) {
  if (!e) return FPC_EINVAL;
  e->tuple_count = 0;
  return 0;
}

int fpc_collect_tuples(fpc_engine *e, const int *game_id, int ply) {
  if (!e || !e->searching) return fail(e, FPC_ESTATE, "fpc_search_begin has not been called");
  USE_DEV(e);
  const int G = e->G;
  if (e->tuple_count + G > e->tuple_cap) return fail(e, FPC_ECAPACITY, "tuple buffer full (%d + %d > %d): fpc_tuples_reserve", e->tuple_count, G, e->tuple_cap);
  if (game_id) HIPCHK(e, hipMemcpyAsync(e->d_tgame, game_id, (size_t)G * sizeof(int), hipMemcpyHostToDevice, e->stream));
  FPC_LAUNCH(k_collect_tuples, G, 64, e->stream, e->t, G, game_id ? (const int *)e->d_tgame : (const int *)nullptr, ply, e->Cpuct,
             forcing(e) ? 1 : 0, e->d_tuples + e->tuple_count);
  HIPCHK(e, hipGetLastError());
  if (game_id) HIPCHK(e, hipStreamSynchronize(e->stream));     // the caller may reuse game_id
  e->tuple_count += G;
  return 0;
}

int fpc_tuples_set_z(fpc_engine *e, const int *game_id, const float *z_team0, const float *z_team1, int n) {
  if (!e || !game_id || !z_team0 || !z_team1 || n < 0) return fail(e, FPC_EINVAL, "bad argument");
  if (n > e->cfg.max_games) return fail(e, FPC_EINVAL, "more games than max_games in one fpc_tuples_set_z call");
  if (n == 0 || e->tuple_count == 0) return 0;
  USE_DEV(e);
  HIPCHK(e, hipMemcpyAsync(e->d_tgame, game_id, (size_t)n * sizeof(int), hipMemcpyHostToDevice, e->stream));
  HIPCHK(e, hipMemcpyAsync(e->d_tz, z_team0, (size_t)n * sizeof(float), hipMemcpyHostToDevice, e->stream));
  HIPCHK(e, hipMemcpyAsync(e->d_tz + e->cfg.max_games, z_team1, (size_t)n * sizeof(float), hipMemcpyHostToDevice, e->stream));
  FPC_LAUNCH(k_tuples_set_z, (e->tuple_count + 255) / 256, 256, e->stream, e->d_tuples, e->tuple_count, (const int *)e->d_tgame,
             (const float *)e->d_tz, (const float *)(e->d_tz + e->cfg.max_games), n);
  HIPCHK(e, hipGetLastError());
  HIPCHK(e, hipStreamSynchronize(e->stream));
  return 0;
}

int fpc_tuples_count(fpc_engine *e) { return e ? e->tuple_count : FPC_EINVAL; }

int fpc_tuples_read(fpc_engine *e, fpc_tuple *host_out, int first, int n) {
  if (!e || !host_out || first < 0 || n < 0 || first + n > e->tuple_count) return fail(e, FPC_EINVAL, "bad tuple range");
  if (n == 0) return 0;
  USE_DEV(e);
  HIPCHK(e, hipMemcpyAsync(host_out, e->d_tuples + first, (size_t)n * sizeof(fpc_tuple), hipMemcpyDeviceToHost, e->stream));
  HIPCHK(e, hipStreamSynchronize(e->stream));
  return 0;
}

// ------------------------------------------------------------------------------------------------
// device-resident replay
namespace {
void dfree(fpc_engine *e, void *p) {
  if (!p) return;
  (void)hipFree(p);
  e->allocs.erase(std::find(e->allocs.begin(), e->allocs.end(), p));
}

int ensure_replay_idx(fpc_engine *e, size_t ints) {
  if (ints <= e->rp_idx_cap) return 0;
  dfree(e, e->d_rp_idx);
  e->d_rp_idx = nullptr;
  e->rp_idx_cap = 0;
  const size_t cap = std::max<size_t>(ints, 1024);
  int r;
  if ((r = dalloc(e, &e->d_rp_idx, cap))) return r;
  e->rp_idx_cap = cap;
  return 0;
}

bool bad_ring(int ring) { return ring < 0 || ring > FPC_REPLAY_SCRATCH; }
}  // namespace

int fpc_replay_reserve(fpc_engine *e, int ring, int capacity) {
  if (!e || bad_ring(ring) || capacity < 1) return fail(e, FPC_EINVAL, "fpc_replay_reserve: ring %d / capacity %d out of range", ring, capacity);
  USE_DEV(e);
  fpc_engine::Ring &g = e->ring[ring];
  // k_replay_store addresses both rings through one int index space
  if (ring < FPC_REPLAY_RINGS && (long long)capacity + e->ring[1 - ring].cap > 0x7fffffffLL) return fail(e, FPC_EINVAL, "fpc_replay_reserve: the two capacities together exceed 2^31 - 1");
  if (capacity != g.cap) {       // the new ring exists before the old one goes: FPC_ENOMEM leaves the ring as it was
    fpc_tuple *d = nullptr;
    int r;
    if ((r = dalloc(e, &d, (size_t)capacity))) return r;
    HIPCHK(e, hipStreamSynchronize(e->stream));
    dfree(e, g.d);
    g.d = d;
    g.cap = capacity;
  }
  g.size = g.next = 0;           // same capacity: the allocation stays, only the cursors go back
  return 0;
}

int fpc_replay_size(fpc_engine *e, int ring) {
  if (!e || bad_ring(ring)) return fail(e, FPC_EINVAL, "fpc_replay_size: ring %d out of range", ring);
  return e->ring[ring].size;
}

int fpc_replay_push(fpc_engine *e, int source, const int *src_index, const int8_t *ring_of, int m) {
  if (!e || m < 0 || (source != FPC_REPLAY_COLLECTED && source != FPC_REPLAY_GATHERED)) return fail(e, FPC_EINVAL, "fpc_replay_push: bad argument");
  const fpc_tuple *src = nullptr;
  int count = 0;
  if (source == FPC_REPLAY_COLLECTED) {
    src = e->d_tuples;
    count = e->tuple_count;
  } else {
    if (!e->d_gather || e->gather_counts.empty()) return fail(e, FPC_ESTATE, "fpc_replay_push: fpc_allgather_tuples has not been called");
    src = e->d_gather;
    for (int c : e->gather_counts) count += c;
  }
  // every argument is checked before a cursor moves
  for (int j = 0; j < m; ++j) {
    const int rg = ring_of ? (int)ring_of[j] : 0, si = src_index ? src_index[j] : j;
    if (rg < -1 || rg >= FPC_REPLAY_RINGS) return fail(e, FPC_EINVAL, "fpc_replay_push: ring_of[%d] = %d outside -1..%d", j, rg, FPC_REPLAY_RINGS - 1);
    if (si < 0 || si >= count) return fail(e, FPC_EINVAL, "fpc_replay_push: source index %d (entry %d) outside 0..%d", si, j, count - 1);
    if (rg >= 0 && !e->ring[rg].d) return fail(e, FPC_ESTATE, "fpc_replay_push: ring %d has not been reserved (fpc_replay_reserve)", rg);
  }
  USE_DEV(e);
  fpc_engine::Ring cur[FPC_REPLAY_RINGS];
  for (int k = 0; k < FPC_REPLAY_RINGS; ++k) cur[k] = e->ring[k];
  const int cap0 = cur[0].cap;
  std::unordered_map<int, int> at;          // destination -> its entry of the launch lists (the last writer of a slot wins)
  std::vector<int> lists[2];                // source | destination
  for (int j = 0; j < m; ++j) {
    const int rg = ring_of ? (int)ring_of[j] : 0;
    if (rg < 0) continue;
    int si = src_index ? src_index[j] : j;
    if (source == FPC_REPLAY_GATHERED) {    // logical index -> (rank, local index): ranks are stored max-padded
      int r = 0;
      while (si >= e->gather_counts[r]) si -= e->gather_counts[r++];
      si += r * e->gather_stride;
    }
    fpc_engine::Ring &g = cur[rg];
    const int dst = (rg ? cap0 : 0) + g.next;       // ReplayBuffer.add: while filling up, _next == len(_items)
    g.next = (g.next + 1) % g.cap;
    g.size = std::min(g.size + 1, g.cap);
    auto it = at.find(dst);
    if (it != at.end()) lists[0][(size_t)it->second] = si;
    else { at.emplace(dst, (int)lists[0].size()); lists[0].push_back(si); lists[1].push_back(dst); }
  }
  const size_t k = lists[0].size();
  if (k) {
    int r;
    if ((r = ensure_replay_idx(e, 2 * k))) return r;
    HIPCHK(e, hipMemcpyAsync(e->d_rp_idx, lists[0].data(), k * sizeof(int), hipMemcpyHostToDevice, e->stream));
    HIPCHK(e, hipMemcpyAsync(e->d_rp_idx + k, lists[1].data(), k * sizeof(int), hipMemcpyHostToDevice, e->stream));
    FPC_LAUNCH(k_replay_store, (int)k, 64, e->stream, src, (const int *)e->d_rp_idx, cur[0].d, cur[1].d, cap0, (const int *)(e->d_rp_idx + k), (int)k);
    HIPCHK(e, hipGetLastError());
    HIPCHK(e, hipStreamSynchronize(e->stream));
  }
  for (int i = 0; i < FPC_REPLAY_RINGS; ++i) e->ring[i] = cur[i];
  return 0;
}

int fpc_replay_load(fpc_engine *e, int ring, const fpc_tuple *host, int n) {
  if (!e || bad_ring(ring) || n < 0 || (!host && n > 0)) return fail(e, FPC_EINVAL, "fpc_replay_load: bad argument");
  fpc_engine::Ring &g = e->ring[ring];
  if (!g.d) return fail(e, FPC_ESTATE, "fpc_replay_load: ring %d has not been reserved (fpc_replay_reserve)", ring);
  if (n == 0) return 0;
  USE_DEV(e);
  // record j goes to slot (next + j) mod capacity; of more than `capacity` records only the last `capacity` survive
  const int first = std::max(0, n - g.cap);
  int j = first;
  while (j < n) {
    const int slot = (int)(((long long)g.next + j) % g.cap), take = std::min(n - j, g.cap - slot);
    HIPCHK(e, hipMemcpyAsync(g.d + slot, host + j, (size_t)take * sizeof(fpc_tuple), hipMemcpyHostToDevice, e->stream));
    j += take;
  }
  HIPCHK(e, hipStreamSynchronize(e->stream));
  g.next = (int)(((long long)g.next + n) % g.cap);
  g.size = (int)std::min<long long>((long long)g.size + n, g.cap);
  return 0;
}

int fpc_replay_read(fpc_engine *e, int ring, fpc_tuple *host_out, int first_slot, int n) {
  if (!e || bad_ring(ring) || !host_out || first_slot < 0 || n < 0 || (long long)first_slot + n > e->ring[ring].size)
    return fail(e, FPC_EINVAL, "fpc_replay_read: bad ring or slot range");
  if (n == 0) return 0;
  USE_DEV(e);
  HIPCHK(e, hipMemcpyAsync(host_out, e->ring[ring].d + first_slot, (size_t)n * sizeof(fpc_tuple), hipMemcpyDeviceToHost, e->stream));
  HIPCHK(e, hipStreamSynchronize(e->stream));
  return 0;
}

// fpc_replay_batch (w_dev null) and fpc_replay_batch_w
static int replay_batch(fpc_engine *e, int ring, const int *slot, int n, float *enc_dev, float *pi_dev, float *z_dev, float *w_dev) {
  if (!e || bad_ring(ring) || n < 0 || !slot || !enc_dev || !pi_dev || !z_dev) return fail(e, FPC_EINVAL, "fpc_replay_batch: bad argument");
  if (((uintptr_t)enc_dev | (uintptr_t)pi_dev) & 15) return fail(e, FPC_EINVAL, "fpc_replay_batch: enc_dev and pi_dev must be 16-byte aligned");
  const fpc_engine::Ring &g = e->ring[ring];
  if (!g.d) return fail(e, FPC_ESTATE, "fpc_replay_batch: ring %d has not been reserved (fpc_replay_reserve)", ring);
  for (int i = 0; i < n; ++i)
    if (slot[i] < 0 || slot[i] >= g.size) return fail(e, FPC_EINVAL, "fpc_replay_batch: slot[%d] = %d outside 0..%d", i, slot[i], g.size - 1);
  if (n == 0) return 0;
  USE_DEV(e);
  int r;
  if ((r = ensure_replay_idx(e, (size_t)n))) return r;
  HIPCHK(e, hipMemcpyAsync(e->d_rp_idx, slot, (size_t)n * sizeof(int), hipMemcpyHostToDevice, e->stream));
  if (e->timing && !e->rp_ev[0]) {
    HIPCHK(e, hipEventCreate(&e->rp_ev[0]));
    HIPCHK(e, hipEventCreate(&e->rp_ev[1]));
  }
  if (e->timing) HIPCHK(e, hipEventRecord(e->rp_ev[0], e->stream));
  FPC_LAUNCH(k_replay_decode, n, RD_THREADS, e->stream, e->dc, (const fpc_tuple *)g.d, (const int *)e->d_rp_idx, n, enc_dev, pi_dev, z_dev, w_dev);
  HIPCHK(e, hipGetLastError());
  if (e->timing) HIPCHK(e, hipEventRecord(e->rp_ev[1], e->stream));
  HIPCHK(e, hipStreamSynchronize(e->stream));
  e->rp_decode_ms = -1.f;
  if (e->timing) HIPCHK(e, hipEventElapsedTime(&e->rp_decode_ms, e->rp_ev[0], e->rp_ev[1]));
  return 0;
}

int fpc_replay_batch(fpc_engine *e, int ring, const int *slot, int n, float *enc_dev, float *pi_dev, float *z_dev) {
  return replay_batch(e, ring, slot, n, enc_dev, pi_dev, z_dev, nullptr);
}

int fpc_replay_batch_w(fpc_engine *e, int ring, const int *slot, int n, float *enc_dev, float *pi_dev, float *z_dev, float *w_dev) {
  if (!w_dev) return fail(e, FPC_EINVAL, "fpc_replay_batch_w: null w_dev");
  return replay_batch(e, ring, slot, n, enc_dev, pi_dev, z_dev, w_dev);
}

int fpc_replay_decode_ms(fpc_engine *e, float *ms_out) {
  if (!e || !ms_out) return fail(e, FPC_EINVAL, "bad argument");
  if (e->rp_decode_ms < 0.f) return fail(e, FPC_ESTATE, "fpc_replay_decode_ms: no fpc_replay_batch has run with fpc_set_timing on");
  *ms_out = e->rp_decode_ms;
  return 0;
}

int fpc_search_play_ms(fpc_engine *e, float *ms_out) {
  if (!e || !ms_out) return fail(e, FPC_EINVAL, "bad argument");
  if (e->play_ms < 0.f) return fail(e, FPC_ESTATE, "fpc_search_play_ms: no fpc_search_play has run with fpc_set_timing on");
  *ms_out = e->play_ms;
  return 0;
}

// ------------------------------------------------------------------------------------------------
// RCCL (backend "nccl" on ROCm), bound at run time: the copy PyTorch-ROCm already mapped into the
// process is preferred (one HIP runtime, one RCCL), else the system librccl.so.
#ifndef FPC_EMUL
namespace {
struct Rccl {
  typedef int (*get_id_t)(void *);
  typedef int (*allgather_t)(const void *, void *, size_t, int, void *, hipStream_t);
  typedef int (*destroy_t)(void *);
  typedef const char *(*errstr_t)(int);
  void *h = nullptr;
  destroy_t abort = nullptr;        // ncclCommAbort (optional)
  get_id_t get_id = nullptr;
  void *init_rank = nullptr;
  allgather_t allgather = nullptr;
  destroy_t destroy = nullptr;
  errstr_t errstr = nullptr;
  std::string err;
};
struct Id128 { char b[128]; };    // ncclUniqueId (rccl.h: NCCL_UNIQUE_ID_BYTES 128), passed by value

extern "C++" Rccl &rccl() {
  static Rccl r;
  if (r.h || !r.err.empty()) return r;
  // FPC_RCCL_LIB: the host layer names the copy that belongs to the HIP runtime already in the process
  // (PyTorch-ROCm ships its own librccl.so next to its libamdhip64.so)
  if (const char *env = getenv("FPC_RCCL_LIB")) {
    r.h = dlopen(env, RTLD_NOW | RTLD_GLOBAL);
    if (!r.h) {                                   // an explicit choice: no silent substitute
      const char *de = dlerror();                 // (dlerror() clears the message when read: once per site)
      r.err = std::string("FPC_RCCL_LIB=") + env + " cannot be loaded: " + (de ? de : "");
      return r;
    }
  }
  const char *names[] = {"librccl.so", "librccl.so.1"};
  for (const char *n : names) if (!r.h) r.h = dlopen(n, RTLD_NOW | RTLD_NOLOAD);
  for (const char *n : names) if (!r.h) r.h = dlopen(n, RTLD_NOW | RTLD_GLOBAL);
  if (!r.h) r.h = dlopen("/opt/rocm/lib/librccl.so.1", RTLD_NOW | RTLD_GLOBAL);
  if (!r.h) {
    const char *de = dlerror();
    r.err = std::string("librccl.so not found: ") + (de ? de : "");
    return r;
  }
  r.get_id = (Rccl::get_id_t)dlsym(r.h, "ncclGetUniqueId");
  r.init_rank = dlsym(r.h, "ncclCommInitRank");
  r.allgather = (Rccl::allgather_t)dlsym(r.h, "ncclAllGather");
  r.destroy = (Rccl::destroy_t)dlsym(r.h, "ncclCommDestroy");
  r.errstr = (Rccl::errstr_t)dlsym(r.h, "ncclGetErrorString");
  r.abort = (Rccl::destroy_t)dlsym(r.h, "ncclCommAbort");
  if (!r.get_id || !r.init_rank || !r.allgather || !r.destroy) r.err = "librccl.so lacks ncclGetUniqueId/CommInitRank/AllGather/CommDestroy";
  return r;
}
int comm_fail(fpc_engine *e, const char *what, int rc) {
  Rccl &r = rccl();
  return fail(e, FPC_ECOMM, "%s failed: ncclResult %d (%s)", what, rc, r.errstr ? r.errstr(rc) : "?");
}
}  // namespace
#endif

int fpc_comm_available(void) {
#ifdef FPC_EMUL
  return fail(nullptr, FPC_EUNSUPPORTED, "RCCL exists only in the gfx950 build");
#else
  Rccl &r = rccl();
  return r.err.empty() ? 0 : fail(nullptr, FPC_ECOMM, "%s", r.err.c_str());
#endif
}

int fpc_comm_unique_id(void *id128) {
  if (!id128) return FPC_EINVAL;
#ifdef FPC_EMUL
  return fail(nullptr, FPC_EUNSUPPORTED, "RCCL exists only in the gfx950 build");
#else
  Rccl &r = rccl();
  if (!r.err.empty()) return fail(nullptr, FPC_ECOMM, "%s", r.err.c_str());
  const int rc = r.get_id(id128);
  return rc ? comm_fail(nullptr, "ncclGetUniqueId", rc) : 0;
#endif
}

int fpc_comm_init(fpc_engine *e, const void *id128, int rank, int world) {
  if (!e || !id128 || world < 1 || rank < 0 || rank >= world) return fail(e, FPC_EINVAL, "bad argument");
#ifdef FPC_EMUL
  return fail(e, FPC_EUNSUPPORTED, "RCCL exists only in the gfx950 build");
#else
  USE_DEV(e);
  Rccl &r = rccl();
  if (!r.err.empty()) return fail(e, FPC_ECOMM, "%s", r.err.c_str());
  if (e->comm) return fail(e, FPC_ESTATE, "communicator already initialised");
  Id128 id;
  memcpy(&id, id128, sizeof(id));
  typedef int (*init_fn)(void **, int, Id128, int);
  const int rc = ((init_fn)r.init_rank)(&e->comm, world, id, rank);
  if (rc) { e->comm = nullptr; return comm_fail(e, "ncclCommInitRank", rc); }
  e->comm_rank = rank; e->comm_world = world;
  int rr;
  if (!e->d_gcounts || e->gcounts_world < world) {
    if ((rr = dalloc(e, &e->d_gcounts, 3 * (size_t)world + 4))) return rr;     // zero-filled: epoch 0 is never a fresh record
    e->gcounts_world = world;
  }
  // a new communicator starts at epoch 0 with every record cleared: a word left behind by an earlier communicator
  // must never pass for a fresh one
  e->comm_epoch = 0;
  if (hipMemset(e->d_gcounts, 0, (3 * (size_t)e->gcounts_world + 4) * sizeof(long long)) != hipSuccess) {
    (void)r.destroy(e->comm); e->comm = nullptr;      // local: nobody waits in a collective yet (tuples.init_comm MIN-reduces the verdicts)
    return fail(e, FPC_ENODEVICE, "clearing the exchange records failed");
  }
  e->gather_counts.assign(world, 0);
  return 0;
#endif
}

int fpc_comm_destroy(fpc_engine *e) {
  if (!e) return FPC_EINVAL;
#ifndef FPC_EMUL
  if (e->comm) {
    (void)hipSetDevice(e->cfg.device);
    (void)rccl().destroy(e->comm);
    e->comm = nullptr;
  }
#endif
  return 0;
}

// The episode-end exchange.  What it guarantees: NO LOCAL FAILURE CAN STRAND A PEER.  Every rank that
// enters goes through the same fixed sequence of collectives -- counts, status, payload -- and which of them run depends
// only on values every rank has agreed on, never on a local success:
//   1. counts round: (tuple count, buffer capacity, epoch) per rank.  A rank whose own HIP calls fail on the way in STILL
//      enters the collective; its slot then carries the previous exchange's epoch, which the others recognise;
//   2. status round, ALWAYS (one 8-byte all-gather per episode): 2 * epoch + 1 = "everything up to here worked on this
//      rank" (counts read back, every peer's record fresh, send / receive buffers big enough).  Anything else -- 2 * epoch
//      (failed) or a stale word (the status upload itself failed) -- makes EVERY rank leave before the payload
//      collective, the failing one with its own error, the others with FPC_ECOMM naming the rank.  The protocol stays in
//      lockstep, so the next exchange on the same communicator works (tests/test_comm_two_ranks_gpu.py);
//   3. payload round.
// Two windows cannot be closed by agreement: an error returned by an RCCL call itself, and a failure to read the status
// words back (the rank cannot know whether the others go on).  There the rank aborts its communicator (ncclCommAbort, where
// the library has it) so that peers blocked on it get an error instead of waiting, and returns; fpc_comm_init is needed again.
int fpc_allgather_tuples(fpc_engine *e, int *counts_out, int *total_out) {
  if (!e || !counts_out || !total_out) return fail(e, FPC_EINVAL, "bad argument");
#ifdef FPC_EMUL
  return fail(e, FPC_EUNSUPPORTED, "RCCL exists only in the gfx950 build");
#else
  if (!e->comm) return fail(e, FPC_ESTATE, "fpc_comm_init has not been called");
  USE_DEV(e);
  Rccl &r = rccl();
  const int W = e->comm_world;
  const long long epoch = ++e->comm_epoch;
  int local_rc = 0;
  std::string local_err;
  auto note = [&](int rc) { if (rc && !local_rc) { local_rc = rc; local_err = e->err; } };
  // a test can make one of this function's HIP calls fail (fpc_debug_comm_fault): the call is then NOT made
  auto faulted = [&](int point) -> bool {
    if (e->comm_fault != point) return false;
    e->comm_fault = 0;
    return true;
  };
  auto hip_ok = [&](hipError_t he, const char *what) -> bool {
    if (he == hipSuccess) return true;
    note(fail(e, FPC_ENODEVICE, "fpc_allgather_tuples: %s failed: %s", what, hipGetErrorString(he)));
    return false;
  };
  auto abort_comm = [&](int rc) -> int {      // leave between collectives without agreement: peers must not wait for this rank
    const std::string keep = e->err;
    if (r.abort) (void)r.abort(e->comm); else (void)r.destroy(e->comm);
    e->comm = nullptr;
    e->err = keep + " (communicator aborted: fpc_comm_init is needed again)";
    return rc;
  };
  long long *slot = e->d_gcounts + 3 * (size_t)W;       // this rank's counts record (3 words) ...
  long long *stslot = slot + 3;                          // ... and its status word: a slot of its own, so that what a failed upload
                                                         // leaves there is the PREVIOUS exchange's status word, never a fresh one
  // 1. counts round
  long long mine[3] = {e->tuple_count, std::min<long long>(e->tuple_cap, (long long)(e->gather_cap / (size_t)W)), epoch};
  hip_ok(faulted(1) ? hipErrorUnknown : hipMemcpyAsync(slot, mine, sizeof(mine), hipMemcpyHostToDevice, e->stream), "counts upload");
  int rc = r.allgather(slot, e->d_gcounts, 3, /*ncclInt64*/ 4, e->comm, e->stream);
  if (rc) return abort_comm(comm_fail(e, "ncclAllGather(counts)", rc));
  std::vector<long long> cnt3(3 * (size_t)W, 0), cnt(W, 0);
  if (hip_ok(faulted(2) ? hipErrorUnknown : hipMemcpyAsync(cnt3.data(), e->d_gcounts, cnt3.size() * sizeof(long long), hipMemcpyDeviceToHost, e->stream), "counts read-back"))
    hip_ok(hipStreamSynchronize(e->stream), "counts read-back");
  long long mx = 1;
  if (!local_rc) {
    for (int i = 0; i < W; ++i) {
      if (cnt3[3 * (size_t)i + 2] != epoch || cnt3[3 * (size_t)i] < 0) {
        note(fail(e, FPC_ECOMM, "rank %d sent no fresh counts record for this exchange (its upload failed)", i));
        break;
      }
      cnt[i] = cnt3[3 * (size_t)i];
      mx = std::max(mx, cnt[i]);
    }
  }
  // 1b. room for the padded payload on both sides (every rank knows mx, so each grows its own buffers)
  if (!local_rc && mx > e->tuple_cap) {
    fpc_tuple *bigger = nullptr;
    if (faulted(3)) note(fail(e, FPC_ENOMEM, "fpc_allgather_tuples: growing the tuple send buffer failed (injected)"));
    else note(dalloc(e, &bigger, (size_t)mx));
    if (!local_rc) {
      hipError_t he = hipSuccess;
      if (e->tuple_count) he = hipMemcpyAsync(bigger, e->d_tuples, (size_t)e->tuple_count * sizeof(fpc_tuple), hipMemcpyDeviceToDevice, e->stream);
      if (he == hipSuccess) he = hipStreamSynchronize(e->stream);
      if (!hip_ok(he, "growing the tuple send buffer")) {
        (void)hipFree(bigger);
        e->allocs.erase(std::find(e->allocs.begin(), e->allocs.end(), (void *)bigger));
      } else {
        if (e->d_tuples) { (void)hipFree(e->d_tuples); e->allocs.erase(std::find(e->allocs.begin(), e->allocs.end(), (void *)e->d_tuples)); }
        e->d_tuples = bigger;
        e->tuple_cap = (int)mx;
      }
    }
  }
  const size_t want = (size_t)W * (size_t)mx;           // tuples in the receive buffer (size_t: world x capacity can pass 2^31)
  if (!local_rc && want > e->gather_cap) {
    if (e->d_gather) { (void)hipFree(e->d_gather); e->allocs.erase(std::find(e->allocs.begin(), e->allocs.end(), (void *)e->d_gather)); e->d_gather = nullptr; }
    e->gather_cap = 0;
    note(dalloc(e, &e->d_gather, want));
    if (!local_rc) e->gather_cap = want;
  }
  // 2. status round -- always
  const long long good = 2 * epoch + 1;
  long long st = local_rc == 0 ? good : 2 * epoch;
  std::vector<long long> sts(W, 0);
  hip_ok(faulted(4) ? hipErrorUnknown : hipMemcpyAsync(stslot, &st, sizeof(st), hipMemcpyHostToDevice, e->stream), "status upload");   // failed: the slot keeps a stale word
  rc = r.allgather(stslot, e->d_gcounts, 1, /*ncclInt64*/ 4, e->comm, e->stream);
  if (rc) return abort_comm(comm_fail(e, "ncclAllGather(status)", rc));
  const int before = local_rc;
  if (hip_ok(faulted(5) ? hipErrorUnknown : hipMemcpyAsync(sts.data(), e->d_gcounts, (size_t)W * sizeof(long long), hipMemcpyDeviceToHost, e->stream), "status read-back"))
    hip_ok(hipStreamSynchronize(e->stream), "status read-back");
  if (local_rc && !before) { e->err = local_err; return abort_comm(local_rc); }     // said "good", cannot see what the others said
  if (local_rc) { e->err = local_err; return local_rc; }                              // the others saw this rank's word: nobody goes on
  for (int i = 0; i < W; ++i)
    if (sts[i] != good) return fail(e, FPC_ECOMM, "rank %d reported a failure before the payload collective; no rank entered it", i);
  // 3. payload, padded to the largest count: ONE collective per episode (latency-bound)
  e->gather_stride = (int)mx;
  rc = r.allgather(e->d_tuples, e->d_gather, (size_t)mx * sizeof(fpc_tuple), /*ncclUint8*/ 1, e->comm, e->stream);
  if (rc) return abort_comm(comm_fail(e, "ncclAllGather(tuples)", rc));
  HIPCHK(e, hipStreamSynchronize(e->stream));            // behind the last collective: nobody waits for this rank any more
  int total = 0;
  for (int i = 0; i < W; ++i) { e->gather_counts[i] = (int)cnt[i]; counts_out[i] = (int)cnt[i]; total += (int)cnt[i]; }
  *total_out = total;
  return 0;
#endif
}

// TEST HOOK: the next fpc_allgather_tuples on this engine treats one of its own HIP calls as failed --
// 1 counts upload, 2 counts read-back, 3 send-buffer growth, 4 status upload, 5 status read-back (0 = none).
int fpc_debug_comm_fault(fpc_engine *e, int point) {
  if (!e || point < 0 || point > 5) return fail(e, FPC_EINVAL, "bad argument");
  e->comm_fault = point;
  return 0;
}

int fpc_gathered_read(fpc_engine *e, fpc_tuple *host_out, int first, int n) {
  if (!e || !host_out || first < 0 || n < 0) return fail(e, FPC_EINVAL, "bad argument");
#ifdef FPC_EMUL
  return fail(e, FPC_EUNSUPPORTED, "RCCL exists only in the gfx950 build");
#else
  if (!e->d_gather) return fail(e, FPC_ESTATE, "fpc_allgather_tuples has not been called");
  USE_DEV(e);
  // logical index -> (rank, local index): ranks are stored max-padded
  int r = 0, base = 0, i = first, left = n;
  fpc_tuple *dst = host_out;
  while (left > 0) {
    while (r < e->comm_world && i >= base + e->gather_counts[r]) { base += e->gather_counts[r]; ++r; }
    if (r >= e->comm_world) return fail(e, FPC_EINVAL, "gathered tuple range out of bounds");
    const int loc = i - base, take = std::min(left, e->gather_counts[r] - loc);
    HIPCHK(e, hipMemcpyAsync(dst, e->d_gather + (size_t)r * e->gather_stride + loc, (size_t)take * sizeof(fpc_tuple), hipMemcpyDeviceToHost, e->stream));
    dst += take; i += take; left -= take;
  }
  HIPCHK(e, hipStreamSynchronize(e->stream));
  return 0;
#endif
}

int fpc_stats_get(fpc_engine *e, fpc_stats *out) {
  if (!e || !out) return FPC_EINVAL;
  *out = e->stats;
  return 0;
}
int fpc_stats_reset(fpc_engine *e) {
  if (!e) return FPC_EINVAL;
  e->stats = fpc_stats{};
  return 0;
}
int fpc_set_policy_mode(fpc_engine *e, int mode) {
  if (!e || (mode != FPC_POLICY_FULL && mode != FPC_POLICY_LEGAL)) return fail(e, FPC_EINVAL, "bad policy mode");
  e->policy_mode = mode;
  return 0;
}

// fpc_set_rules keeps the range it always had (0..31); the sets with FPC_RULES_VISITS come in through fpc_set_rule_bits
static int set_rules_upto(fpc_engine *e, int rules, int top);
int fpc_set_rules(fpc_engine *e, int rules) { return set_rules_upto(e, rules, FPC_RULES_TRAINING); }
int fpc_set_rule_bits(fpc_engine *e, int rules) { return set_rules_upto(e, rules, FPC_RULES_SELFPLAY); }

static int set_rules_upto(fpc_engine *e, int rules, int top) {
  if (!e || rules < 0 || rules > top) return fail(e, FPC_EINVAL, "bad rule set");
  if (e->searching && rules != e->dc.rules) e->searching = false;     // a search in flight was started under the other rules
  e->dc.rules = rules;
  e->t.born = born_visits(rules);
#ifndef FPC_EMUL
  e->nn.dc.rules = rules;
#endif
  return 0;
}

int fpc_search_set_root_noise(fpc_engine *e, const float *gamma, int n_games, float eps) {
  if (!e) return FPC_EINVAL;
  USE_DEV(e);
  if (!gamma) { e->t.noise = nullptr; e->t.noise_eps = 0.f; e->noise_n = 0; return 0; }
  if (n_games < 1 || n_games > e->cfg.max_games || !(eps >= 0.f && eps <= 1.f)) return fail(e, FPC_EINVAL, "bad root-noise arguments");
  int r;
  if (!e->d_noise && (r = dalloc(e, &e->d_noise, (size_t)e->cfg.max_games * FPC_MAX_MOVES))) return r;
  HIPCHK(e, hipMemcpyAsync(e->d_noise, gamma, (size_t)n_games * FPC_MAX_MOVES * sizeof(float), hipMemcpyHostToDevice, e->stream));
  HIPCHK(e, hipStreamSynchronize(e->stream));
  e->t.noise = e->d_noise;
  e->t.noise_eps = eps;
  e->noise_n = n_games;
  return 0;
}

int fpc_set_timing(fpc_engine *e, int enabled) {
  if (!e) return FPC_EINVAL;
  e->timing = enabled != 0;
  return 0;
}
int fpc_set_fc_weight_type(fpc_engine *e, int type) {
  if (!e || (type != FPC_FC_W16 && type != FPC_FC_W8)) return fail(e, FPC_EINVAL, "fpc_set_fc_weight_type: type must be FPC_FC_W16 or FPC_FC_W8");
  e->fc_wtype = type;
  return 0;
}
const char *fpc_nn_fc_kernel(fpc_engine *e) {
#ifdef FPC_EMUL
  (void)e;
  return "";
#else
  if (!e || !e->nn.loaded) return "";
  return e->nn.fc_wtype ? "k_fcw8" : e->nn.fc_layout == 2 ? "k_fcw" : "k_fc16";
#endif
}
const char *fpc_nn_kernel(fpc_engine *e) {
#ifdef FPC_EMUL
  (void)e;
  return "";
#else
  if (!e || !e->nn.loaded) return "";
  return e->nn.use_towerw ? "k_towerw" : e->nn.use_tower ? (e->nn.tower_compact && e->nn.tower_waves == 8 && e->dc.R == 14 ? "k_towerc" : "k_tower") : "k_conv3x3";
#endif
}
void *fpc_stream(fpc_engine *e) { return e ? (void *)e->stream : nullptr; }

int fpc_memory_is_host(void) {
#ifdef FPC_EMUL
  return 1;
#else
  return 0;
#endif
}

#ifdef FPC_TREE_STAMPS
// diagnostic builds only (tools/tree_stamps.py): the s_memtime stamps the tree kernels left for game FPC_TREE_STAMPS
int fpc_debug_tree_stamps(unsigned long long *out32) {
  return hipMemcpyFromSymbol(out32, HIP_SYMBOL(fpc::g_tree_stamps), 32 * sizeof(unsigned long long)) == hipSuccess ? 0 : FPC_ENODEVICE;
}
#endif

}  // extern "C"

// ------------------------------------------------------------------------------------------------
// device-side weight pack (fpc_pack.h)
namespace {

int pack_cus() {
#ifdef FPC_EMUL
  return 256;
#else
  return fpc::NN::device_cus();
#endif
}

// the geometry a network of this width and depth packs into on this engine's board: fc_layout 0 chooses as
// weights.default_fc_layout does; shapes fpc_load_weights refuses are refused with its messages
int pack_geom_from(fpc_engine *e, int hidden, int nblocks, int fc_layout, PackGeom *g, const char *fn) {
  if (fc_layout < 0 || fc_layout > 2) return fail(e, FPC_EINVAL, "%s: fc_layout must be 0 (default), 1 (k_fc16) or 2 (k_fcw)", fn);
  const int A = e->dc.A;
  g->R = e->dc.R; g->RR = e->dc.RR; g->A = A; g->A_ch = e->dc.A_ch; g->F = hidden; g->nblocks = nblocks; g->dtype = e->cfg.nn_dtype ? 1 : 0;
  g->Fp = (hidden + 127) / 128 * 128;
  g->Kp = (A + 511) / 512 * 512;
  if (fc_layout == 0) fc_layout = pk_plan_fcw((A + PK_FCW_COLS - 1) / PK_FCW_COLS * PK_FCW_COLS, g->Kp, pack_cus()) ? 2 : 1;
  g->fc_layout = fc_layout;
  g->fc_wtype = e->fc_wtype;
  const int gw = fc_layout == 2 ? PK_FCW_COLS : 256;
  g->Np = (A + gw - 1) / gw * gw;
  return pk_check_geom(g->F, g->nblocks, g->Np, g->Kp, g->fc_layout, g->fc_wtype, g->dtype, A, pack_cus(), &g->fcw_split, &e->err);
}

// convolution i of the descriptor in blob order: stem, c1[0], c2[0], ..., policy, value
const fpc_conv_src &conv_at(const fpc_net_src *s, int i) {
  if (i == 0) return s->stem;
  if (i <= 2 * s->nblocks) return (i - 1) & 1 ? s->c2[(i - 1) / 2] : s->c1[(i - 1) / 2];
  return i == 2 * s->nblocks + 1 ? s->pconv : s->vconv;
}

// argument checks and the geometry of the packed network; nothing is launched
int pack_geom(fpc_engine *e, const fpc_net_src *s, int fc_layout, PackGeom *g, const char *fn) {
  if (!s) return fail(e, FPC_EINVAL, "%s: null descriptor", fn);
  if (e->dc.A_ch > PK_MAXCH || e->dc.A_ch % 8) return fail(e, FPC_EINVAL, "%s: board too large for k_pack_fc's tile", fn);
  auto conv_ok = [](const fpc_conv_src &c) { return c.w && c.bn_weight && c.bn_bias && c.bn_mean && c.bn_var; };
  bool ptrs = conv_ok(s->stem) && conv_ok(s->pconv) && conv_ok(s->vconv) && s->fc_w && s->fc_b && s->vfc_w && s->vfc_b;
  if (s->nblocks > 0 && (!s->c1 || !s->c2)) ptrs = false;
  for (int i = 0; ptrs && i < s->nblocks; ++i) ptrs = conv_ok(s->c1[i]) && conv_ok(s->c2[i]);
  if (!ptrs) return fail(e, FPC_EINVAL, "%s: null parameter pointer in the descriptor", fn);
  const int rc = pack_geom_from(e, s->hidden, s->nblocks, fc_layout, g, fn);
  if (rc) return rc;
  for (int i = 0; i < g->nconv(); ++i) {
    const fpc_conv_src &c = conv_at(s, i);
    int cin, cout, cin_pad, cout_pad;
    g->conv_dims(i, &cin, &cout, &cin_pad, &cout_pad);
    if (c.cin != cin || c.cout != cout)
      return fail(e, FPC_EINVAL, "%s: convolution %d of the descriptor is %d -> %d channels, this board and hidden width need %d -> %d", fn, i, c.cin, c.cout, cin, cout);
  }
  return 0;
}

// room for the descriptors of `nconv` convolutions (networks of more than 64 blocks: the table grows once)
int pack_ensure_tab(fpc_engine *e, int nconv) {
  if (nconv <= e->pack_tab_convs) return 0;
  unsigned char *grown = nullptr;
  int r;
  if ((r = dalloc(e, &grown, (size_t)nconv * sizeof(PackConv) + 16))) return r;
  (void)hipFree(e->d_pack_tab);
  e->allocs.erase(std::find(e->allocs.begin(), e->allocs.end(), (void *)e->d_pack_tab));
  e->d_pack_tab = grown;
  e->pack_tab_convs = nconv;
  return 0;
}

// int8 policy Linear, first pass (k_fc_rowmax): the row scales into the engine's scratch row and the non-finite flag to
// the host.  Runs BEFORE anything is written to a blob or to the live network: a non-finite weight refuses the pack.
int pack_fc8_scan(fpc_engine *e, const fpc_net_src *s, const PackGeom &g, const char *fn) {
  if (!g.fc_wtype) return 0;
  int r;
  if (e->fc8_scale_n < g.Np) {
    float *grown = nullptr;
    if ((r = dalloc(e, &grown, (size_t)g.Np + 16))) return r;
    if (e->d_fc8_scale) {
      (void)hipFree(e->d_fc8_scale);
      e->allocs.erase(std::find(e->allocs.begin(), e->allocs.end(), (void *)e->d_fc8_scale));
    }
    e->d_fc8_scale = grown;
    e->fc8_scale_n = g.Np;
  }
  int *flag = reinterpret_cast<int *>(e->d_fc8_scale + g.Np);
  int bad = 0;
  HIPCHK(e, hipMemcpyAsync(flag, &bad, sizeof(int), hipMemcpyHostToDevice, e->stream));
  FPC_LAUNCH(k_fc_rowmax, g.Np, PK_THREADS, e->stream, s->fc_w, g.A, e->d_fc8_scale, flag);
  HIPCHK(e, hipGetLastError());
  HIPCHK(e, hipMemcpyAsync(&bad, flag, sizeof(int), hipMemcpyDeviceToHost, e->stream));
  HIPCHK(e, hipStreamSynchronize(e->stream));
  if (bad) return fail(e, FPC_EWEIGHTS, "%s: the policy Linear holds a non-finite weight: int8 export refused, nothing was written", fn);
  return 0;
}

// launches the three pack kernels on the engine's stream (timed if fpc_set_timing is on); the caller synchronises
int pack_launch(fpc_engine *e, const fpc_net_src *s, const PackGeom &g, const PackDst &d) {
  const int nconv = g.nconv();
  if (nconv > e->pack_tab_convs) return fail(e, FPC_ESTATE, "descriptor table too small");
  std::vector<PackConv> tab((size_t)nconv);
  int max_items = 0;
  for (int i = 0; i < nconv; ++i) {
    const fpc_conv_src &c = conv_at(s, i);
    PackConv &t = tab[(size_t)i];
    t.w = c.w; t.b = c.b; t.g = c.bn_weight; t.beta = c.bn_bias; t.mean = c.bn_mean; t.var = c.bn_var; t.eps = c.eps;
    g.conv_dims(i, &t.cin, &t.cout, &t.cin_pad, &t.cout_pad);
    t.w16 = d.cw[(size_t)i]; t.b32 = d.cb[(size_t)i];
    max_items = std::max(max_items, 9 * t.cout_pad * (t.cin_pad / 8));
  }
  HIPCHK(e, hipMemcpyAsync(e->d_pack_tab, tab.data(), tab.size() * sizeof(PackConv), hipMemcpyHostToDevice, e->stream));
  HIPCHK(e, hipStreamSynchronize(e->stream));      // `tab` is pageable host memory about to go out of scope
  if (e->timing && !e->pk_ev[0]) {
    HIPCHK(e, hipEventCreate(&e->pk_ev[0]));
    HIPCHK(e, hipEventCreate(&e->pk_ev[1]));
  }
  if (e->timing) HIPCHK(e, hipEventRecord(e->pk_ev[0], e->stream));
  const int bpc = std::min(64, (max_items + PK_THREADS - 1) / PK_THREADS);
  FPC_LAUNCH(k_pack_conv, nconv * bpc, PK_THREADS, e->stream, (const PackConv *)e->d_pack_tab, bpc, g.dtype);
  const int nchunks = (g.RR + PK_PC - 1) / PK_PC;
  if (g.fc_wtype)       // the scales: pack_fc8_scan left them in the scratch row
    FPC_LAUNCH(k_pack_fc8, (g.Np / PK_ROWS8) * nchunks, PK_THREADS, e->stream, s->fc_w, (const float *)e->d_fc8_scale, g.A, g.A_ch, g.RR, g.Np, g.Kp,
               reinterpret_cast<unsigned char *>(d.fcw), d.fcs);
  else
    FPC_LAUNCH(k_pack_fc, (g.Np / 16) * nchunks, PK_THREADS, e->stream, s->fc_w, g.A, g.A_ch, g.RR, g.Np, g.Kp, g.dtype, d.fcw);
  const int mblk = std::min(64, (g.Np + g.RR * 32 + PK_THREADS) / PK_THREADS);
  FPC_LAUNCH(k_pack_misc, mblk, PK_THREADS, e->stream, s->fc_b, s->vfc_w, s->vfc_b, g.A, g.RR, g.Np, mblk, d.fcb, d.vw, d.vb);
  HIPCHK(e, hipGetLastError());
  if (e->timing) HIPCHK(e, hipEventRecord(e->pk_ev[1], e->stream));
  return 0;
}

int pack_finish_timing(fpc_engine *e) {
  e->pack_ms = -1.f;
  if (e->timing) HIPCHK(e, hipEventElapsedTime(&e->pack_ms, e->pk_ev[0], e->pk_ev[1]));
  return 0;
}

}  // namespace

extern "C" {

int fpc_weights_blob_size(const fpc_engine *ce, int hidden, int nblocks, int fc_layout, uint64_t *nbytes) {
  fpc_engine *e = const_cast<fpc_engine *>(ce);
  if (!e || !nbytes) return fail(e, FPC_EINVAL, "fpc_weights_blob_size: null argument");
  USE_DEV(e);
  PackGeom g;
  const int rc = pack_geom_from(e, hidden, nblocks, fc_layout, &g, "fpc_weights_blob_size");
  if (rc) return rc;
  *nbytes = pk_blob_layout(g, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr);
  return 0;
}

int fpc_weights_pack(fpc_engine *e, const fpc_net_src *src, int fc_layout, void *blob_dev, uint64_t cap, uint64_t *nbytes) {
  if (!e || !blob_dev) return fail(e, FPC_EINVAL, "fpc_weights_pack: null argument");
  if ((uintptr_t)blob_dev & 15) return fail(e, FPC_EINVAL, "fpc_weights_pack: blob_dev must be 16-byte aligned");
  USE_DEV(e);
  PackGeom g;
  int r;
  if ((r = pack_geom(e, src, fc_layout, &g, "fpc_weights_pack"))) return r;
  std::vector<uint64_t> cw, cb;
  uint64_t fcw, fcb, vw, vb, fcs;
  const uint64_t total = pk_blob_layout(g, &cw, &cb, &fcw, &fcb, &vw, &vb, &fcs);
  if (cap < total) return fail(e, FPC_EINVAL, "fpc_weights_pack: the blob needs %llu bytes, cap is %llu", (unsigned long long)total, (unsigned long long)cap);
  unsigned char *base = (unsigned char *)blob_dev;
  PackDst d;
  for (size_t i = 0; i < cw.size(); ++i) { d.cw.push_back((uint16_t *)(base + cw[i])); d.cb.push_back((float *)(base + cb[i])); }
  d.fcw = (uint16_t *)(base + fcw); d.fcb = (float *)(base + fcb); d.vw = (float *)(base + vw); d.vb = (float *)(base + vb);
  d.fcs = g.fc_wtype ? (float *)(base + fcs) : nullptr;
  if ((r = pack_ensure_tab(e, g.nconv()))) return r;
  if ((r = pack_fc8_scan(e, src, g, "fpc_weights_pack"))) return r;      // the last thing that can fail before something is written
  int32_t hdr[16] = {0, 3 + g.fc_wtype, g.R, g.F, g.nblocks, g.dtype, g.A_ch, g.Np, g.Kp, g.fc_layout, g.fc_wtype, 0, 0, 0, 0, 0};
  memcpy(hdr, "FPCW", 4);
  HIPCHK(e, hipMemcpyAsync(base, hdr, sizeof(hdr), hipMemcpyHostToDevice, e->stream));
  if ((r = pack_launch(e, src, g, d))) return r;
  HIPCHK(e, hipStreamSynchronize(e->stream));
  if ((r = pack_finish_timing(e))) return r;
  if (nbytes) *nbytes = total;
  return 0;
}

int fpc_load_weights_device(fpc_engine *e, const fpc_net_src *src, int fc_layout) {
  if (!e) return fail(e, FPC_EINVAL, "fpc_load_weights_device: null engine");
  USE_DEV(e);
  PackGeom g;
  int r;
  if ((r = pack_geom(e, src, fc_layout, &g, "fpc_load_weights_device"))) return r;
#ifdef FPC_EMUL
  return fail(e, FPC_EWEIGHTS, "the internal ResNet exists only in the gfx950 build");
#else
  fpc::NN &nn = e->nn;
  if ((r = pack_ensure_tab(e, g.nconv()))) return r;
  if ((r = pack_fc8_scan(e, src, g, "fpc_load_weights_device"))) return r;
  // same geometry (the weight type included): straight into the live allocations, nothing freed or allocated; else allocate as fpc_load_weights does
  if (!nn.same_geom(g.F, g.nblocks, g.Np, g.Kp, g.fc_layout, g.fc_wtype) && (r = nn.alloc_net(g.F, g.nblocks, g.Np, g.Kp, g.fc_layout, g.fc_wtype, g.fcw_split, &e->err))) return r;
  PackDst d;
  for (fpc::ConvW *cw : nn.convs_in_blob_order()) { d.cw.push_back(cw->w); d.cb.push_back(cw->b); }
  d.fcw = nn.fcw; d.fcb = nn.fcb; d.vw = nn.vw; d.fcs = nn.fcs;
  d.vb = (float *)(e->d_pack_tab + (size_t)e->pack_tab_convs * sizeof(PackConv));
  nn.loaded = false;      // the live weights are about to be rewritten: a HIP failure on the way leaves no half-new network in use
  if ((r = pack_launch(e, src, g, d))) return r;
  HIPCHK(e, hipMemcpyAsync(&nn.vb, d.vb, 4, hipMemcpyDeviceToHost, e->stream));
  HIPCHK(e, hipStreamSynchronize(e->stream));
  if ((r = pack_finish_timing(e))) return r;
  return nn.finish_weights(&e->err);
#endif
}

int fpc_weights_pack_ms(fpc_engine *e, float *ms_out) {
  if (!e || !ms_out) return fail(e, FPC_EINVAL, "bad argument");
  if (e->pack_ms < 0.f) return fail(e, FPC_ESTATE, "fpc_weights_pack_ms: no weight pack has run with fpc_set_timing on");
  *ms_out = e->pack_ms;
  return 0;
}

}  // extern "C"
