"""ctypes binding of the C-ABI in include/fpc_engine.h (libfpc_engine.so, built by hipcc for gfx950).

There is no CPU implementation behind this module: if the HIP library is missing or no GPU is
visible, loading / Engine() raises.  Everything above this file (alphazero_cpp.py, mcts.py,
four_player_chess_board.py) is the Python mirror of the reference's binding surface.
"""
import ctypes as C
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
# FPC_ENGINE_LIB: developer knob for A/B timing of two builds of the same engine (tools/ab.sh)
LIB_PATH = os.environ.get("FPC_ENGINE_LIB") or os.path.join(HERE, "csrc", "libfpc_engine.so")

MAX_SQ, MAX_PL, NO_SQ, MAX_MOVES = 196, 16, 255, 256
MAX_LEAVES = 8                          # FPC_MAX_LEAVES: leaves per game per step of a leaf-parallel search
REPLAY_RINGS, REPLAY_SCRATCH, REPLAY_COLLECTED, REPLAY_GATHERED = 2, 2, 0, 1     # FPC_REPLAY_*: ring 0 experience, 1 validation
RULES_STRICT, RULES_PUCT, RULES_ROTATION, RULES_PLANES, RULES_FULL_MOVES, RULES_FIXED = 0, 1, 2, 4, 8, 15
RULES_TERMINAL, RULES_TRAINING = 16, 31   # Q5 + the terminal value (search past terminal leaves, value by result); FIXED | TERMINAL
RULES_VISITS, RULES_SELFPLAY = 32, 63     # Q1: N counts backups, every node is born with N = 0; TRAINING | VISITS
PROOF_UNKNOWN, PROOF_WIN, PROOF_LOSS, PROOF_DRAW = 0, 1, 2, 3      # fpc_search_proofs: a node's status, from its own side to move
FPU_ZERO, FPU_PARENT = 0, 1               # fpc_search_set_fpu: q of an unvisited child (PUCT): 0, or the parent's Q - reduction


class Board(C.Structure):
    """fpc_board: the 288-byte POD position (include/fpc_engine.h)."""
    _fields_ = [("sq", C.c_uint8 * MAX_SQ), ("pl", (C.c_uint8 * MAX_PL) * 4), ("plen", C.c_uint8 * 4),
                ("king", C.c_uint8 * 4), ("castle", C.c_uint8 * 4), ("turn", C.c_uint8), ("pad", C.c_uint8 * 15)]


assert C.sizeof(Board) == 288


class Move(C.Structure):
    _fields_ = [("frm", C.c_uint8), ("to", C.c_uint8), ("capture", C.c_uint8), ("promo", C.c_uint8),
                ("flat", C.c_uint16), ("pad", C.c_uint16)]


class Config(C.Structure):
    _fields_ = [("board_size", C.c_int), ("invalid_area", C.c_int), ("max_games", C.c_int), ("max_sims", C.c_int),
                ("avg_children", C.c_int), ("device", C.c_int), ("nn_dtype", C.c_int)]


class Stats(C.Structure):
    _fields_ = [("ms_select", C.c_double), ("ms_tower", C.c_double), ("ms_fc", C.c_double), ("ms_expand", C.c_double),
                ("launches_select", C.c_uint64), ("launches_nn", C.c_uint64), ("launches_expand", C.c_uint64),
                ("sims", C.c_uint64), ("nodes", C.c_uint64)]


MAX_TUPLE_C = 256
TUPLE_FAST = 1          # fpc_tuple::flags bit: the record comes from a fast search (fpc_search_set_fast_rows)


class Tuple(C.Structure):
    """fpc_tuple: one (state, pi, z) training record, 1280 bytes (include/fpc_engine.h)."""
    _fields_ = [("sq", C.c_uint8 * MAX_SQ), ("turn", C.c_uint8), ("flags", C.c_uint8), ("n", C.c_uint16), ("z", C.c_float),
                ("game", C.c_int32), ("ply", C.c_int32), ("flat", C.c_uint16 * MAX_TUPLE_C), ("visits", C.c_uint16 * MAX_TUPLE_C),
                ("pad1", C.c_uint8 * 44)]


assert C.sizeof(Tuple) == 1280

P = C.POINTER


class ConvSrc(C.Structure):
    """fpc_conv_src: one Conv2d(3x3) + BatchNorm2d of the live module, fp32 device pointers (include/fpc_engine.h)."""
    _fields_ = [("w", P(C.c_float)), ("b", P(C.c_float)), ("bn_weight", P(C.c_float)), ("bn_bias", P(C.c_float)),
                ("bn_mean", P(C.c_float)), ("bn_var", P(C.c_float)), ("eps", C.c_float), ("cin", C.c_int), ("cout", C.c_int)]


class NetSrc(C.Structure):
    """fpc_net_src: what the device-side weight pack reads (built by weights.net_src)."""
    _fields_ = [("hidden", C.c_int), ("nblocks", C.c_int), ("stem", ConvSrc), ("pconv", ConvSrc), ("vconv", ConvSrc),
                ("c1", P(ConvSrc)), ("c2", P(ConvSrc)), ("fc_w", P(C.c_float)), ("fc_b", P(C.c_float)),
                ("vfc_w", P(C.c_float)), ("vfc_b", P(C.c_float))]


BOARD_BYTES = C.sizeof(Board)
TURN_OFFSET = Board.turn.offset          # byte of a POD row that holds the side to move


def _bp(pods):
    """Board* over a C-contiguous [n, 288] uint8 array"""
    return C.cast(pods.ctypes.data, P(Board))


def pods_of(boards):
    """list of Board -> [n, 288] uint8 array (copy)"""
    out = np.zeros((len(boards), BOARD_BYTES), np.uint8)
    for i, b in enumerate(boards):
        C.memmove(out[i].ctypes.data, C.byref(b), BOARD_BYTES)
    return out


def board_of(row):
    """one [288] uint8 row -> Board (copy)"""
    b = Board()
    C.memmove(C.byref(b), row.ctypes.data, BOARD_BYTES)
    return b


class _LazyBoards:
    """search_results()["boards"]: Board objects made when indexed (a search returns hundreds of roots; most callers
    read none of them as objects)"""

    def __init__(self, pods):
        self._pods = pods

    def __len__(self):
        return self._pods.shape[0]

    def __getitem__(self, g):
        return board_of(self._pods[g])

    def __iter__(self):
        return (board_of(self._pods[g]) for g in range(self._pods.shape[0]))


_SIGS = {
    "fpc_abi_version": (C.c_int, []),
    "fpc_create": (C.c_int, [P(Config), P(C.c_void_p)]),
    "fpc_destroy": (None, [C.c_void_p]),
    "fpc_last_error": (C.c_char_p, [C.c_void_p]),
    "fpc_num_action_channels": (C.c_int, [C.c_int]),
    "fpc_action_space_size": (C.c_int, [C.c_int]),
    "fpc_is_legal_location": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int]),
    "fpc_move_flat_index": (C.c_int, [C.c_int, C.c_int, C.c_int]),
    "fpc_flat_to_move": (C.c_int, [C.c_int, C.c_int, P(C.c_int), P(C.c_int)]),
    "fpc_board_from_dict": (C.c_int, [P(Board), C.c_int, C.c_int, P(C.c_uint8), P(C.c_uint8), C.c_int, P(C.c_uint8)]),
    "fpc_board_heuristic": (C.c_int, [P(Board), C.c_int]),
    "fpc_boards_legal_moves": (C.c_int, [C.c_void_p, P(Board), C.c_int, P(Move), P(C.c_int)]),
    "fpc_boards_game_result": (C.c_int, [C.c_void_p, P(Board), C.c_int, P(C.c_int), P(C.c_int)]),
    "fpc_boards_take_action": (C.c_int, [C.c_void_p, P(Board), P(C.c_int), C.c_int, P(Board)]),
    "fpc_boards_encode": (C.c_int, [C.c_void_p, P(Board), C.c_int, C.c_void_p]),
    "fpc_boards_legal_mask": (C.c_int, [C.c_void_p, P(Board), C.c_int, C.c_void_p]),
    "fpc_search_begin": (C.c_int, [C.c_void_p, P(Board), C.c_int, C.c_double]),
    "fpc_search_select": (C.c_int, [C.c_void_p, P(C.c_int), P(C.c_void_p)]),
    "fpc_search_expand": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p]),
    "fpc_search_expand_select": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, P(C.c_int), P(C.c_void_p)]),
    "fpc_search_run": (C.c_int, [C.c_void_p, C.c_int]),
    "fpc_search_results": (C.c_int, [C.c_void_p, P(Board), C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p,
                                     C.c_void_p, C.c_void_p, C.c_void_p]),
    "fpc_search_advance": (C.c_int, [C.c_void_p, P(C.c_int), P(C.c_int), C.c_int, P(Board), P(C.c_int)]),
    "fpc_search_advance_refill": (C.c_int, [C.c_void_p, P(C.c_int), P(C.c_int), P(Board), C.c_int, P(Board), P(C.c_int)]),
    "fpc_search_set_budget": (C.c_int, [C.c_void_p, P(C.c_int), C.c_int]),
    "fpc_search_set_fast_rows": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int]),
    "fpc_search_play": (C.c_int, [C.c_void_p, C.c_double, P(C.c_double), P(C.c_int), P(C.c_int), P(Board)]),
    "fpc_search_play_ms": (C.c_int, [C.c_void_p, P(C.c_float)]),
    "fpc_search_grandchildren": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, P(C.c_int), C.c_void_p, C.c_void_p]),
    "fpc_load_weights": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64]),
    "fpc_nn_forward": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]),
    "fpc_weights_blob_size": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, P(C.c_uint64)]),
    "fpc_weights_pack": (C.c_int, [C.c_void_p, P(NetSrc), C.c_int, C.c_void_p, C.c_uint64, P(C.c_uint64)]),
    "fpc_load_weights_device": (C.c_int, [C.c_void_p, P(NetSrc), C.c_int]),
    "fpc_weights_pack_ms": (C.c_int, [C.c_void_p, P(C.c_float)]),
    "fpc_stats_get": (C.c_int, [C.c_void_p, P(Stats)]),
    "fpc_stats_reset": (C.c_int, [C.c_void_p]),
    "fpc_set_timing": (C.c_int, [C.c_void_p, C.c_int]),
    "fpc_set_policy_mode": (C.c_int, [C.c_void_p, C.c_int]),
    "fpc_stream": (C.c_void_p, [C.c_void_p]),
    "fpc_memory_is_host": (C.c_int, []),
    "fpc_set_rules": (C.c_int, [C.c_void_p, C.c_int]),
    "fpc_set_rule_bits": (C.c_int, [C.c_void_p, C.c_int]),
    "fpc_search_set_root_noise": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_float]),
    "fpc_search_set_leaves": (C.c_int, [C.c_void_p, C.c_int, C.c_double]),
    "fpc_search_set_live_rows": (C.c_int, [C.c_void_p, C.c_int]),
    "fpc_search_set_fpu": (C.c_int, [C.c_void_p, C.c_int, C.c_double]),
    "fpc_search_set_solver": (C.c_int, [C.c_void_p, C.c_int]),
    "fpc_search_proofs": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]),
    "fpc_search_set_forced": (C.c_int, [C.c_void_p, C.c_double]),
    "fpc_search_targets": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p]),
    "fpc_tuples_reserve": (C.c_int, [C.c_void_p, C.c_int]),
    "fpc_tuples_reset": (C.c_int, [C.c_void_p]),
    "fpc_collect_tuples": (C.c_int, [C.c_void_p, P(C.c_int), C.c_int]),
    "fpc_tuples_set_z": (C.c_int, [C.c_void_p, P(C.c_int), P(C.c_float), P(C.c_float), C.c_int]),
    "fpc_tuples_count": (C.c_int, [C.c_void_p]),
    "fpc_tuples_read": (C.c_int, [C.c_void_p, P(Tuple), C.c_int, C.c_int]),
    "fpc_comm_unique_id": (C.c_int, [C.c_void_p]),
    "fpc_comm_init": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int]),
    "fpc_comm_destroy": (C.c_int, [C.c_void_p]),
    "fpc_comm_available": (C.c_int, []),
    "fpc_nn_kernel": (C.c_char_p, [C.c_void_p]),
    "fpc_set_fc_weight_type": (C.c_int, [C.c_void_p, C.c_int]),
    "fpc_nn_fc_kernel": (C.c_char_p, [C.c_void_p]),
    "fpc_allgather_tuples": (C.c_int, [C.c_void_p, P(C.c_int), P(C.c_int)]),
    "fpc_debug_comm_fault": (C.c_int, [C.c_void_p, C.c_int]),
    "fpc_boards_attack_maps": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]),
    "fpc_gathered_read": (C.c_int, [C.c_void_p, P(Tuple), C.c_int, C.c_int]),
    "fpc_replay_reserve": (C.c_int, [C.c_void_p, C.c_int, C.c_int]),
    "fpc_replay_push": (C.c_int, [C.c_void_p, C.c_int, P(C.c_int), P(C.c_int8), C.c_int]),
    "fpc_replay_load": (C.c_int, [C.c_void_p, C.c_int, P(Tuple), C.c_int]),
    "fpc_replay_size": (C.c_int, [C.c_void_p, C.c_int]),
    "fpc_replay_read": (C.c_int, [C.c_void_p, C.c_int, P(Tuple), C.c_int, C.c_int]),
    "fpc_replay_batch": (C.c_int, [C.c_void_p, C.c_int, P(C.c_int), C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
    "fpc_replay_batch_w": (C.c_int, [C.c_void_p, C.c_int, P(C.c_int), C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "fpc_replay_decode_ms": (C.c_int, [C.c_void_p, P(C.c_float)]),
}
EXPORTS = sorted(_SIGS)


def bind(cdll):
    for name, (res, args) in _SIGS.items():
        fn = getattr(cdll, name)     # AttributeError if the library does not export it
        fn.restype = res
        fn.argtypes = args
    return cdll


_lib = None


def _check_fresh():
    """The in-tree library must have been built from the sources that lie beside it (__graft_entry__.build() stores
    their content hash): a stale engine must not be tested or measured.  Variant libraries named by FPC_ENGINE_LIB
    (A/B timing) are exempt."""
    if os.environ.get("FPC_ENGINE_LIB"):
        return
    try:
        want = open(LIB_PATH + ".srchash").read().strip()
    except OSError:
        return                                  # built by hand (hipcc ... -o libfpc_engine.so): nothing recorded
    import importlib.util
    spec = importlib.util.spec_from_file_location("_fpc_graft_entry", os.path.join(os.path.dirname(HERE), "__graft_entry__.py"))
    ge = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ge)
    csrc = os.path.join(HERE, "csrc")
    srcs = [os.path.join(csrc, f) for f in sorted(os.listdir(csrc)) if f.endswith((".cpp", ".h"))]
    srcs.append(os.path.join(os.path.dirname(HERE), "include", "fpc_engine.h"))
    if ge._src_hash(srcs, ge.HIPCC_FLAGS) != want:
        raise RuntimeError("stale HIP engine library: %s was built from other sources than the ones beside it; "
                           "rebuild with `python __graft_entry__.py`" % LIB_PATH)


def lib():
    """The product library.  Raises if it has not been built (python __graft_entry__.py)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError("HIP engine library missing: %s (build it with `python __graft_entry__.py`); "
                               "there is no CPU fallback" % LIB_PATH)
        _check_fresh()
        # PyTorch-ROCm ships its own libamdhip64.so.7; it must be the copy already mapped when the
        # engine library is loaded, otherwise two HIP runtimes end up in one process and the second
        # one to initialise sees no GPU.  torch is plumbing here (device tensors for the evaluator
        # seam, torch.distributed), not a compute path.
        try:
            import torch  # noqa: F401
            rccl = os.path.join(os.path.dirname(torch.__file__), "lib", "librccl.so")
            if os.path.exists(rccl):
                os.environ.setdefault("FPC_RCCL_LIB", rccl)    # fpc_comm_*: the RCCL that matches this HIP runtime
        except ImportError:
            pass
        _lib = bind(C.CDLL(LIB_PATH))
    return _lib


def comm_unique_id(_lib=None):
    """rank 0: the 128-byte ncclUniqueId to hand to the other ranks"""
    L = _lib if _lib is not None else lib()
    buf = (C.c_char * 128)()
    rc = L.fpc_comm_unique_id(buf)
    if rc != 0:
        raise RuntimeError("fpc_comm_unique_id failed (%d): %s" % (rc, (L.fpc_last_error(None) or b"").decode()))
    return bytes(buf)


def clone_board(b):
    nb = Board()
    C.memmove(C.byref(nb), C.byref(b), C.sizeof(Board))
    return nb


class Engine:
    """One engine handle == one GPU.  Thin, allocation-free-on-the-hot-path wrapper over the C-ABI."""

    def __init__(self, board_size, invalid_area, max_games=256, max_sims=400, avg_children=0, device=0, nn_dtype=0,
                 _lib=None):
        self.L = _lib if _lib is not None else lib()
        self.R, self.INV = board_size, invalid_area
        self.A_ch = self.L.fpc_num_action_channels(board_size)
        self.A = self.L.fpc_action_space_size(board_size)
        self.max_games, self.max_sims = max_games, max_sims
        self.device = device
        cfg = Config(board_size, invalid_area, max_games, max_sims, avg_children, device, nn_dtype)
        h = C.c_void_p()
        rc = self.L.fpc_create(C.byref(cfg), C.byref(h))
        if rc != 0:
            raise RuntimeError("fpc_create failed (%d): %s" % (rc, (self.L.fpc_last_error(None) or b"").decode()))
        self.h = h
        self.G = 0
        self.host_memory = bool(self.L.fpc_memory_is_host())   # the emulator build: "device" pointers are host memory
        self.replay_cap = [0] * (REPLAY_SCRATCH + 1)            # capacity of each replay ring (replay_reserve)
        self.replay_gen = [0] * (REPLAY_SCRATCH + 1)            # how often each ring has been reserved, i.e. emptied

    def close(self):
        if getattr(self, "h", None):
            self.L.fpc_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _chk(self, rc):
        if rc != 0:
            raise RuntimeError((self.L.fpc_last_error(self.h) or b"").decode() or ("fpc error %d" % rc))

    # ---- batched position ops (boards: list of Board, mutated in place like the reference) ----
    @staticmethod
    def _arr(boards):
        return (Board * len(boards))(*boards)

    @staticmethod
    def _writeback(arr, boards):
        for i, b in enumerate(boards):
            C.memmove(C.byref(b), C.byref(arr[i]), C.sizeof(Board))

    def legal_moves(self, boards):
        n = len(boards)
        arr = self._arr(boards)
        mv = (Move * (n * MAX_MOVES))()
        cnt = (C.c_int * n)()
        self._chk(self.L.fpc_boards_legal_moves(self.h, arr, n, mv, cnt))
        self._writeback(arr, boards)
        out = []
        for i in range(n):
            out.append([(mv[i * MAX_MOVES + k].frm, mv[i * MAX_MOVES + k].to, mv[i * MAX_MOVES + k].flat,
                         mv[i * MAX_MOVES + k].promo, mv[i * MAX_MOVES + k].capture) for k in range(cnt[i])])
        return out

    def game_result(self, boards, players=None):
        n = len(boards)
        arr = self._arr(boards)
        res = (C.c_int * n)()
        pl = (C.c_int * n)(*players) if players is not None else None
        self._chk(self.L.fpc_boards_game_result(self.h, arr, n, pl, res))
        self._writeback(arr, boards)
        return list(res)

    def take_action(self, boards, flats):
        n = len(boards)
        arr = self._arr(boards)
        out = (Board * n)()
        fl = (C.c_int * n)(*flats)
        self._chk(self.L.fpc_boards_take_action(self.h, arr, fl, n, out))
        return [clone_board(out[i]) for i in range(n)]

    def encode(self, boards):
        n = len(boards)
        out = np.zeros((n, 24, self.R, self.R), dtype=np.float32)
        self._chk(self.L.fpc_boards_encode(self.h, self._arr(boards), n, out.ctypes.data))
        return out

    def attack_maps(self, boards):
        """[n][6][R*R] uint8: attacked-square maps by colour (0..3, Board::IsAttackedByPlayer) and by team (4..5)"""
        n = len(boards)
        out = np.zeros((n, 6, self.R * self.R), dtype=np.uint8)
        self._chk(self.L.fpc_boards_attack_maps(self.h, self._arr(boards), n, out.ctypes.data))
        return out

    def legal_mask(self, boards):
        n = len(boards)
        arr = self._arr(boards)
        out = np.zeros((n, self.A_ch, self.R, self.R), dtype=np.float32)
        self._chk(self.L.fpc_boards_legal_mask(self.h, arr, n, out.ctypes.data))
        self._writeback(arr, boards)
        return out

    # ---- search ----
    def search_begin(self, roots, c_puct):
        self.G = len(roots)
        self._chk(self.L.fpc_search_begin(self.h, self._arr(roots), self.G, float(c_puct)))

    def search_select(self):
        n = C.c_int()
        p = C.c_void_p()
        self._chk(self.L.fpc_search_select(self.h, C.byref(n), C.byref(p)))
        return n.value, p.value

    def search_expand(self, logits_ptr, value_ptr):
        self._chk(self.L.fpc_search_expand(self.h, logits_ptr, value_ptr))

    def search_expand_select(self, logits_ptr, value_ptr):
        """search_expand of this simulation + search_select of the next one in one launch."""
        n = C.c_int()
        p = C.c_void_p()
        self._chk(self.L.fpc_search_expand_select(self.h, logits_ptr, value_ptr, C.byref(n), C.byref(p)))
        return n.value, p.value

    def search_run(self, sims):
        self._chk(self.L.fpc_search_run(self.h, sims))

    def search_results(self, max_children=256, roots=None, roots_np=None):
        """roots: list of Board to receive the root PODs as the search left them (piece-list order);
        roots_np: the same for a [G, 288] uint8 array (no per-game Python work)"""
        G = self.G
        rv = np.zeros(G, np.int32); nc = np.zeros(G, np.int32); sd = np.zeros(G, np.int32)
        cf = np.zeros((G, max_children), np.int32); cv = np.zeros((G, max_children), np.int32)
        cp = np.zeros((G, max_children), np.float32); cw = np.zeros((G, max_children), np.float64)
        pods = np.zeros((G, BOARD_BYTES), np.uint8) if roots_np is None else roots_np
        assert pods.shape == (G, BOARD_BYTES) and pods.dtype == np.uint8 and pods.flags.c_contiguous
        self._chk(self.L.fpc_search_results(self.h, _bp(pods), rv.ctypes.data, nc.ctypes.data, sd.ctypes.data, max_children,
                                            cf.ctypes.data, cv.ctypes.data, cp.ctypes.data, cw.ctypes.data))
        if roots is not None:
            for g, b in enumerate(roots):
                C.memmove(C.byref(b), pods[g].ctypes.data, BOARD_BYTES)
        return {"root_n": rv, "n_children": nc, "sims_done": sd, "flat": cf, "visits": cv, "prior": cp, "w": cw,
                "boards": _LazyBoards(pods)}

    def search_advance(self, flats, src_games=None, roots=None, roots_np=None):
        """subtree reuse (include/fpc_engine.h fpc_search_advance): re-root the finished search; new game i continues old
        game src_games[i] (None: game i) from the root child whose move is flats[i].  roots: list of Board, roots_np:
        [n, 288] uint8 array, to receive the new root PODs.  Returns the new roots' visit counts (int32 [n]); continue
        with search_run / the step entry points and search_results."""
        fl = np.ascontiguousarray(flats, np.int32)
        n = int(fl.shape[0])
        sg = None
        if src_games is not None:
            sa = np.ascontiguousarray(src_games, np.int32)
            assert sa.shape == (n,)
            sg = C.cast(sa.ctypes.data, P(C.c_int))
        pods = np.zeros((n, BOARD_BYTES), np.uint8) if roots_np is None else roots_np
        assert pods.shape == (n, BOARD_BYTES) and pods.dtype == np.uint8 and pods.flags.c_contiguous
        kept = np.zeros(n, np.int32)
        rc = self.L.fpc_search_advance(self.h, sg, C.cast(fl.ctypes.data, P(C.c_int)), n, _bp(pods) if n else None,
                                       C.cast(kept.ctypes.data, P(C.c_int)))
        if rc == 0 or rc == -7:           # FPC_EMOVE: the other games were advanced
            self.G = n
        self._chk(rc)
        if roots is not None:
            for g, b in enumerate(roots):
                C.memmove(C.byref(b), pods[g].ctypes.data, BOARD_BYTES)
        return kept

    def search_advance_refill(self, flats, src_games, fresh=None, roots=None, roots_np=None):
        """subtree reuse with refill (include/fpc_engine.h fpc_search_advance_refill): search_advance in which
        src_games[i] == -1 starts a new game in row i on fresh[i] instead (flats[i] is then ignored).  fresh: list of
        Board or [n, 288] uint8 array, read at the -1 positions only (None where there is none); src_games None:
        identity.  roots / roots_np receive the new root PODs.  Returns the kept visit counts (int32 [n], 1 for a fresh
        row)."""
        fl = np.ascontiguousarray(flats, np.int32)
        n = int(fl.shape[0])
        sg = None
        if src_games is not None:
            sa = np.ascontiguousarray(src_games, np.int32)
            assert sa.shape == (n,)
            sg = C.cast(sa.ctypes.data, P(C.c_int))
        fr = None
        if fresh is not None:
            if isinstance(fresh, np.ndarray):
                assert fresh.shape == (n, BOARD_BYTES) and fresh.dtype == np.uint8 and fresh.flags.c_contiguous
                fr = _bp(fresh)
            else:
                assert len(fresh) == n
                arr = (Board * n)()
                for i, b in enumerate(fresh):
                    if b is not None:
                        C.memmove(C.byref(arr[i]), C.byref(b), BOARD_BYTES)
                fr = arr
        pods = np.zeros((n, BOARD_BYTES), np.uint8) if roots_np is None else roots_np
        assert pods.shape == (n, BOARD_BYTES) and pods.dtype == np.uint8 and pods.flags.c_contiguous
        kept = np.zeros(n, np.int32)
        rc = self.L.fpc_search_advance_refill(self.h, sg, C.cast(fl.ctypes.data, P(C.c_int)), fr, n, _bp(pods) if n else None,
                                              C.cast(kept.ctypes.data, P(C.c_int)))
        if rc == 0 or rc == -7:           # FPC_EMOVE: the other games were advanced
            self.G = n
        self._chk(rc)
        if roots is not None:
            for g, b in enumerate(roots):
                C.memmove(C.byref(b), pods[g].ctypes.data, BOARD_BYTES)
        return kept

    def search_set_budget(self, budget):
        """per-game simulation budgets of the search in progress (include/fpc_engine.h fpc_search_set_budget): budget[g]
        caps the simulations game g completes in this search (sims_done[g]); a game at its budget selects nothing.  Set
        after search_begin / search_advance(_refill) and before the search's first selection; None clears them, and so
        does every later begin / advance.  The step count stays the caller's: run max(budget) simulations."""
        if budget is None:
            self._chk(self.L.fpc_search_set_budget(self.h, None, self.G))
            return
        b = np.ascontiguousarray(budget, np.int32)
        assert b.ndim == 1
        self._chk(self.L.fpc_search_set_budget(self.h, C.cast(b.ctypes.data, P(C.c_int)), int(b.shape[0])))

    def search_set_fast_rows(self, fast):
        """playout cap randomization (include/fpc_engine.h fpc_search_set_fast_rows): fast[g] true marks game g's search of
        this ply as a fast search -- no forced playouts in its selection, no pruning of its target, TUPLE_FAST in its
        record.  Noise is the caller's: give a fast row an all-zero gamma row.  Set after search_begin /
        search_advance(_refill) and before the search's first selection; None clears the mask, and so does every later
        begin / advance."""
        if fast is None:
            self._chk(self.L.fpc_search_set_fast_rows(self.h, None, self.G))
            return
        m = np.ascontiguousarray(fast, np.uint8)
        assert m.ndim == 1
        self._chk(self.L.fpc_search_set_fast_rows(self.h, m.ctypes.data, int(m.shape[0])))

    def search_finish(self):
        """fpc_search_results with every array NULL: waits for the search, reads the games' error words (raises on one)
        and nothing else.  For callers that go on with search_play / search_advance and need no child arrays."""
        self._chk(self.L.fpc_search_results(self.h, None, None, None, None, 0, None, None, None, None))

    def search_play(self, temperature, uniforms, want_boards=True):
        """device-side move choice (include/fpc_engine.h fpc_search_play) on the finished search: per game, draw the move
        from the root's visit counts with uniforms[g] in [0, 1) (temperature 0: first maximum), make it on the root state
        and run GetGameResult.  Returns (flats int32 [G], results int32 [G], boards): boards is the [G, 288] uint8 array
        of next states search_begin_np takes (None unless want_boards).  A game with a childless root gets -1, -1 and
        its root state.  The tree is left as it is: search_advance(flats) or a new search may follow."""
        G = self.G
        u = np.ascontiguousarray(uniforms, np.float64)
        assert u.shape == (G,), (u.shape, G)
        flats, results = np.zeros(G, np.int32), np.zeros(G, np.int32)
        pods = np.zeros((G, BOARD_BYTES), np.uint8) if want_boards else None
        self._chk(self.L.fpc_search_play(self.h, float(temperature), C.cast(u.ctypes.data, P(C.c_double)),
                                         C.cast(flats.ctypes.data, P(C.c_int)), C.cast(results.ctypes.data, P(C.c_int)),
                                         _bp(pods) if want_boards and G else None))
        return flats, results, pods

    def search_play_ms(self):
        """HIP-event time of k_play_ply in the last search_play (set_timing(True) first)"""
        ms = C.c_float()
        self._chk(self.L.fpc_search_play_ms(self.h, C.byref(ms)))
        return ms.value

    # ---- the same position ops on [n, 288] uint8 arrays of PODs (callers that keep a whole batch in one array:
    #      bench.py's per-ply host section, mcts.py's root-children prefetch) ----
    def search_begin_np(self, pods, c_puct):
        assert pods.ndim == 2 and pods.shape[1] == BOARD_BYTES and pods.dtype == np.uint8 and pods.flags.c_contiguous
        self.G = pods.shape[0]
        self._chk(self.L.fpc_search_begin(self.h, _bp(pods), self.G, float(c_puct)))

    def take_action_np(self, pods, flats):
        """pods [n, 288] (left untouched), flats int32 [n] -> the n successor PODs"""
        pods = np.ascontiguousarray(pods, np.uint8)
        fl = np.ascontiguousarray(flats, np.int32)
        n = pods.shape[0]
        out = np.zeros((n, BOARD_BYTES), np.uint8)
        if n:
            self._chk(self.L.fpc_boards_take_action(self.h, _bp(pods), C.cast(fl.ctypes.data, P(C.c_int)), n, _bp(out)))
        return out

    def game_result_np(self, pods, players=None):
        """GetGameResult of every POD of the C-contiguous array `pods`, which is rewritten in place (the reference's
        GetGameResult permutes the piece lists); returns int32 [n]"""
        assert pods.dtype == np.uint8 and pods.flags.c_contiguous
        n = pods.shape[0]
        res = np.zeros(n, np.int32)
        pl = None if players is None else C.cast(np.ascontiguousarray(players, np.int32).ctypes.data, P(C.c_int))
        if n:
            self._chk(self.L.fpc_boards_game_result(self.h, _bp(pods), n, pl, C.cast(res.ctypes.data, P(C.c_int))))
        return res

    def grandchildren(self, game, child_idx, max_children=256):
        n = C.c_int()
        fl = np.zeros(max_children, np.int32); vi = np.zeros(max_children, np.int32)
        self._chk(self.L.fpc_search_grandchildren(self.h, game, child_idx, max_children, C.byref(n), fl.ctypes.data,
                                                  vi.ctypes.data))
        return [[int(fl[i]), int(vi[i])] for i in range(min(n.value, max_children))]

    def load_weights(self, blob):
        buf = (C.c_char * len(blob)).from_buffer_copy(blob)
        self._chk(self.L.fpc_load_weights(self.h, buf, len(blob)))

    # ---- device-side weight pack (include/fpc_engine.h fpc_weights_pack / fpc_load_weights_device) ----
    def _net_src(self, model, fc_layout):
        """(descriptor, keep-alive list, fc_layout word): the module's tensors on this engine's device (the emulator:
        the host), torch's work on them finished"""
        import torch
        import weights
        dev = "cpu" if self.host_memory else "cuda:%d" % self.device
        src, keep = weights.net_src(model, dev)
        if not self.host_memory:
            torch.cuda.current_stream(self.device).synchronize()
        if fc_layout is None:
            fc_layout = weights.FC_LAYOUT if weights.FC_LAYOUT is not None else 0     # 0: the engine chooses as default_fc_layout does
        return src, keep, int(fc_layout)

    def weights_blob_size(self, hidden, nblocks, fc_layout=0):
        n = C.c_uint64()
        self._chk(self.L.fpc_weights_blob_size(self.h, int(hidden), int(nblocks), int(fc_layout), C.byref(n)))
        return n.value

    def set_fc_weight_type(self, fc_weights):
        """the policy Linear's weight type of the NEXT weights_blob_size / weights_pack / load_weights_device: "w16" (the
        default) or "int8" (opt-in: fp16 engines and fc_layout 2 only; include/fpc_engine.h fpc_set_fc_weight_type).
        Persistent.  load_weights takes the type from the blob's header."""
        import weights
        if fc_weights not in weights.FC_WEIGHTS:
            raise ValueError("fc_weights must be \"w16\" or \"int8\"")
        self._chk(self.L.fpc_set_fc_weight_type(self.h, weights.FC_WEIGHTS[fc_weights]))

    def nn_fc_kernel(self):
        """"k_fcw8" | "k_fcw" | "k_fc16": the kernel that runs the policy Linear for the loaded weights ("" before a load)"""
        return (self.L.fpc_nn_fc_kernel(self.h) or b"").decode()

    def weights_pack(self, model, fc_layout=None, fc_weights=None):
        """the module packed ON THE DEVICE into a version-3 blob (fc_weights "int8": version 4; None: the type last set),
        read back: the bytes of weights.export_weights(model, nn_dtype, fc_layout, fc_weights) computed op for op in f32 with correctly rounded divide and
        square root.  Where torch's CPU sqrt is not correctly rounded (0.69 % of random BN variances on the
        build measured) export_weights itself is one unit off in that channel and the two blobs differ there."""
        import torch
        if fc_weights is not None:
            self.set_fc_weight_type(fc_weights)
        src, keep, fl = self._net_src(model, fc_layout)
        cap = self.weights_blob_size(src.hidden, src.nblocks, fl)
        buf = torch.empty(cap + 64, dtype=torch.uint8, device="cpu" if self.host_memory else "cuda:%d" % self.device)
        ptr = (buf.data_ptr() + 63) & ~63
        n = C.c_uint64()
        self._chk(self.L.fpc_weights_pack(self.h, C.byref(src), fl, ptr, cap, C.byref(n)))
        off = ptr - buf.data_ptr()
        out = buf[off:off + n.value].cpu().numpy().tobytes()
        del keep
        return out

    def load_weights_device(self, model, fc_layout=None, fc_weights=None):
        """load_weights(export_weights(model)) without the host: the pack kernels read the module's parameters in device
        memory and write the engine's weight allocations (in place when the network's geometry has not changed).
        fc_weights "w16" | "int8": set_fc_weight_type first (None: the type last set, "w16" on a fresh engine)."""
        if fc_weights is not None:
            self.set_fc_weight_type(fc_weights)
        src, keep, fl = self._net_src(model, fc_layout)
        self._chk(self.L.fpc_load_weights_device(self.h, C.byref(src), fl))
        del keep

    def weights_pack_ms(self):
        """HIP-event time of the pack kernels in the last weights_pack / load_weights_device (set_timing(True) first)"""
        ms = C.c_float()
        self._chk(self.L.fpc_weights_pack_ms(self.h, C.byref(ms)))
        return ms.value

    def nn_forward(self, enc_ptr, n, logits_ptr, value_ptr):
        self._chk(self.L.fpc_nn_forward(self.h, enc_ptr, n, logits_ptr, value_ptr))

    def stats(self):
        s = Stats()
        self.L.fpc_stats_get(self.h, C.byref(s))
        return {k: getattr(s, k) for k, _ in Stats._fields_}

    def stats_reset(self):
        self.L.fpc_stats_reset(self.h)

    def set_policy_mode(self, legal_only):
        """fpc_search_run's policy head: False = the whole Linear + full softmax (reference arithmetic),
        True = only the leaf's legal moves (same priors up to f32 rounding; include/fpc_engine.h)."""
        self._chk(self.L.fpc_set_policy_mode(self.h, 1 if legal_only else 0))

    def set_timing(self, on):
        self.L.fpc_set_timing(self.h, 1 if on else 0)

    # ---- N4: non-strict rule set and root Dirichlet noise (include/fpc_engine.h FPC_RULES_*) ----
    def set_rules(self, rules):
        """0 = strict reference semantics (default); RULES_FIXED = the four corrections of selection, rotation, planes and
        moves; RULES_TRAINING = those plus RULES_TERMINAL (a terminal leaf is valued by its result and the search goes on).
        0..31, as ever; the sets with RULES_VISITS go through set_rule_bits"""
        self._chk(self.L.fpc_set_rules(self.h, int(rules)))

    def set_rule_bits(self, rules):
        """set_rules over all six bits, 0..63 (include/fpc_engine.h fpc_set_rule_bits): RULES_SELFPLAY = RULES_TRAINING plus
        RULES_VISITS (every node is born with N = 0: N counts real visits only), or RULES_VISITS with any other bits"""
        self._chk(self.L.fpc_set_rule_bits(self.h, int(rules)))

    def set_leaves(self, k, virtual_loss=1.0):
        """leaf-parallel search (include/fpc_engine.h fpc_search_set_leaves): up to k leaves per game per simulation
        step, kept apart by virtual loss; the step-wise evaluator then sees [k*G, 24, R, R].  k = 1: one leaf per game."""
        self._chk(self.L.fpc_search_set_leaves(self.h, int(k), float(virtual_loss)))

    def set_fpu(self, mode, reduction=0.0):
        """first-play urgency (include/fpc_engine.h fpc_search_set_fpu): FPU_ZERO (default) or FPU_PARENT -- under RULES_PUCT a
        child with no visit, pending ones included, gets q = W_p / N_p - reduction of the node above it.  Persistent; without
        RULES_VISITS no child is ever unvisited and the setting has no effect."""
        self._chk(self.L.fpc_search_set_fpu(self.h, int(mode), float(reduction)))

    def set_solver(self, on):
        """MCTS solver (include/fpc_engine.h fpc_search_set_solver): terminal results are proven up the tree -- proven
        children are backed up without a board, moves that lose are left out of the selection, a proven root idles, and
        search_play plays a proven win or draw.  In effect only under RULES_PUCT | RULES_TERMINAL; persistent."""
        self._chk(self.L.fpc_search_set_solver(self.h, int(on)))

    def search_proofs(self, max_children=256):
        """(root statuses uint8 [G], child statuses uint8 [G, max_children]) of the search: PROOF_* from each node's own
        side to move, children in search_results' order (include/fpc_engine.h fpc_search_proofs)"""
        G = self.G
        root = np.zeros(G, np.uint8)
        child = np.zeros((G, max_children), np.uint8)
        self._chk(self.L.fpc_search_proofs(self.h, int(max_children), root.ctypes.data, child.ctypes.data))
        return root, child

    def set_forced(self, factor):
        """forced playouts and policy target pruning at the root (include/fpc_engine.h fpc_search_set_forced): a visited
        root child is guaranteed sqrt(factor * P * N) simulations, and collect_tuples / search_play / search_targets take the
        visits that only the forcing put there out again.  0: off (default); 2.0 is the usual value.  In effect only under
        RULES_PUCT | RULES_VISITS; persistent."""
        self._chk(self.L.fpc_search_set_forced(self.h, float(factor)))

    def search_targets(self, max_children=256):
        """int32 [G, max_children]: the pruned visit counts of each root's children in search_results' order, zero past a
        root's children; the stored visit counts when forcing is not in effect (include/fpc_engine.h fpc_search_targets)"""
        out = np.zeros((self.G, max_children), np.int32)
        self._chk(self.L.fpc_search_targets(self.h, int(max_children), out.ctypes.data))
        return out

    def set_live_rows(self, on):
        """live-row numbering (include/fpc_engine.h fpc_search_set_live_rows): every step's live leaves are the network's
        rows 0..n_live-1 in ascending row order; the step-wise evaluator's encodings are in that order (rows n_live.. are
        zero) and its logits / values are read at n_live rows only.  Same search results; persistent."""
        self._chk(self.L.fpc_search_set_live_rows(self.h, int(on)))

    def set_root_noise(self, gamma, eps):
        """gamma: float32 array [n_games, MAX_MOVES] of Gamma(alpha) draws (None: off)"""
        if gamma is None:
            self._chk(self.L.fpc_search_set_root_noise(self.h, None, 0, 0.0))
            return
        g = np.ascontiguousarray(gamma, dtype=np.float32)
        assert g.ndim == 2 and g.shape[1] == MAX_MOVES
        self._chk(self.L.fpc_search_set_root_noise(self.h, g.ctypes.data, g.shape[0], float(eps)))

    # ---- training tuples (device resident) and their RCCL exchange ----
    def tuples_reserve(self, capacity):
        self._chk(self.L.fpc_tuples_reserve(self.h, int(capacity)))

    def tuples_reset(self):
        self._chk(self.L.fpc_tuples_reset(self.h))

    def collect_tuples(self, game_ids, ply):
        """one tuple per game of the search that just finished (root mailbox, side to move, sparse pi);
        game_ids: sequence or int32 array"""
        ids = None
        if game_ids is not None:
            ia = np.ascontiguousarray(game_ids, np.int32)
            ids = C.cast(ia.ctypes.data, P(C.c_int))
        self._chk(self.L.fpc_collect_tuples(self.h, ids, int(ply)))

    def tuples_set_z(self, game_ids, z_team0, z_team1):
        """one call for any number of finished games (sequences or arrays)"""
        ia = np.ascontiguousarray(game_ids, np.int32)
        z0 = np.ascontiguousarray(z_team0, np.float32)
        z1 = np.ascontiguousarray(z_team1, np.float32)
        n = ia.shape[0]
        assert z0.shape[0] == n and z1.shape[0] == n
        self._chk(self.L.fpc_tuples_set_z(self.h, C.cast(ia.ctypes.data, P(C.c_int)), C.cast(z0.ctypes.data, P(C.c_float)),
                                          C.cast(z1.ctypes.data, P(C.c_float)), n))

    def tuples_count(self):
        return self.L.fpc_tuples_count(self.h)

    def tuples_read(self, first=0, n=None):
        n = self.tuples_count() - first if n is None else n
        arr = (Tuple * max(n, 1))()
        self._chk(self.L.fpc_tuples_read(self.h, arr, first, n))
        return arr, n

    def comm_init(self, id128, rank, world):
        buf = (C.c_char * 128).from_buffer_copy(bytes(id128))
        self._chk(self.L.fpc_comm_init(self.h, buf, rank, world))
        self.comm_world = world

    def debug_comm_fault(self, point):
        """TEST HOOK: the next allgather_tuples treats one of its own HIP calls as failed (include/fpc_engine.h)"""
        self._chk(self.L.fpc_debug_comm_fault(self.h, point))

    def allgather_tuples_device(self):
        """episode end: RCCL all-gather of every rank's tuples, driven from the C++ host; the gathered
        tuples stay on the device.  Returns (per-rank counts, total)."""
        counts, total = (C.c_int * max(getattr(self, 'comm_world', 1), 1))(), C.c_int()
        self._chk(self.L.fpc_allgather_tuples(self.h, counts, C.byref(total)))
        return counts, total.value

    def gathered_read(self, total):
        arr = (Tuple * max(total, 1))()
        if total:
            self._chk(self.L.fpc_gathered_read(self.h, arr, 0, total))
        return arr

    def allgather_tuples(self):
        """(per-rank counts, ctypes array of all tuples in rank order, total)"""
        counts, total = self.allgather_tuples_device()
        return counts, self.gathered_read(total), total

    # ---- device-resident replay (include/fpc_engine.h fpc_replay_*) ----
    def replay_reserve(self, ring, capacity):
        """(re)allocate and empty one ring of `capacity` records in device memory (1280 B each)"""
        self._chk(self.L.fpc_replay_reserve(self.h, int(ring), int(capacity)))
        self.replay_cap[ring] = int(capacity)
        self.replay_gen[ring] += 1

    def replay_push(self, source=REPLAY_COLLECTED, src_index=None, ring_of=None, m=None):
        """append source tuples src_index[j] (None: 0..m-1) to ring ring_of[j] (None: ring 0; -1: dropped), j in order,
        device to device.  source: REPLAY_COLLECTED (index space of tuples_read) or REPLAY_GATHERED (gathered_read)."""
        si = None if src_index is None else np.ascontiguousarray(src_index, np.int32)
        ro = None if ring_of is None else np.ascontiguousarray(ring_of, np.int8)
        if m is None:
            m = si.shape[0] if si is not None else ro.shape[0] if ro is not None else self.tuples_count()
        assert (si is None or si.shape == (m,)) and (ro is None or ro.shape == (m,))
        self._chk(self.L.fpc_replay_push(self.h, int(source), None if si is None else C.cast(si.ctypes.data, P(C.c_int)),
                                         None if ro is None else C.cast(ro.ctypes.data, P(C.c_int8)), int(m)))

    def replay_load(self, ring, arr, n=None):
        """append n records of a ctypes fpc_tuple array from host memory (resume, tests)"""
        n = len(arr) if n is None else n
        self._chk(self.L.fpc_replay_load(self.h, int(ring), arr, int(n)))

    def replay_size(self, ring):
        n = self.L.fpc_replay_size(self.h, int(ring))
        if n < 0:
            self._chk(n)
        return n

    def replay_read(self, ring, first=0, n=None):
        """(ctypes fpc_tuple array, n): slots first .. first+n-1 of the ring (default: all of it)"""
        n = self.replay_size(ring) - first if n is None else n
        arr = (Tuple * max(n, 1))()
        self._chk(self.L.fpc_replay_read(self.h, int(ring), arr, int(first), int(n)))
        return arr, n

    def replay_batch(self, ring, slots, enc, pi, z, w=None):
        """decode the records in `slots` (any order, repeats allowed) into enc [n,24,R,R], pi [n,A], z [n] (f32, device
        memory; on the emulator, host memory): contiguous torch tensors / numpy arrays, or raw pointers.  One launch;
        the engine's stream is synchronised before this returns.  w (optional, [n] f32): the records' policy-loss weights,
        0.0 for a record with TUPLE_FAST and 1.0 otherwise (fpc_replay_batch_w)."""
        sl = np.ascontiguousarray(slots, np.int32)
        n = int(sl.shape[0])
        ptrs = []
        outs = [(enc, (n, 24, self.R, self.R)), (pi, (n, self.A)), (z, (n,))] + ([] if w is None else [(w, (n,))])
        for t, shape in outs:
            if isinstance(t, int):
                ptrs.append(t)
                continue
            if isinstance(t, np.ndarray):
                assert t.dtype == np.float32 and t.flags.c_contiguous and t.size == int(np.prod(shape)), shape
                ptrs.append(t.ctypes.data)
            else:
                assert str(t.dtype) == "torch.float32" and t.is_contiguous() and t.numel() == int(np.prod(shape)), shape
                ptrs.append(t.data_ptr())
        if (ptrs[0] | ptrs[1]) & 15:
            raise ValueError("replay_batch: enc and pi must start on a 16-byte boundary (the kernel writes 16-byte pieces); "
                             "a sliced view with an odd storage offset does not -- pass a tensor of its own")
        fn = self.L.fpc_replay_batch if w is None else self.L.fpc_replay_batch_w
        self._chk(fn(self.h, int(ring), C.cast(sl.ctypes.data, P(C.c_int)), n, *ptrs))

    def replay_decode_ms(self):
        """HIP-event time of k_replay_decode in the last replay_batch (set_timing(True) first)"""
        ms = C.c_float()
        self._chk(self.L.fpc_replay_decode_ms(self.h, C.byref(ms)))
        return ms.value


def board_from_dict(R, turn, entries, castle=None, _lib=None):
    """entries: [(sq, colour, type), ...] in dict insertion order -> Board with the reference's ctor order."""
    L = _lib if _lib is not None else lib()
    n = len(entries)
    sqs = (C.c_uint8 * max(n, 1))(*[e[0] for e in entries])
    pcs = (C.c_uint8 * max(n, 1))(*[0x80 | (e[1] << 5) | (e[2] << 2) for e in entries])
    cs = (C.c_uint8 * 4)(*castle) if castle is not None else None
    b = Board()
    rc = L.fpc_board_from_dict(C.byref(b), R, turn, sqs, pcs, n, cs)
    if rc != 0:
        raise RuntimeError("fpc_board_from_dict failed (%d)" % rc)
    return b


def board_from_lists(R, turn, pl):
    """pl: per colour [[sq, type], ...] already in piece-list order (fixture format)."""
    b = Board()
    for c in range(4):
        b.king[c] = NO_SQ
    b.turn = turn
    for colour, col in enumerate(pl):
        for sq, typ in col:
            b.sq[sq] = 0x80 | (colour << 5) | (typ << 2)
            b.pl[colour][b.plen[colour]] = sq
            b.plen[colour] += 1
            if typ == 5:
                b.king[colour] = sq
    return b


def lists_of(b):
    return [[[b.pl[c][i], (b.sq[b.pl[c][i]] >> 2) & 7] for i in range(b.plen[c])] for c in range(4)]
