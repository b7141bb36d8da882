"""Plain-Python model of the engine's search beyond the oracle's orc_search (oracle/fpc_oracle.cpp): up to K leaves per
game per simulation step, kept apart by virtual loss (include/fpc_engine.h fpc_search_set_leaves), on
trees that PERSIST from ply to ply (fpc_search_advance).  `Model.search` runs simulations on the trees
as they are, `Model.advance` re-roots every kept game on the root child that was played: the child's object subtree is
kept as it is (statistics, priors, children's order, every state already made), the state of a child that was never
selected is made with orc.take_action and nothing else, an already expanded new root gets the root noise.  `search` is
the one-ply form: fresh trees, one Model.search.

Board work goes through the oracle's primitives (orc.legal_moves / game_result / take_action / encode) and the priors
through orc_policy_priors -- with policy_head="legal" through orc_policy_priors_legal, the arithmetic of the opt-in
legal-only head (fpc_set_policy_mode) and the ONLY thing the switch changes -- so that the model and the
kernels meet at bit level.  Selection arithmetic is fp64 without
contraction (Python floats), the log table is math.log(math.sqrt(n)) as the host table is; f32 work (values, root
noise) is done on numpy float32 scalars.

Also here: `run_steps` / `run_stepwise` / `run_plies`, which drive an engine through the step-wise C-ABI the way
mcts.MCTS does with K leaves (the loop itself is fpc_testlib.run_schedule), the pick rule of the tree-reuse tests, and
the comparison helpers.
"""
import ctypes as C
import math

import numpy as np

import fpc_ffi
from fpc_testlib import run_schedule
from oracle import orc

RULES_PUCT, RULES_ROTATION = 1, 2


class _Node:
    __slots__ = ("N", "W", "VL", "P", "flat", "parent", "children", "state")

    def __init__(self, P, flat, parent, state=None):
        self.N, self.W, self.VL = 1, 0.0, 0      # node.h:28 default visit_count 1 (Q1)
        self.P, self.flat, self.parent = P, flat, parent
        self.children = []                       # parent / children hold node OBJECTS
        self.state = state                       # made from the parent's state the first time the node is reached


POLICY_HEADS = ("full", "legal")


def _priors(logits_row, R, rot, legal, policy_head="full"):
    L = orc.lib()
    lg = np.ascontiguousarray(logits_row, dtype=np.float32)
    lf = np.ascontiguousarray(legal, dtype=np.int32)
    out = np.zeros(max(len(legal), 1), dtype=np.float32)
    fn = L.orc_policy_priors_legal if policy_head == "legal" else L.orc_policy_priors
    rc = fn(lg.ctypes.data_as(C.POINTER(C.c_float)), R, rot, lf.ctypes.data_as(C.POINTER(C.c_int)), len(legal),
            out.ctypes.data_as(C.POINTER(C.c_float)))
    return rc, out[:len(legal)]


def schedule(sims, leaves):
    """leaves per step: an int K -> ceil(sims / K) steps of K, the last one of the remainder; a list is taken as it is"""
    if not isinstance(leaves, int):
        return list(leaves)
    steps = (sims + leaves - 1) // leaves
    return [leaves if s + 1 < steps else sims - leaves * (steps - 1) for s in range(steps)]


class Model:
    def __init__(self, boards, R, INV, Cpuct, evaluator, rules=0, vl=1.0, noise_eps=0.0, policy_head="full"):
        """boards: orc boards (mutated like the engine mutates its roots' piece lists).  evaluator: numpy callable
        enc[B,24,R,R] -> (logits[B,A], value[B]).  policy_head: "full" | "legal" (the priors' arithmetic, nothing else)."""
        assert policy_head in POLICY_HEADS
        self.R, self.INV, self.Cpuct, self.ev, self.rules, self.vl = R, INV, float(Cpuct), evaluator, rules, float(vl)
        self.policy_head = policy_head
        # per simulation step: {"rows", "dead": the rows without a leaf to expand (terminal leaf, collision, game over),
        # "pairs": (live row, legal move) pairs, "turns": the live rows' sides to move, "max_legal"}
        self.steps = []
        # a list: every expansion appends (the leaf is a root, its logits row, rotation, legal list) -- tests/prior_cases.py
        self.expansions = None
        self.noise, self.noise_eps = None, noise_eps
        self.roots = [_Node(0.0, -1, None, state=b) for b in boards]
        self.alive = [True] * len(boards)
        self.sims_done = [0] * len(boards)
        self.counts = {"collisions": 0, "terminals": 0}

    def set_noise(self, gamma):
        """float32 [G][MAX_MOVES] gamma draws for the NEXT advance / expansions (None: off)"""
        self.noise = None if gamma is None else np.asarray(gamma, dtype=np.float32)

    def _noisy(self, g, pri):
        gm = self.noise[g]
        sg = np.float32(0)
        for j in range(len(pri)):
            sg = np.float32(sg + gm[j])
        if not sg > 0:
            return pri
        one, eps = np.float32(1), np.float32(self.noise_eps)
        return [np.float32((one - eps) * np.float32(p)) + np.float32(eps * np.float32(gm[j] / sg)) for j, p in enumerate(pri)]

    @staticmethod
    def _backprop(path, v):                      # node.cpp:133-142 along the descent path: leaf +v, parent -v, ...
        v = np.float32(v)
        for nd in reversed(path):
            nd.W += float(v)
            nd.N += 1
            v = -v

    def search(self, sims, leaves=1):
        """`sims` more simulations on the trees as they stand; leaves: K, or a list of leaves per step (schedule()).
        rc: 0, -2 (no child selectable), -3 (policy error), -4 (move failed)"""
        orc.set_rules(self.rules)
        try:
            return self._search(schedule(sims, leaves))
        finally:
            orc.set_rules(0)

    def _search(self, sched):
        R, INV, rules, vl, Cpuct = self.R, self.INV, self.rules, self.vl, self.Cpuct
        G = len(self.roots)
        for ks in sched:
            nrows = ks * G
            rows = [None] * nrows
            # ---- selection: per game, ks descents in sequence; collision / terminal leaf end the game's step
            for g in range(G):
                if not self.alive[g]:
                    continue
                for k in range(ks):
                    nd = self.roots[g]
                    path = [nd]
                    while nd.children:
                        Np = nd.N + nd.VL
                        lp, sq = math.log(math.sqrt(Np)), math.sqrt(Np)
                        best, bu = None, -math.inf
                        for ch in nd.children:
                            Nc = ch.N + ch.VL
                            if rules & RULES_PUCT:
                                Wc = ch.W + vl * ch.VL
                                q = -(Wc / Nc) if Nc > 0 else 0.0
                                u = q + Cpuct * ch.P * sq / (1 + Nc)
                            else:
                                Wc = ch.W - vl * ch.VL
                                q = Wc / Nc if Nc > 0 else 0.0
                                u = q + Cpuct * math.sqrt(lp / (1 + Nc)) * ch.P
                            if u > bu:
                                best, bu = ch, u
                        if best is None:
                            return -2
                        nd = best
                        path.append(nd)
                    if nd.VL > 0:                # collision: nothing is touched
                        self.counts["collisions"] += 1
                        break
                    if nd.state is None:
                        st, mrc = orc.take_action(nd.parent.state, R, nd.flat)
                        if mrc != 0:
                            return -4
                        nd.state = st
                    res = orc.game_result(nd.state, R, INV)
                    if res != 0:                 # node.cpp:31-42, Q5
                        self._backprop(path, 0.0 if res == 3 else -1.0)
                        self.sims_done[g] += 1
                        self.alive[g] = False
                        self.counts["terminals"] += 1
                        break
                    legal = sorted(set(m[2] for m in orc.legal_moves(nd.state, R, INV)))
                    rows[k * G + g] = (g, nd, path, legal)
                    for p in path:
                        p.VL += 1
            live = [r for r in range(nrows) if rows[r] is not None]
            self.steps.append({"rows": nrows, "dead": [r for r in range(nrows) if rows[r] is None],
                               "pairs": sum(len(rows[r][3]) for r in live),
                               "turns": [rows[r][1].state.turn for r in live],
                               "max_legal": max([len(rows[r][3]) for r in live], default=0)})
            if not live:
                continue
            # ---- evaluation of rows 0 .. ks*G-1, dead rows all-zero
            states = [rows[r][1].state for r in live]
            enc = np.zeros((nrows, 24, R, R), dtype=np.float32)
            enc[live] = orc.encode(states, R)    # rotation: the first live row's turn (Q6) or each row's own
            logits, value = self.ev(enc)
            logits = np.asarray(logits, dtype=np.float32).reshape(nrows, -1)
            value = np.asarray(value, dtype=np.float32).reshape(nrows)
            turn0 = states[0].turn
            # ---- expansion: per game, live rows in ascending k
            for g in range(G):
                for k in range(ks):
                    row = rows[k * G + g]
                    if row is None:
                        continue
                    _, nd, path, legal = row
                    r = k * G + g
                    rot = nd.state.turn if rules & RULES_ROTATION else turn0
                    prc, pri = _priors(logits[r], R, rot, legal, self.policy_head)
                    if self.expansions is not None:
                        self.expansions.append((nd is self.roots[g], logits[r].copy(), rot, legal))
                    if prc:
                        return -3
                    if self.noise is not None and nd is self.roots[g]:
                        pri = self._noisy(g, pri)
                    self._backprop(path, value[r])
                    for p in path:
                        p.VL -= 1
                    self.sims_done[g] += 1
                    for j, fl in enumerate(legal):
                        if pri[j] == 0:
                            continue             # torch.nonzero drops exact zeros
                        nd.children.append(_Node(float(pri[j]), fl, nd))
        return 0

    def advance(self, src_games, flats):
        """new game i continues old game src_games[i] (None: game i) from the root child whose move is flats[i]"""
        src_games = list(range(len(flats))) if src_games is None else list(src_games)
        assert all(a < b for a, b in zip(src_games, src_games[1:]))
        orc.set_rules(self.rules)
        try:
            roots = []
            for i, (sg, fl) in enumerate(zip(src_games, flats)):
                old = self.roots[sg]
                ch = next(c for c in old.children if c.flat == fl)
                if ch.state is None:                 # never selected (Q1: N = 1): the move is made, and no more
                    ch.state, mrc = orc.take_action(old.state, self.R, fl)
                    assert mrc == 0
                ch.parent, ch.flat = None, -1
                if self.noise is not None and ch.children:
                    for c, p in zip(ch.children, self._noisy(i, [c.P for c in ch.children])):
                        c.P = float(p)
                roots.append(ch)
        finally:
            orc.set_rules(0)
        self.roots = roots
        self.alive = [True] * len(roots)
        self.sims_done = [0] * len(roots)
        return [r.N for r in roots]

    def results(self):
        """orc.search's format + "grand" per root child"""
        out = []
        for g, root in enumerate(self.roots):
            kids = root.children
            out.append({"root_n": root.N, "terminated": not self.alive[g], "sims_done": self.sims_done[g],
                        "children": [[c.flat, c.N] for c in kids],
                        "priors": np.array([c.P for c in kids], dtype=np.float32),
                        "w": np.array([c.W for c in kids], dtype=np.float64),
                        "grand": [[[x.flat, x.N] for x in c.children] for c in kids],
                        "board": root.state})
        return out


def search(boards, R, INV, sims, Cpuct, evaluator, leaves, vl=1.0, rules=0, noise=None, noise_eps=0.0, policy_head="full"):
    """One ply on fresh trees.  noise: float32 [G][MAX_MOVES] gamma draws or None.
    Returns (rc of Model.search, Model.results() or None, counts {"collisions", "terminals", "steps": Model.steps})."""
    model = Model(boards, R, INV, Cpuct, evaluator, rules=rules, vl=vl, noise_eps=noise_eps, policy_head=policy_head)
    model.set_noise(noise)
    rc = model.search(sims, leaves)
    return rc, model.results() if rc == 0 else None, dict(model.counts, steps=model.steps)


# ---- the engine through the step-wise C-ABI -----------------------------------------------------------------------
def run_steps(eng, backend, sims, evaluator, K=1, vl=1.0, fused=True, begin=None):
    """`sims` simulations of the search in progress (after search_begin or search_advance) through the step-wise
    entry points with K leaves per step (schedule(): an int K, or a list of leaves per step), each step's count set
    through set_leaves before its selection.  begin: (roots, c_puct) of a search to begin first, once the first step's
    count is set.  evaluator: numpy callable on [rows,24,R,R]."""
    sched = schedule(sims, K)
    K = K if isinstance(K, int) else sched[0]
    eng.set_leaves(sched[0] if sched else K, vl)
    if begin is not None:
        eng.search_begin(*begin)
    run_schedule(eng, backend, sched, evaluator, fused, set_leaves=lambda k: eng.set_leaves(k, vl))
    eng.set_leaves(K, vl)


def run_stepwise(eng, backend, roots, sims, c_puct, evaluator, leaves, vl=1.0, fused=True):
    """a whole search of `roots` with `leaves` leaves per step: run_steps between search_begin and search_results"""
    run_steps(eng, backend, sims, evaluator, leaves, vl, fused, begin=(roots, c_puct))
    return eng.search_results(roots=roots)


def run_plies(eng, backend, roots, plan, evaluator, K=1, c_puct=3.0, vl=1.0, fused=True):
    """Generator over the plies of `plan`, a list of (sims, pick): ply 0 is fpc_search_begin on `roots`, every later one
    fpc_search_advance with what the previous ply's pick(res) returned -- (src_games or None, flats).  Every ply runs
    its simulations -- as many of `sims` as max_sims leaves room for beside the kept visits -- through the step-wise C-ABI
    and yields {"res", "sims", "src", "flats", "kept", "roots", "after"}: the search results, the simulations run, what the ply was advanced with, the advance's kept visit counts and root PODs ([n, 288] uint8), and
    the results read right after the advance, before any simulation."""
    eng.set_leaves(K, vl)
    eng.search_begin(roots, c_puct)
    info = {"src": None, "flats": None, "kept": None, "roots": None, "after": None}
    for ply, (sims, pick) in enumerate(plan):
        if info["kept"] is not None:                 # kept + new simulations stay within the engine's max_sims
            sims = min(sims, eng.max_sims - (int(info["kept"].max()) - 1))
        run_steps(eng, backend, sims, evaluator, K, vl, fused)
        info["sims"] = sims
        info["res"] = eng.search_results()
        yield info
        if ply + 1 == len(plan):
            return
        src, flats = pick(info["res"])
        pods = np.zeros((len(flats), fpc_ffi.BOARD_BYTES), np.uint8)
        kept = eng.search_advance(flats, src, roots_np=pods)
        info = {"src": src, "flats": list(flats), "kept": kept, "roots": pods, "after": eng.search_results()}


def results_raw(eng, max_children=256):
    """(status, results dict) of fpc_search_results without raising: a game killed by fpc_search_advance keeps its error"""
    G = eng.G
    rv = np.zeros(G, np.int32); nc = np.zeros(G, np.int32); sd = np.zeros(G, np.int32)
    cf = np.zeros((G, max_children), np.int32); cv = np.zeros((G, max_children), np.int32)
    cp = np.zeros((G, max_children), np.float32); cw = np.zeros((G, max_children), np.float64)
    pods = np.zeros((G, fpc_ffi.BOARD_BYTES), np.uint8)
    rc = eng.L.fpc_search_results(eng.h, fpc_ffi._bp(pods), rv.ctypes.data, nc.ctypes.data, sd.ctypes.data, max_children,
                                  cf.ctypes.data, cv.ctypes.data, cp.ctypes.data, cw.ctypes.data)
    return rc, {"root_n": rv, "n_children": nc, "sims_done": sd, "flat": cf, "visits": cv, "prior": cp, "w": cw,
                "boards": fpc_ffi._LazyBoards(pods)}


def pick_rule(res, stats=None):
    """The tests' moves: even games play the most-visited root child, odd games a child that was never selected
    (visits == 1) if there is one, else the least-visited.  Games whose root has no child (the game is over) are
    dropped.  Returns (src_games, flats); stats counts the kinds of pick."""
    src, flats = [], []
    for g in range(len(res["n_children"])):
        n = int(res["n_children"][g])
        if n == 0:
            continue
        vis = res["visits"][g, :n]
        if g % 2 == 0:
            k = int(np.argmax(vis))
        else:
            ones = np.nonzero(vis == 1)[0]
            k = int(ones[0]) if len(ones) else int(np.argmin(vis))
        if stats is not None:
            stats["unvisited" if vis[k] == 1 else "visited"] += 1
        src.append(g)
        flats.append(int(res["flat"][g, k]))
    return src, flats


def same_state(fb, ob):
    """an engine POD and an oracle board hold the same state, piece-list order included"""
    return (bytes(fb.sq) == bytes(ob.sq) and fpc_ffi.lists_of(fb) == orc.lists_of(ob) and fb.turn == ob.turn and
            list(fb.king) == list(ob.king) and list(fb.castle) == list(ob.castle))


def compare(eng, res, model, tag, grand_every=1):
    """engine result dict vs Model.results(), bit for bit; the second level (through grandchildren) for every
    `grand_every`-th game (0: none), under every root child the model has visited -- one that was expanded has its
    children, a terminal one has none"""
    assert len(res["root_n"]) == len(model), (tag, "games")
    for gi, o in enumerate(model):
        n = int(res["n_children"][gi])
        assert int(res["root_n"][gi]) == o["root_n"], (tag, gi, "root N")
        assert n == len(o["children"]), (tag, gi, "n_children")
        got = [[int(res["flat"][gi, k]), int(res["visits"][gi, k])] for k in range(n)]
        assert got == o["children"], (tag, gi, "children")
        assert int(res["sims_done"][gi]) == o["sims_done"], (tag, gi, "sims_done")
        assert np.array_equal(res["prior"][gi, :n], o["priors"]), (tag, gi, "priors")
        assert np.array_equal(res["w"][gi, :n], o["w"]), (tag, gi, "value sums")
        assert same_state(res["boards"][gi], o["board"]), (tag, gi, "root state")
        if grand_every and gi % grand_every == 0:
            for ci in range(n):
                if o["children"][ci][1] > 1:
                    assert eng.grandchildren(gi, ci) == o["grand"][ci], (tag, gi, ci, "second level")


def same_results(a, b, ia=None, ib=None):
    """two engine result dicts agree bit for bit on games ia of a / ib of b (None: all)"""
    ia = list(range(len(a["root_n"]))) if ia is None else ia
    ib = list(range(len(b["root_n"]))) if ib is None else ib
    assert len(ia) == len(ib)
    for k in ("root_n", "n_children", "sims_done"):
        assert np.array_equal(a[k][ia], b[k][ib]), k
    for x, y in zip(ia, ib):
        n = int(a["n_children"][x])                  # the arrays hold nothing defined past a game's children
        for k in ("flat", "visits", "prior", "w"):
            assert np.array_equal(a[k][x, :n], b[k][y, :n]), (k, x, y)
        assert bytes(a["boards"][x]) == bytes(b["boards"][y]), (x, y)


def positions(R, n, seed, near_end=False, rules=0):
    """n seeded positions from random playouts through the oracle (mid-game), or `near_end`: a few plies before the
    end of a random game, so that searches meet terminal leaves.  Returns orc boards of positions still in progress."""
    import random
    import positions as pos
    INV = {8: 2, 10: 2, 13: 3, 14: 3}[R]
    turn, entries = pos.start_entries(R)
    rng = random.Random(seed)
    out = []
    orc.set_rules(rules)
    try:
        while len(out) < n:
            b = orc.board_from_dict(R, turn, [list(e) for e in entries])
            hist = [b]
            for _ply in range(rng.randrange(0, 40) if not near_end else 800):
                if orc.game_result(orc.clone(b), R, INV) != 0:
                    break
                flats = sorted(set(x[2] for x in orc.legal_moves(b, R, INV)))
                b, rc = orc.take_action(b, R, flats[rng.randrange(len(flats))])
                assert rc == 0
                hist.append(b)
            if near_end:
                if orc.game_result(orc.clone(b), R, INV) == 0:
                    continue                         # no end within the playout: another game
                b = hist[max(0, len(hist) - 1 - rng.randrange(1, 4))]
            if orc.game_result(orc.clone(b), R, INV) == 0:
                out.append(b)
    finally:
        orc.set_rules(0)
    return out
