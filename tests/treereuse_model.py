"""Plain-Python model of subtree reuse (include/fpc_engine.h fpc_search_advance): the search of
tests/leafpar_model.py on trees that PERSIST from ply to ply.  `Model.search` runs simulations on the trees as they are,
`Model.advance` re-roots every kept game on the root child that was played: the child's object subtree is kept as it is
(statistics, priors, children's order, every state already made), the state of a child that was never selected is made
with orc.take_action and nothing else, an already expanded new root gets the root noise.

Board work goes through the oracle's primitives and the priors through orc_policy_priors, as in leafpar_model.

Also here: `run_plies`, which drives an engine ply by ply through the step-wise C-ABI (fpc_search_begin once, then
fpc_search_advance), the pick rule of the tests, and the comparison helpers.
"""
import ctypes as C
import math

import numpy as np

import fpc_ffi
import leafpar_model as lm
from oracle import orc

RULES_PUCT, RULES_ROTATION = lm.RULES_PUCT, lm.RULES_ROTATION


class Model:
    def __init__(self, boards, R, INV, Cpuct, evaluator, rules=0, vl=1.0, noise_eps=0.0):
        self.R, self.INV, self.Cpuct, self.ev, self.rules, self.vl = R, INV, float(Cpuct), evaluator, rules, float(vl)
        self.noise, self.noise_eps = None, noise_eps
        self.roots = [lm._Node(0.0, -1, None, state=b) for b in boards]      # parent / children hold node OBJECTS here
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
    def _backprop(path, v):
        v = np.float32(v)
        for nd in reversed(path):
            nd.W += float(v)
            nd.N += 1
            v = -v

    def search(self, sims, leaves=1):
        """`sims` more simulations on the trees as they stand; rc as leafpar_model.search"""
        orc.set_rules(self.rules)
        try:
            return self._search(lm.schedule(sims, leaves))
        finally:
            orc.set_rules(0)

    def _search(self, sched):
        R, INV, rules, vl, Cpuct = self.R, self.INV, self.rules, self.vl, self.Cpuct
        G = len(self.roots)
        for ks in sched:
            nrows = ks * G
            rows = [None] * nrows
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
                    if nd.VL > 0:
                        self.counts["collisions"] += 1
                        break
                    if nd.state is None:
                        st, mrc = orc.take_action(nd.parent.state, R, nd.flat)
                        if mrc != 0:
                            return -4
                        nd.state = st
                    res = orc.game_result(nd.state, R, INV)
                    if res != 0:
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
            if not live:
                continue
            states = [rows[r][1].state for r in live]
            enc = np.zeros((nrows, 24, R, R), dtype=np.float32)
            enc[live] = orc.encode(states, R)
            logits, value = self.ev(enc)
            logits = np.asarray(logits, dtype=np.float32).reshape(nrows, -1)
            value = np.asarray(value, dtype=np.float32).reshape(nrows)
            turn0 = states[0].turn
            for g in range(G):
                for k in range(ks):
                    row = rows[k * G + g]
                    if row is None:
                        continue
                    _, nd, path, legal = row
                    r = k * G + g
                    rot = nd.state.turn if rules & RULES_ROTATION else turn0
                    prc, pri = lm._priors(logits[r], R, rot, legal)
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
                            continue
                        nd.children.append(lm._Node(float(pri[j]), fl, nd))
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


# ---- the engine, ply by ply ---------------------------------------------------------------------------------------
def run_steps(eng, backend, sims, evaluator, K=1, vl=1.0, fused=True):
    """`sims` simulations of the search in progress (after search_begin or search_advance) through the step-wise
    entry points with K leaves per step -- leafpar_model.run_stepwise without its search_begin / search_results"""
    G, R = eng.G, eng.R
    sched = lm.schedule(sims, K)
    steps = len(sched)
    eng.set_leaves(sched[0] if steps else K, vl)
    keep = []
    n_live, enc_ptr = eng.search_select() if steps else (0, None)
    for s in range(steps):
        last = s == steps - 1
        rows = sched[s] * G
        if not last:
            eng.set_leaves(sched[s + 1], vl)
        if n_live == 0:
            if not last:
                n_live, enc_ptr = eng.search_select()
            continue
        if backend == "emul":
            enc = np.ctypeslib.as_array(C.cast(enc_ptr, C.POINTER(C.c_float)), shape=(rows, 24, R, R))
            lg, v = evaluator(enc.copy())
            lg = np.ascontiguousarray(lg, dtype=np.float32)
            v = np.ascontiguousarray(v, dtype=np.float32)
            keep = [lg, v]
            lp, vp = lg.ctypes.data, v.ctypes.data
        else:
            import torch
            from fpc_testlib import DevPtr
            enc = torch.as_tensor(DevPtr(enc_ptr, (rows, 24, R, R)), device="cuda").cpu().numpy()
            lg, v = evaluator(enc)
            lg_t = torch.from_numpy(np.ascontiguousarray(lg, dtype=np.float32)).cuda()
            v_t = torch.from_numpy(np.ascontiguousarray(v, dtype=np.float32)).cuda()
            torch.cuda.synchronize()
            keep = [lg_t, v_t]
            lp, vp = lg_t.data_ptr(), v_t.data_ptr()
        if fused and not last:
            n_live, enc_ptr = eng.search_expand_select(lp, vp)
        else:
            eng.search_expand(lp, vp)
            if not last:
                n_live, enc_ptr = eng.search_select()
        if backend != "emul":
            import torch
            torch.cuda.synchronize()
    del keep
    eng.set_leaves(K, vl)


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


def compare(eng, res, model, tag, grand_every=5):
    """engine results vs Model.results(), bit for bit; the second level for every `grand_every`-th game"""
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
                if o["grand"][ci]:
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
