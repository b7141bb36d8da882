"""Plain-Python model of the leaf-parallel search (include/fpc_engine.h fpc_search_set_leaves; DESIGN.md
"Leaf-parallel search"): the loop of the oracle's orc_search (oracle/fpc_oracle.cpp) extended to up to K leaves per
game per simulation step, kept apart by virtual loss.

Board work goes through the oracle's primitives (orc.legal_moves / game_result / take_action / encode) and the priors
through orc_policy_priors, so that the model and the kernels meet at bit level.  Selection arithmetic is fp64 without
contraction (Python floats), the log table is math.log(math.sqrt(n)) as the host table is; f32 work (values, root
noise) is done on numpy float32 scalars.

Also here: `run_stepwise`, which drives an engine through the step-wise C-ABI the way mcts.MCTS does with K leaves.
"""
import ctypes as C
import math

import numpy as np

import fpc_ffi
from oracle import orc

RULES_PUCT, RULES_ROTATION = 1, 2


class _Node:
    __slots__ = ("N", "W", "VL", "P", "flat", "parent", "children", "state")

    def __init__(self, P, flat, parent, state=None):
        self.N, self.W, self.VL = 1, 0.0, 0      # node.h:28 default visit_count 1 (Q1)
        self.P, self.flat, self.parent = P, flat, parent
        self.children = []
        self.state = state                       # made from the parent's state the first time the node is reached


def _priors(logits_row, R, rot, legal):
    L = orc.lib()
    lg = np.ascontiguousarray(logits_row, dtype=np.float32)
    lf = np.ascontiguousarray(legal, dtype=np.int32)
    out = np.zeros(max(len(legal), 1), dtype=np.float32)
    rc = L.orc_policy_priors(lg.ctypes.data_as(C.POINTER(C.c_float)), R, rot, lf.ctypes.data_as(C.POINTER(C.c_int)),
                             len(legal), out.ctypes.data_as(C.POINTER(C.c_float)))
    return rc, out[:len(legal)]


def schedule(sims, leaves):
    """leaves per step: an int K -> ceil(sims / K) steps of K, the last one of the remainder; a list is taken as it is"""
    if not isinstance(leaves, int):
        return list(leaves)
    steps = (sims + leaves - 1) // leaves
    return [leaves if s + 1 < steps else sims - leaves * (steps - 1) for s in range(steps)]


def search(boards, R, INV, sims, Cpuct, evaluator, leaves, vl=1.0, rules=0, noise=None, noise_eps=0.0):
    """leaves: K, or a list of leaves per step (schedule()).
    boards: orc boards (mutated like the engine mutates its roots' piece lists).  evaluator: numpy callable
    enc[B,24,R,R] -> (logits[B,A], value[B]).  noise: float32 [G][MAX_MOVES] gamma draws or None.
    Returns (rc, results in orc.search's format + "grand" per root child, counts {"collisions", "terminals"});
    rc: 0, -2 (no child selectable), -3 (policy error), -4 (move failed)."""
    G = len(boards)
    orc.set_rules(rules)
    try:
        return _search(boards, G, R, INV, schedule(sims, leaves), float(Cpuct), evaluator, float(vl), rules, noise, noise_eps)
    finally:
        orc.set_rules(0)


def _search(boards, G, R, INV, sched, Cpuct, evaluator, vl, rules, noise, noise_eps):
    trees = [[_Node(0.0, -1, -1, state=boards[g])] for g in range(G)]
    alive = [True] * G
    sims_done = [0] * G
    counts = {"collisions": 0, "terminals": 0}
    rc = 0

    def backprop(t, path, v):                    # node.cpp:133-142 along the descent path: leaf +v, parent -v, ...
        v = np.float32(v)
        for n in reversed(path):
            t[n].W += float(v)
            t[n].N += 1
            v = -v

    for ks in sched:
        nrows = ks * G
        rows = [None] * nrows
        # ---- selection: per game, ks descents in sequence; collision / terminal leaf end the game's step
        for g in range(G):
            if not alive[g]:
                continue
            t = trees[g]
            for k in range(ks):
                n, path = 0, [0]
                while t[n].children:
                    nd = t[n]
                    Np = nd.N + nd.VL
                    lp, sq = math.log(math.sqrt(Np)), math.sqrt(Np)
                    best, bu = -1, -math.inf
                    for i, ci in enumerate(nd.children):
                        ch = t[ci]
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
                            best, bu = i, u
                    if best < 0:
                        return -2, None, counts
                    n = nd.children[best]
                    path.append(n)
                if t[n].VL > 0:                  # collision: nothing is touched
                    counts["collisions"] += 1
                    break
                if t[n].state is None:
                    st, mrc = orc.take_action(t[t[n].parent].state, R, t[n].flat)
                    if mrc != 0:
                        return -4, None, counts
                    t[n].state = st
                res = orc.game_result(t[n].state, R, INV)
                if res != 0:                     # node.cpp:31-42, Q5
                    backprop(t, path, 0.0 if res == 3 else -1.0)
                    sims_done[g] += 1
                    alive[g] = False
                    counts["terminals"] += 1
                    break
                legal = sorted(set(m[2] for m in orc.legal_moves(t[n].state, R, INV)))
                rows[k * G + g] = (g, n, path, legal)
                for p in path:
                    t[p].VL += 1
        live = [r for r in range(nrows) if rows[r] is not None]
        if not live:
            continue
        # ---- evaluation of rows 0 .. ks*G-1, dead rows all-zero
        states = [trees[rows[r][0]][rows[r][1]].state for r in live]
        enc = np.zeros((nrows, 24, R, R), dtype=np.float32)
        enc[live] = orc.encode(states, R)        # rotation: the first live row's turn (Q6) or each row's own
        logits, value = evaluator(enc)
        logits = np.asarray(logits, dtype=np.float32).reshape(nrows, -1)
        value = np.asarray(value, dtype=np.float32).reshape(nrows)
        turn0 = states[0].turn
        # ---- expansion: per game, live rows in ascending k
        for g in range(G):
            t = trees[g]
            for k in range(ks):
                row = rows[k * G + g]
                if row is None:
                    continue
                _, n, path, legal = row
                r = k * G + g
                rot = t[n].state.turn if rules & RULES_ROTATION else turn0
                prc, pri = _priors(logits[r], R, rot, legal)
                if prc:
                    return -3, None, counts
                if noise is not None and n == 0:
                    gm = np.asarray(noise[g], dtype=np.float32)
                    sg = np.float32(0)
                    for j in range(len(legal)):
                        sg = np.float32(sg + gm[j])
                    if sg > 0:
                        one, eps = np.float32(1), np.float32(noise_eps)
                        for j in range(len(legal)):
                            pri[j] = np.float32((one - eps) * pri[j]) + np.float32(eps * np.float32(gm[j] / sg))
                backprop(t, path, value[r])
                for p in path:
                    t[p].VL -= 1
                sims_done[g] += 1
                for j, fl in enumerate(legal):
                    if pri[j] == 0:
                        continue                 # torch.nonzero drops exact zeros
                    t.append(_Node(float(pri[j]), fl, n))
                    t[n].children.append(len(t) - 1)
    out = []
    for g in range(G):
        t = trees[g]
        kids = [t[c] for c in t[0].children]
        out.append({"root_n": t[0].N, "terminated": not alive[g], "sims_done": sims_done[g],
                    "children": [[c.flat, c.N] for c in kids],
                    "priors": np.array([c.P for c in kids], dtype=np.float32),
                    "w": np.array([c.W for c in kids], dtype=np.float64),
                    "grand": [[[t[x].flat, t[x].N] for x in c.children] for c in kids],
                    "board": t[0].state})
    return rc, out, counts


def run_stepwise(eng, backend, roots, sims, c_puct, evaluator, leaves, vl=1.0, fused=True):
    """The step-wise C-ABI driven with `leaves` leaves per step (schedule(): an int K, or a list of leaves per step),
    each step's count set through set_leaves before its selection.  evaluator: numpy callable on [rows,24,R,R]."""
    G, R = len(roots), eng.R
    sched = schedule(sims, leaves)
    steps = len(sched)
    K = sched[0] if isinstance(leaves, (list, tuple)) else leaves

    def k_of(s):
        return sched[s]

    eng.set_leaves(k_of(0) if steps else K, vl)
    eng.search_begin(roots, c_puct)
    keep = []
    n_live, enc_ptr = eng.search_select() if steps else (0, None)
    for s in range(steps):
        last = s == steps - 1
        rows = k_of(s) * G
        if not last:
            eng.set_leaves(k_of(s + 1), vl)
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
    return eng.search_results(roots=roots)


def compare(eng, res, model, tag, grand=True):
    """engine result dict (+ second level through grandchildren) vs the model, bit for bit"""
    for gi, o in enumerate(model):
        n = int(res["n_children"][gi])
        assert int(res["root_n"][gi]) == o["root_n"], (tag, gi, "root N")
        got = [[int(res["flat"][gi, k]), int(res["visits"][gi, k])] for k in range(n)]
        assert got == o["children"], (tag, gi, "children")
        assert int(res["sims_done"][gi]) == o["sims_done"], (tag, gi, "sims_done")
        assert np.array_equal(res["prior"][gi, :n], o["priors"]), (tag, gi, "priors")
        assert np.array_equal(res["w"][gi, :n], o["w"]), (tag, gi, "value sums")
        assert fpc_ffi.lists_of(res["boards"][gi]) == orc.lists_of(o["board"]), (tag, gi, "root list order")
        if grand:
            for ci in range(n):
                if o["children"][ci][1] > 1:
                    assert eng.grandchildren(gi, ci) == o["grand"][ci], (tag, gi, ci, "second level")


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
