"""The plain-Python model of FPC_RULES_VISITS and first-play urgency (include/fpc_engine.h):
terminal_model.Model -- the search with refill, budgets and the terminal rule bit -- in which
  * with the bit (32) set every node is born with N = 0: the roots, the fresh rows of advance_refill and the children an
    expansion makes.  A node's N is then the number of backups through it, and advance / advance_refill return those
    counts (0 for a fresh row and for a child that was never visited);
  * with fpu = r (a float; None: FPC_FPU_ZERO) a child whose effective count N + VL is 0 gets q = W_p / N_p - r in the PUCT
    branch, W_p and N_p the STORED statistics of the node the descent stands on (no virtual loss), in f64 as written.  The
    strict branch keeps q = 0.
The oracle knows neither: it is given rules & 15, as in terminal_model.  Counted besides terminal_model's counts:
counts["unvisited"], the root children with N = 0 after the last search, and counts["fpu_decided"], the selections whose
argmax under FPC_FPU_PARENT differs from the argmax of the same node under FPC_FPU_ZERO.
With the bit clear and fpu None the search is terminal_model.Model's (tests/test_visits_cpu.py holds it to that).
Everything else is terminal_model.Model._search, line for line."""
import math

import numpy as np

import search_model as sm
import terminal_model as tm
from oracle import orc

RULES_VISITS = 32
STALEMATE, WIN_BG = tm.STALEMATE, tm.WIN_BG


class _Node0(sm._Node):
    """a node born with N = 0"""
    __slots__ = ()

    def __init__(self, P, flat, parent, state=None):
        super().__init__(P, flat, parent, state)
        self.N = 0


class Model(tm.Model):
    def __init__(self, boards, R, INV, Cpuct, evaluator, rules=0, fpu=None, **kw):
        super().__init__(boards, R, INV, Cpuct, evaluator, rules=rules & 31, **kw)
        self.visits = bool(rules & RULES_VISITS)
        self.fpu = None if fpu is None else float(fpu)
        self.node = _Node0 if self.visits else sm._Node
        if self.visits:
            for r in self.roots:
                r.N = 0
        self.counts.update({"unvisited": 0, "fpu_decided": 0})

    def advance_refill(self, src, flats, fresh):
        super().advance_refill(src, flats, fresh)
        full = list(range(len(flats))) if src is None else list(src)
        if self.visits:
            for r, s in zip(self.roots, full):
                if s < 0:
                    r.N = 0                      # a fresh row: born like every other node
        return [r.N for r in self.roots]

    def search(self, sims, leaves=1):
        rc = super().search(sims, leaves)
        self.counts["unvisited"] = sum(1 for r in self.roots for c in r.children if c.N == 0)
        return rc

    def _search(self, sched):
        R, INV, rules, vl, Cpuct = self.R, self.INV, self.rules, self.vl, self.Cpuct
        G = len(self.roots)
        for ks in sched:
            nrows = ks * G
            rows = [None] * nrows
            idle, cut = [], []                   # games the budget kept from selecting at all / from descent k > 0
            # ---- selection: per game, ks descents in sequence; the budget, a collision or a terminal leaf end the game's step
            for g in range(G):
                if not self.alive[g]:
                    continue
                done0 = self.sims_done[g]
                for k in range(ks):
                    if self.budget is not None and not done0 + k < self.budget[g]:
                        (cut if k else idle).append(g)
                        break
                    nd = self.roots[g]
                    path = [nd]
                    while nd.children:
                        Np = nd.N + nd.VL
                        lp, sq = math.log(math.sqrt(Np)), math.sqrt(Np)      # a node with children has N >= 1
                        q0 = nd.W / float(nd.N) - self.fpu if self.fpu is not None else 0.0     # stored W, N: no virtual loss
                        best, bu = None, -math.inf
                        zbest, zbu = None, -math.inf                         # the same argmax under FPC_FPU_ZERO
                        for ch in nd.children:
                            Nc = ch.N + ch.VL
                            if rules & sm.RULES_PUCT:
                                Wc = ch.W + vl * ch.VL
                                q = -(Wc / Nc) if Nc > 0 else q0
                                u = q + Cpuct * ch.P * sq / (1 + Nc)
                                zu = u if Nc > 0 else 0.0 + Cpuct * ch.P * sq / (1 + Nc)
                            else:
                                Wc = ch.W - vl * ch.VL
                                q = Wc / Nc if Nc > 0 else 0.0
                                u = q + Cpuct * math.sqrt(lp / (1 + Nc)) * ch.P
                                zu = u
                            if u > bu:
                                best, bu = ch, u
                            if zu > zbu:
                                zbest, zbu = ch, zu
                        if best is None:
                            return -2
                        if self.fpu is not None and best is not zbest:
                            self.counts["fpu_decided"] += 1
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
                    if res != 0:
                        turn = nd.state.turn
                        won = res != STALEMATE and (1 if res == WIN_BG else 0) == (turn & 1)
                        if self.terminal:        # value by result; only a terminal root leaves the search
                            self._backprop(path, tm.terminal_value(res, turn))
                            if nd is self.roots[g]:
                                self.alive[g] = False
                        else:                    # node.cpp:31-42, Q5
                            self._backprop(path, 0.0 if res == STALEMATE else -1.0)
                            self.alive[g] = False
                        self.sims_done[g] += 1
                        self.counts["terminals"] += 1
                        self.counts["stalemate" if res == STALEMATE else "won" if won else "lost"] += 1
                        self.backups[g] += 1
                        break
                    legal = sorted(set(m[2] for m in orc.legal_moves(nd.state, R, INV)))
                    rows[k * G + g] = (g, nd, path, legal)
                    for p in path:
                        p.VL += 1
            live = [r for r in range(nrows) if rows[r] is not None]
            self.steps.append({"rows": nrows, "dead": [r for r in range(nrows) if rows[r] is None],
                               "pairs": sum(len(rows[r][3]) for r in live),
                               "turns": [rows[r][1].state.turn for r in live],
                               "max_legal": max([len(rows[r][3]) for r in live], default=0),
                               "idle": idle, "cut": cut, "live": live,
                               "live_turns": {r: rows[r][1].state.turn for r in live}})
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
                    rot = nd.state.turn if rules & sm.RULES_ROTATION else turn0
                    prc, pri = sm._priors(logits[r], R, rot, legal, self.policy_head)
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
                        nd.children.append(self.node(float(pri[j]), fl, nd))
        return 0
