"""The plain-Python model of forced playouts and policy target pruning at the root (fpc_search_set_forced /
fpc_search_targets; include/fpc_engine.h): solver_model.Model -- the search with refill, budgets, the
terminal rule bit, FPC_RULES_VISITS, first-play urgency and the solver -- plus forced=<factor>.  Forcing is IN EFFECT only with
a factor > 0 under a rule set that holds both FPC_RULES_PUCT and FPC_RULES_VISITS (forced_in_effect(); in_effect() stays the
solver's rule, which pick() and the solver's steps read).  Then
  * at the ROOT level of a descent a child with 0 < N' < sqrt(factor * P * N'_root) gets u = +infinity; the argmax, the
    solver's exclusion and everything after the choice are as they are (counts["forced_decided"]: the root selections whose
    argmax differs from the argmax of the same node without the rule);
  * targets() reports, and pick() draws from, the pruned visit counts of `targets(N_p, N, W, P, C, factor)` below, which
    is the header's block line for line (counts["pruned_visits"], counts["pruned_to_zero"]: over the roots' children
    after the last search, the visits taken out and the children with N > 0 whose target is 0).
Python floats are f64 and nothing is contracted; math.sqrt is the correctly rounded square root the device's is.
With forcing not in effect the search is solver_model.Model's (tests/test_forced_cpu.py holds it to that).  Everything
else is solver_model.Model._search, line for line, with the solver's four steps under `solving`."""
import math

import numpy as np

import search_model as sm
import solver_model as so
import terminal_model as tm
from oracle import orc

RULES_VISITS = 32
STALEMATE, WIN_BG = tm.STALEMATE, tm.WIN_BG
UNKNOWN, WIN = so.UNKNOWN, so.WIN


def targets(N_p, N, W, P, C, factor):
    """the pruned visit counts T_k of a root with stored count N_p whose children have stored N, W, P (tree order)"""
    n = len(N)
    if n == 0:
        return []
    b = 0
    for k in range(1, n):
        if N[k] > N[b]:
            b = k
    T_all = [int(x) for x in N]
    if N[b] == 0:
        return T_all
    sq = math.sqrt(float(N_p))
    ub = -(W[b] / float(N[b])) + C * float(P[b]) * sq / float(1 + N[b])
    for k in range(n):
        if k == b:
            continue
        T = int(N[k])
        if N[k] > 0:
            F = int(math.sqrt(factor * float(P[k]) * float(N_p)))
            q = -(W[k] / float(N[k]))
            a = C * float(P[k]) * sq
            for _ in range(F):
                if T == 0 or q + a / float(T) >= ub:
                    break
                T = T - 1
            if T < N[k] and T <= 1:
                T = 0
        T_all[k] = T
    return T_all


class Model(so.Model):
    def __init__(self, boards, R, INV, Cpuct, evaluator, rules=0, fpu=None, solver=False, forced=0.0, **kw):
        super().__init__(boards, R, INV, Cpuct, evaluator, rules=rules, fpu=fpu, solver=solver, **kw)
        self.forced = float(forced)
        self.counts.update({"forced_decided": 0, "pruned_visits": 0, "pruned_to_zero": 0})

    def forced_in_effect(self):
        return self.forced > 0 and self.visits and bool(self.rules & sm.RULES_PUCT)

    def targets(self):
        """what fpc_search_targets reports: per game the children's pruned counts (the stored ones when not in effect)"""
        out = []
        for r in self.roots:
            kids = r.children
            if self.forced_in_effect():
                out.append(targets(r.N, [c.N for c in kids], [c.W for c in kids], [c.P for c in kids], self.Cpuct, self.forced))
            else:
                out.append([c.N for c in kids])
        return out

    def search(self, sims, leaves=1):
        rc = super().search(sims, leaves)
        pv = pz = 0
        for r, T in zip(self.roots, self.targets()):
            for c, t in zip(r.children, T):
                pv += c.N - t
                pz += 1 if c.N > 0 and t == 0 else 0
        self.counts["pruned_visits"], self.counts["pruned_to_zero"] = pv, pz
        return rc

    def pick(self, g, temperature, uniform):
        """index of the root child fpc_search_play plays for game g: the solver's pick, else the draw from the targets"""
        root = self.roots[g]
        if not root.children:
            return None
        rs = self.status(root) if self.in_effect() else UNKNOWN
        return so.sample_pick([c.flat for c in root.children], self.targets()[g], rs,
                              [self.status(c) for c in root.children], temperature, uniform)

    # ---- the search -------------------------------------------------------------------------------------------------
    def _search(self, sched):
        if not self.forced_in_effect():
            return super()._search(sched)
        solving = self.in_effect()
        R, INV, rules, vl, Cpuct = self.R, self.INV, self.rules, self.vl, self.Cpuct
        G = len(self.roots)
        S = self.S
        factor = self.forced
        for ks in sched:
            nrows = ks * G
            rows = [None] * nrows
            idle, cut, proven_idle = [], [], []
            # ---- selection: per game, ks descents in sequence; the budget, a collision, a terminal leaf or a proof end the game's step
            for g in range(G):
                if not self.alive[g]:
                    continue
                done0 = self.sims_done[g]
                for k in range(ks):
                    if self.budget is not None and not done0 + k < self.budget[g]:
                        (cut if k else idle).append(g)
                        break
                    nd = self.roots[g]
                    if solving and nd.children and nd in S:      # 1. a proven root: a dead row, nothing is written
                        assert k == 0
                        self.counts["idle_proven"] += 1
                        proven_idle.append(g)
                        break
                    path = [nd]
                    proven = False
                    while nd.children:
                        assert not solving or nd not in S
                        at_root = nd is self.roots[g]
                        Np = nd.N + nd.VL
                        sq = math.sqrt(Np)
                        q0 = nd.W / float(nd.N) - self.fpu if self.fpu is not None else 0.0     # stored W, N: no virtual loss
                        best, bu = None, -math.inf
                        pbest, pbu = None, -math.inf                         # the same argmax without the forced rule
                        for ch in nd.children:
                            if solving and S.get(ch, UNKNOWN) == WIN:      # 2. the move that loses is no candidate
                                self.counts["excluded"] += 1
                                continue
                            Nc = ch.N + ch.VL
                            Wc = ch.W + vl * ch.VL
                            q = -(Wc / Nc) if Nc > 0 else q0
                            u = q + Cpuct * ch.P * sq / (1 + Nc)
                            pu = u
                            if at_root and Nc > 0 and float(Nc) < math.sqrt(factor * ch.P * float(Np)):
                                u = math.inf             # the forced playout
                            if u > bu:
                                best, bu = ch, u
                            if pu > pbu:
                                pbest, pbu = ch, pu
                        if best is None:
                            return -2
                        if best is not pbest:
                            self.counts["forced_decided"] += 1
                        nd = best
                        path.append(nd)
                        if solving and nd in S:      # 3. the descent ends on a proven child
                            proven = True
                            break
                    if proven:
                        assert nd.VL == 0
                        self._backprop(path, so.PV[S[nd]])
                        self.sims_done[g] += 1
                        self.counts["proven_backups"] += 1
                        if nd.children:
                            self.counts["proven_backups_interior"] += 1
                        break
                    if nd.VL > 0:                    # collision: nothing is touched
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
                            v = tm.terminal_value(res, turn)
                            self._backprop(path, v)
                            if nd is self.roots[g]:
                                self.alive[g] = False
                        else:                    # node.cpp:31-42, Q5
                            v = 0.0 if res == STALEMATE else -1.0
                            self._backprop(path, v)
                            self.alive[g] = False
                        self.sims_done[g] += 1
                        self.counts["terminals"] += 1
                        self.counts["stalemate" if res == STALEMATE else "won" if won else "lost"] += 1
                        self.backups[g] += 1
                        if solving:
                            self._prove(nd, v)       # 4.
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
                               "idle": idle, "cut": cut, "live": live, "proven_idle": proven_idle,
                               "live_turns": {r: rows[r][1].state.turn for r in live}})
            if proven_idle and live:
                self.counts["idle_while_expanding"] += 1
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
