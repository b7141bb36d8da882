"""The plain-Python model of fpc_search_set_budget (per-game simulation budgets; include/fpc_engine.h):
refill_model.Model whose selection is gated per game.  budget[g] caps sims_done[g], the simulations game g completes in
this search; descent k (0-based) of a step is made only while sims_done[g] + k < budget[g], with sims_done as it stands
when the step's selection starts.  A game at its budget selects nothing: its rows are None rows (dead for the step), the
game stays alive and nothing of it is touched -- so the batch-wide rotation (Q6) comes from the first row that is live.
Budgets belong to one ply: advance / advance_refill clear them.  Everything else is search_model.Model._search, line
for line."""
import math

import numpy as np

import refill_model as rm
import search_model as sm
from oracle import orc


class Model(rm.Model):
    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self.budget = None

    def set_budget(self, budget):
        """list of per-game caps on sims_done for the search in progress, or None (no budgets)"""
        if budget is not None:
            budget = [int(b) for b in budget]
            assert len(budget) == len(self.roots) and min(budget) >= 0
        self.budget = budget

    def advance(self, src_games, flats):
        self.budget = None
        return super().advance(src_games, flats)

    def advance_refill(self, src, flats, fresh):
        kept = super().advance_refill(src, flats, fresh)
        self.budget = None
        return kept

    def _search(self, sched):
        if self.budget is None:
            return super()._search(sched)
        R, INV, rules, vl, Cpuct = self.R, self.INV, self.rules, self.vl, self.Cpuct
        G = len(self.roots)
        for ks in sched:
            nrows = ks * G
            rows = [None] * nrows
            idle, cut = [], []                   # games the gate kept from selecting at all / from descent k > 0
            # ---- selection: per game, ks descents in sequence; the budget, a collision or a terminal leaf end the game's step
            for g in range(G):
                if not self.alive[g]:
                    continue
                done0 = self.sims_done[g]
                for k in range(ks):
                    if not done0 + k < self.budget[g]:       # the gate: the rest of the game's rows are dead rows
                        (cut if k else idle).append(g)
                        break
                    nd = self.roots[g]
                    path = [nd]
                    while nd.children:
                        Np = nd.N + nd.VL
                        lp, sq = math.log(math.sqrt(Np)), math.sqrt(Np)
                        best, bu = None, -math.inf
                        for ch in nd.children:
                            Nc = ch.N + ch.VL
                            if rules & sm.RULES_PUCT:
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
                        nd.children.append(sm._Node(float(pri[j]), fl, nd))
        return 0
