"""The plain-Python model of playout cap randomization (fpc_search_set_fast_rows; include/fpc_engine.h):
forced_model.Model plus set_fast(mask).  For a game g with mask[g] == 1
  * the forced-playout rule is not applied at the root level of g's descents, at any leaf of a leaf-parallel step;
  * targets() reports, and pick() draws from, the stored visit counts N_k;
everything else, and every game with mask[g] == 0, is forced_model.Model's.  The mask belongs to one ply: advance and
advance_refill clear it.  Noise is not the mask's business: a fast game is noised like any other unless its gamma row is zero.
decided[g]: the root selections of game g that the forced rule decided (forced_model's counts["forced_decided"], per game);
withheld[g]: the root selections of a FAST game g whose argmax would have been another child had the rule been applied.
_search is forced_model.Model._search line for line, with the gate and the two counters."""
import math

import numpy as np

import forced_model as fm
import search_model as sm
import solver_model as so
import terminal_model as tm
from oracle import orc

STALEMATE, WIN_BG = tm.STALEMATE, tm.WIN_BG
UNKNOWN, WIN = so.UNKNOWN, so.WIN


class Model(fm.Model):
    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self.fast = None
        self.decided = [0] * len(self.roots)
        self.withheld = [0] * len(self.roots)

    def set_fast(self, mask):
        """mask: one 0 / 1 per game, or None (fpc_search_set_fast_rows)"""
        if mask is not None:
            assert len(mask) == len(self.roots) and all(int(m) in (0, 1) for m in mask)
            mask = [int(m) for m in mask]
        self.fast = mask
        self.decided = [0] * len(self.roots)
        self.withheld = [0] * len(self.roots)

    def is_fast(self, g):
        return self.fast is not None and bool(self.fast[g])

    def targets(self):
        out = super().targets()
        for g, r in enumerate(self.roots):
            if self.is_fast(g):
                out[g] = [c.N for c in r.children]
        return out

    def advance(self, src_games, flats):
        kept = super().advance(src_games, flats)
        self.set_fast(None)
        return kept

    def advance_refill(self, src, flats, fresh):
        kept = super().advance_refill(src, flats, fresh)
        self.set_fast(None)
        return kept

    # ---- the search -------------------------------------------------------------------------------------------------
    def _search(self, sched):
        if not self.forced_in_effect() or self.fast is None or not any(self.fast):
            return super()._search(sched)            # no fast row, or nothing to gate: the forced model's search
        fast = self.fast
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
                        fbest, fbu = None, -math.inf                         # ... and with it, for a fast game
                        for ch in nd.children:
                            if solving and S.get(ch, UNKNOWN) == WIN:      # 2. the move that loses is no candidate
                                self.counts["excluded"] += 1
                                continue
                            Nc = ch.N + ch.VL
                            Wc = ch.W + vl * ch.VL
                            q = -(Wc / Nc) if Nc > 0 else q0
                            u = q + Cpuct * ch.P * sq / (1 + Nc)
                            pu = fu = u
                            if at_root and Nc > 0 and float(Nc) < math.sqrt(factor * ch.P * float(Np)):
                                if fast[g]:
                                    fu = math.inf        # a fast game: the rule is not applied; what it would have done
                                else:
                                    u = math.inf         # the forced playout
                            if u > bu:
                                best, bu = ch, u
                            if pu > pbu:
                                pbest, pbu = ch, pu
                            if fu > fbu:
                                fbest, fbu = ch, fu
                        if best is None:
                            return -2
                        if best is not pbest:
                            self.counts["forced_decided"] += 1
                            self.decided[g] += 1
                        if fast[g] and fbest is not best:
                            self.withheld[g] += 1
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
