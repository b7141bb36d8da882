"""The plain-Python model of FPC_RULES_TERMINAL (include/fpc_engine.h): budget_model.Model -- the search of
search_model.Model with refill and optional per-game budgets -- whose terminal branch is the rule bit's.  When a descent
ends on a leaf whose GetGameResult is not in progress:
  * the value backed up (leaf first, sign alternating) is 0.0 for a stalemate, else +1.0 if the winning team (WIN_RY -> 0,
    WIN_BG -> 1) is the leaf's side-to-move team (turn & 1), else -1.0;
  * sims_done += 1, the row is dead for the step, the game's selection of the step ends there (no pending visit), and the
    game STAYS alive: it selects again in the next step, and a terminal leaf reached again backs up again;
  * a terminal ROOT takes the game out of the search as under every other rule set.
With the bit clear the branch is search_model's (0 / -1, the root leaves the search: Q5).  The oracle does not know the
bit: it is always given rules & 15.  Terminal backups are counted by kind in counts["lost"] (the side to move has no king,
or is mated), counts["won"] (its first legal move takes a king) and counts["stalemate"]; backups[g] counts game g's.
Everything else is budget_model.Model._search, line for line."""
import math

import numpy as np

import budget_model as bm
import search_model as sm
from oracle import orc

RULES_TERMINAL = 16
WIN_RY, WIN_BG, STALEMATE = 1, 2, 3


def terminal_value(res, turn):
    """the bit's value of a terminal leaf with result `res` whose side to move is `turn`"""
    if res == STALEMATE:
        return 0.0
    return 1.0 if (1 if res == WIN_BG else 0) == (turn & 1) else -1.0


class Model(bm.Model):
    def __init__(self, boards, R, INV, Cpuct, evaluator, rules=0, **kw):
        super().__init__(boards, R, INV, Cpuct, evaluator, rules=rules & 15, **kw)      # self.rules: what the oracle is given
        self.terminal = bool(rules & RULES_TERMINAL)
        self.counts.update({"lost": 0, "won": 0, "stalemate": 0})
        self.backups = [0] * len(boards)         # terminal backups per game, over the model's life (indices of the current batch)

    def advance(self, src_games, flats):
        src = list(range(len(flats))) if src_games is None else list(src_games)
        kept = super().advance(src_games, flats)
        self.backups = [self.backups[s] for s in src]
        return kept

    def advance_refill(self, src, flats, fresh):
        old = self.backups
        kept = super().advance_refill(src, flats, fresh)     # (goes through advance with the kept rows)
        full = list(range(len(flats))) if src is None else list(src)
        self.backups = [old[s] if s >= 0 else 0 for s in full]
        return kept

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
                    if res != 0:
                        turn = nd.state.turn
                        won = res != STALEMATE and (1 if res == WIN_BG else 0) == (turn & 1)
                        if self.terminal:        # value by result; only a terminal root leaves the search
                            self._backprop(path, terminal_value(res, turn))
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
                        nd.children.append(sm._Node(float(pri[j]), fl, nd))
        return 0
