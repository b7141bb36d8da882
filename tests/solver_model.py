"""The plain-Python model of the MCTS solver (fpc_search_set_solver; include/fpc_engine.h):
visits_model.Model -- the search with refill, budgets, the terminal rule bit, FPC_RULES_VISITS and first-play urgency -- in
which every node carries a proof status seen from its own side to move (UNKNOWN 0, WIN 1, LOSS 2, DRAW 3).  The solver is
IN EFFECT only with solver=True under a rule set that holds both FPC_RULES_PUCT and FPC_RULES_TERMINAL; then one descent of
game g is
  1. a root with children and a status: the row is dead, nothing is touched (counts["idle_proven"], steps[-1]["proven_idle"]);
  2. a child with status WIN is no candidate of the argmax (counts["excluded"]);
  3. a chosen child with a status ends the descent: pv(status) is backed up from it, sims_done += 1, the game's selection
     of the step ends (counts["proven_backups"], ["proven_backups_interior"] where that node has children);
  4. an unknown leaf whose game is over makes the terminal backup, takes its status from the value backed up and the proof
     is propagated towards the root (_prove).
counts["proven"][(kind, origin)]: nodes proven by kind (1, 2, 3) and origin ("terminal", "loss_child", "scan").
Statuses live in a dict keyed by the node objects, so advance / advance_refill carry them with the subtrees; a fresh row
has none.  With the solver not in effect the search is visits_model.Model's (tests/test_solver_cpu.py holds it to that).
Everything else is visits_model.Model._search, line for line."""
import math

import numpy as np

import search_model as sm
import terminal_model as tm
import visits_model as vm
from oracle import orc

UNKNOWN, WIN, LOSS, DRAW = 0, 1, 2, 3
PV = {WIN: 1.0, LOSS: -1.0, DRAW: 0.0}
STALEMATE, WIN_BG = tm.STALEMATE, tm.WIN_BG


def status_of_value(v):
    return WIN if v > 0 else LOSS if v < 0 else DRAW


def sample_pick(flats, visits, root_status, child_status, temperature, u):
    """the pick rule of fpc_search_play with the solver in effect: the index of the child played"""
    import selfplay
    if root_status == WIN:
        return list(child_status).index(LOSS)
    if root_status == DRAW:
        return list(child_status).index(DRAW)
    flat = selfplay.sample_move(list(range(len(flats))), visits, temperature, u)      # today's draw, over child indices
    return int(flat)


class Model(vm.Model):
    def __init__(self, boards, R, INV, Cpuct, evaluator, rules=0, fpu=None, solver=False, **kw):
        super().__init__(boards, R, INV, Cpuct, evaluator, rules=rules, fpu=fpu, **kw)
        self.solver = bool(solver)
        self.S = {}                                  # node object -> status (absent: UNKNOWN)
        self.counts.update({"proven_backups": 0, "proven_backups_interior": 0, "excluded": 0, "idle_proven": 0,
                            "idle_while_expanding": 0, "proven": {}})

    # ---- statuses ---------------------------------------------------------------------------------------------------
    def in_effect(self):
        return self.solver and self.terminal and bool(self.rules & sm.RULES_PUCT)

    def status(self, nd):
        return self.S.get(nd, UNKNOWN)

    def _set(self, nd, st, origin):
        assert nd not in self.S                      # a status never changes once it is set
        self.S[nd] = st
        key = (st, origin)
        self.counts["proven"][key] = self.counts["proven"].get(key, 0) + 1

    def _prove(self, leaf, v):
        """step 4: the leaf's status from the value backed up, then upwards"""
        if leaf in self.S:                           # a childless proven root (after an advance): nothing changes
            return
        self._set(leaf, status_of_value(v), "terminal")
        c = leaf
        while True:
            p = c.parent
            if p is None or p in self.S:
                return
            if self.S[c] == LOSS:
                self._set(p, WIN, "loss_child")
            else:
                sts = [self.status(x) for x in p.children]
                if UNKNOWN in sts:
                    return
                self._set(p, LOSS if all(s == WIN for s in sts) else DRAW, "scan")
            c = p

    def proofs(self):
        """what fpc_search_proofs reports: (root statuses, per game the children's statuses in child order)"""
        return [self.status(r) for r in self.roots], [[self.status(c) for c in r.children] for r in self.roots]

    def check_invariants(self):
        """(a) an unknown node with children has an unknown child; a proven WIN has a LOSS child, a proven LOSS only WIN
        children, a proven DRAW no LOSS child, none unknown and a DRAW child"""
        stack = list(self.roots)
        while stack:
            nd = stack.pop()
            stack.extend(nd.children)
            if not nd.children:
                continue
            sts = [self.status(c) for c in nd.children]
            st = self.status(nd)
            if st == UNKNOWN:
                assert UNKNOWN in sts and LOSS not in sts, sts
            elif st == WIN:
                assert LOSS in sts
            elif st == LOSS:
                assert all(s == WIN for s in sts)
            else:
                assert UNKNOWN not in sts and LOSS not in sts and DRAW in sts

    def pick(self, g, temperature, uniform):
        """index of the root child fpc_search_play plays for game g (None: no child / dead game's -1)"""
        root = self.roots[g]
        if not root.children:
            return None
        rs = self.status(root) if self.in_effect() else UNKNOWN
        return sample_pick([c.flat for c in root.children], [c.N for c in root.children], rs,
                           [self.status(c) for c in root.children], temperature, uniform)

    def advance(self, src_games, flats):
        kept = super().advance(src_games, flats)
        self._prune()
        return kept

    def advance_refill(self, src, flats, fresh):
        kept = super().advance_refill(src, flats, fresh)
        self._prune()
        return kept

    def _prune(self):
        """the statuses of the nodes that are still in a tree (the rest of the old trees is dropped)"""
        keep, stack = {}, list(self.roots)
        while stack:
            nd = stack.pop()
            stack.extend(nd.children)
            if nd in self.S:
                keep[nd] = self.S[nd]
        self.S = keep

    # ---- the search -------------------------------------------------------------------------------------------------
    def _search(self, sched):
        if not self.in_effect():
            return super()._search(sched)
        R, INV, rules, vl, Cpuct = self.R, self.INV, self.rules, self.vl, self.Cpuct
        G = len(self.roots)
        S = self.S
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
                    if nd.children and nd in S:      # 1. a proven root: a dead row, nothing is written
                        assert k == 0                # invariant (c): a proof ends the game's selection of the step
                        self.counts["idle_proven"] += 1
                        proven_idle.append(g)
                        break
                    path = [nd]
                    proven = False
                    while nd.children:
                        assert nd not in S           # invariant (b): a proven node is never descended through
                        Np = nd.N + nd.VL
                        sq = math.sqrt(Np)
                        q0 = nd.W / float(nd.N) - self.fpu if self.fpu is not None else 0.0     # stored W, N: no virtual loss
                        best, bu = None, -math.inf
                        for ch in nd.children:
                            if S.get(ch, UNKNOWN) == WIN:      # 2. the move that loses is no candidate
                                self.counts["excluded"] += 1
                                continue
                            Nc = ch.N + ch.VL
                            Wc = ch.W + vl * ch.VL
                            q = -(Wc / Nc) if Nc > 0 else q0
                            u = q + Cpuct * ch.P * sq / (1 + Nc)
                            if u > bu:
                                best, bu = ch, u
                        if best is None:
                            return -2
                        nd = best
                        path.append(nd)
                        if nd in S:                  # 3. the descent ends on a proven child
                            proven = True
                            break
                    if proven:
                        assert nd.VL == 0            # invariant (c)
                        self._backprop(path, PV[S[nd]])
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
                        v = tm.terminal_value(res, turn)
                        self._backprop(path, v)
                        if nd is self.roots[g]:
                            self.alive[g] = False
                        self.sims_done[g] += 1
                        self.counts["terminals"] += 1
                        self.counts["stalemate" if res == STALEMATE else "won" if won else "lost"] += 1
                        self.backups[g] += 1
                        self._prove(nd, v)           # 4.
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
            # ---- expansion: per game, live rows in ascending k (rows pending below a node proven later in the step included)
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


def negamax(model, nd):
    """the exhaustive value of `nd` over the model's OWN tree, from nd's side to move: +1 / -1 / 0, or None where the tree
    does not decide it.  A childless node counts only with a status of origin terminal (its game is over); an interior
    node is a win with a child that is lost, a loss with every child won, a draw when every child is decided and no
    child is lost -- otherwise undecided."""
    if not nd.children:
        st = model.status(nd)
        return None if st == UNKNOWN else PV[st]
    vals = [negamax(model, c) for c in nd.children]
    if any(v == -1.0 for v in vals):
        return 1.0
    if any(v is None for v in vals):
        return None
    return -1.0 if all(v == 1.0 for v in vals) else 0.0
