"""Live-row numbering (fpc_search_set_live_rows; include/fpc_engine.h): the cases that run both on the
wavefront emulator (tests/test_live_rows_emul.py) and on the GPU (tests/test_live_rows_gpu.py) through the step entry
points, with evaluators.make("hash", R) -- a row-wise function of the encodings.  The same search runs with the switch
off and on: the trees must be the same, and only where a leaf lies in the evaluator's batch may differ.

Dead rows are made BY CONSTRUCTION: budget[g] == 0 selects nothing (fpc_search_set_budget), and the root positions meet
no terminal leaf within the few steps of a case (asserted: every case states the live rows it meant to produce).  With the
switch on the evaluator's outputs are handed over in buffers of exactly n_live rows.  Everything is compared exactly."""
import ctypes as C

import numpy as np
import pytest

import evaluators
import search_model as sm
import terminal_cases as tc
import terminal_model as tm
from fpc_testlib import DevPtr, make_engine, roots_of
from oracle import orc

R, INV = 8, 2


# ---- the step entry points, the switch on or off ----------------------------------------------------------------------
def _enc_of(backend, ptr, rows):
    if backend == "emul":
        return np.ctypeslib.as_array(C.cast(ptr, C.POINTER(C.c_float)), shape=(rows, 24, R, R)).copy()
    import torch
    return torch.as_tensor(DevPtr(ptr, (rows, 24, R, R)), device="cuda").cpu().numpy()


def drive(eng, backend, sched, ev, on, vl=1.0):
    """The steps of `sched` (leaves per game, one entry per step) of the search in progress, expansion and next selection
    in one call.  Returns one (n_live, enc [rows,24,R,R]) per step.  on: the evaluator sees enc[:n_live] and its outputs
    live in buffers of n_live rows; off: all `rows` rows, as ever."""
    G = eng.G
    recs = []
    eng.set_leaves(sched[0], vl)
    n_live, ptr = eng.search_select()
    for s, k in enumerate(sched):
        last = s == len(sched) - 1
        rows = k * G
        enc = _enc_of(backend, ptr, rows)
        recs.append((n_live, enc))
        if not last:
            eng.set_leaves(sched[s + 1], vl)
        if n_live == 0:
            if not last:
                n_live, ptr = eng.search_select()
            continue
        n_eval = n_live if on else rows
        lg, v = ev(enc[:n_eval])
        lg, v = np.ascontiguousarray(lg, np.float32), np.ascontiguousarray(v, np.float32)
        assert lg.shape == (n_eval, eng.A) and v.shape == (n_eval,)
        if backend == "emul":
            lp, vp = lg.ctypes.data, v.ctypes.data
        else:
            import torch
            lg, v = torch.from_numpy(lg).cuda(), torch.from_numpy(v).cuda()
            torch.cuda.synchronize()
            lp, vp = lg.data_ptr(), v.data_ptr()
        if last:
            eng.search_expand(lp, vp)
        else:
            n_live, ptr = eng.search_expand_select(lp, vp)
        if backend != "emul":
            torch.cuda.synchronize()
    eng.set_leaves(sched[0], vl)
    return recs


def grand_of(eng, res):
    """the second level under every root child that was visited"""
    return [[eng.grandchildren(g, c) if int(res["visits"][g, c]) > 1 else None for c in range(int(res["n_children"][g]))]
            for g in range(len(res["root_n"]))]


def one_ply(eng, backend, on, sched, budget, ev):
    """budgets, the steps, the results and the second level of the search that has just been begun or advanced"""
    eng.set_live_rows(on)                       # between begin / advance and the first selection
    if budget is not None:
        eng.search_set_budget(budget)
    recs = drive(eng, backend, sched, ev, on)
    res = eng.search_results()
    return res, grand_of(eng, res), recs


def same_search(a, b):
    (ra, ga, _), (rb, gb, _) = a, b
    sm.same_results(ra, rb)
    assert ga == gb


def check_layout(off, on, rows_of_step, want_live=None):
    """step by step: the same n_live; the on-run's row j is the off-run's j-th live row in ascending order, its rows
    n_live.. are zero.  want_live(step) -> the live rows the case meant to produce (None: not stated)."""
    assert len(off) == len(on) == len(rows_of_step)
    seen = []
    for s, ((n0, e0), (n1, e1)) in enumerate(zip(off, on)):
        assert e0.shape[0] == e1.shape[0] == rows_of_step[s]
        live = [r for r in range(e0.shape[0]) if e0[r].any()]          # a leaf's encoding holds its pieces: never all-zero
        assert n0 == n1 == len(live), (s, n0, n1, len(live))
        if want_live is not None:
            assert live == want_live(s), (s, live)
        assert np.array_equal(e1[:n1], e0[live]), s
        assert not e1[n1:].any(), s
        seen.append(live)
    return seen


# ---- 1. the layout, K = 1, patterns by budget zeros ---------------------------------------------------------------------
STEPS = 4
PATTERNS = {                                    # G, the rows with budget > 0
    "one-live": (1, [0]),
    "one-dead": (1, []),                        # n_live == 0 at every step: nothing is evaluated
    "64-last": (64, [63]),
    "65-ends": (65, [0, 64]),                   # the second scan chunk holds one live row
    "65-all": (65, list(range(65))),            # the identity map
    "70-thirds": (70, [g for g in range(70) if g % 3 != 2]),
}
_boards = {}


def _quiet(board):
    """a search of the position alone meets no terminal leaf within a case's simulations (in a batch the strict rotation
    may differ: this only picks the positions, the cases assert the live rows they get)"""
    model = tm.Model([orc.clone(board)], R, INV, 3.0, evaluators.make("hash", R), rules=0)
    return model.search(STEPS + 2, 1) == 0 and model.counts["terminals"] == 0


def mid_boards(n, seed=41):
    """n seeded positions one to eight random plies after the start (distinct rows, sides to move of all four colours, and
    no end of the game within the few simulations of a case: the cases assert their live rows), made once, never changed"""
    import random
    import positions as pos
    if (n, seed) not in _boards:
        turn, entries = pos.start_entries(R)
        rng = random.Random(seed)
        out = []
        while len(out) < n:
            b = orc.board_from_dict(R, turn, [list(e) for e in entries])
            for _ply in range(1 + len(out) % 8):
                flats = sorted(set(x[2] for x in orc.legal_moves(b, R, INV)))
                b, rc = orc.take_action(b, R, flats[rng.randrange(len(flats))])
                assert rc == 0
            if orc.game_result(orc.clone(b), R, INV) == 0 and _quiet(b):
                out.append(b)
        _boards[(n, seed)] = out
    return _boards[(n, seed)]


def layout(backend, name):
    G, alive = PATTERNS[name]
    boards = mid_boards(70)[:G]
    if G > 1:
        assert len(set(b.turn for b in boards)) > 1           # strict rules: the rotation is that of the first LIVE row
    budget = [STEPS if g in alive else 0 for g in range(G)]
    ev = evaluators.make("hash", R)
    eng = make_engine(backend, R, INV, max_games=G, max_sims=STEPS)
    try:
        runs = {}
        for on in (0, 1):
            eng.search_begin(roots_of(boards, R), 3.0)
            runs[on] = one_ply(eng, backend, on, [1] * STEPS, budget, ev)
        check_layout(runs[0][2], runs[1][2], [G] * STEPS, want_live=lambda s: alive)
        same_search(runs[0], runs[1])
        assert [int(x) for x in runs[1][0]["sims_done"]] == budget
    finally:
        eng.set_live_rows(0)
        eng.close()


# ---- 2. K = 2 x G = 65 on near-end positions: budgets, terminal backups and collisions make the dead rows ------------------
NEAR_G, NEAR_K, NEAR_STEPS = 65, 2, 5
_near = {}


def near_case(rules):
    """boards (terminal_cases' eight near-end positions of the rule set, in turn), budgets and the model's search, once.
    Budgets: every seventh game 0; odd games 3 or 4 -- the first step completes one simulation (descent k = 1 meets the
    pending root), so some later step's descent k = 1 is cut; the others the whole count."""
    if rules not in _near:
        shape_rules = tc.T if rules == 0 else rules                       # rules 16 and 0 generate the same positions (rules & 15)
        Rr, G8, _, _, seed = tc.SHAPES[("8x8", shape_rules)]
        assert Rr == R
        base = sm.positions(R, G8, seed=seed, near_end=True, rules=rules & 15)
        boards = [base[g % G8] for g in range(NEAR_G)]
        sims = NEAR_K * NEAR_STEPS
        budget = [0 if g % 7 == 3 else (3, 4)[g // 2 % 2] if g % 2 else sims for g in range(NEAR_G)]
        ev = evaluators.make("hash", R)
        model = tm.Model([orc.clone(b) for b in boards], R, INV, 3.0, ev, rules=rules, vl=1.0)
        model.set_budget(budget)
        assert model.search(sims, NEAR_K) == 0
        _near[rules] = (boards, budget, model, model.results())
    return _near[rules]


def near_end(backend, rules):
    boards, budget, model, want = near_case(rules)
    rows = NEAR_K * NEAR_G
    steps = model.steps
    # conditions of the case, from the model alone
    assert len(steps) == NEAR_STEPS and all(st["rows"] == rows for st in steps)
    assert any(0 < len(st["live"]) < rows for st in steps)
    assert any(st["cut"] for st in steps) and any(st["idle"] for st in steps)
    assert model.counts["terminals"] > 0 and model.counts["collisions"] > 0, model.counts
    assert any(r >= 128 for st in steps for r in st["live"])              # a live row in the third scan chunk
    ev = evaluators.make("hash", R)
    eng = make_engine(backend, R, INV, max_games=rows, max_sims=NEAR_K * NEAR_STEPS)
    try:
        eng.set_rules(rules)
        runs = {}
        for on in (0, 1):
            eng.set_leaves(NEAR_K, 1.0)
            eng.search_begin(roots_of(boards, R), 3.0)
            runs[on] = one_ply(eng, backend, on, [NEAR_K] * NEAR_STEPS, budget, ev)
        seen = check_layout(runs[0][2], runs[1][2], [rows] * NEAR_STEPS)
        assert seen == [st["live"] for st in steps]
        same_search(runs[0], runs[1])
        sm.compare(eng, runs[1][0], want, ("live rows, near-end", rules))
    finally:
        eng.set_live_rows(0)
        eng.set_leaves(1)
        eng.set_rules(0)
        eng.close()


# ---- 3. reuse: fpc_search_advance_refill after a switched-on search, then a second ply -------------------------------------
def reuse(backend):
    G, sims = 9, 5
    boards, fresh = mid_boards(70)[:G], mid_boards(70)[20:20 + G]
    budget1 = [sims, 0, sims, sims, 2, sims, 0, sims, sims]
    ev = evaluators.make("hash", R)
    eng = make_engine(backend, R, INV, max_games=G, max_sims=2 * sims)
    try:
        runs = {}
        for on in (0, 1):
            eng.search_begin(roots_of(boards, R), 3.0)
            first = one_ply(eng, backend, on, [1] * sims, budget1, ev)
            src, flats = sm.pick_rule(first[0])                           # games 1 and 6 have no child: they are dropped
            assert src == [0, 2, 3, 4, 5, 7, 8]
            src2 = src[:3] + [-1] + src[3:] + [-1]                        # ... and two rows are refilled
            flats2 = flats[:3] + [0] + flats[3:] + [0]
            kept = eng.search_advance_refill(flats2, src2, fresh=roots_of(fresh, R))
            assert int(kept.max()) > 1
            budget2 = [0 if i in (1, 3) else sims for i in range(G)]      # a kept row and a fresh row stay idle
            second = one_ply(eng, backend, on, [1] * sims, budget2, ev)
            runs[on] = (first, second, [int(k) for k in kept])
        for ply in (0, 1):
            live = [g for g in range(G) if (budget1, [0 if i in (1, 3) else sims for i in range(G)])[ply][g] > 0]
            seen = check_layout(runs[0][ply][2], runs[1][ply][2], [G] * sims)
            assert seen[0] == live and all(set(x) <= set(live) for x in seen) and 0 < len(live) < G
            same_search(runs[0][ply], runs[1][ply])
        assert runs[0][2] == runs[1][2]
    finally:
        eng.set_live_rows(0)
        eng.close()


# ---- 4. the state rules -------------------------------------------------------------------------------------------------
def state_rules(backend):
    ESTATE, EINVAL = -9, -1
    G, sims = 3, 3
    boards = mid_boards(70)[:G]
    ev = evaluators.make("hash", R)
    eng = make_engine(backend, R, INV, max_games=G, max_sims=sims)
    try:
        L, h = eng.L, eng.h
        assert L.fpc_search_set_live_rows(None, 1) == EINVAL
        for bad in (2, -1):
            assert L.fpc_search_set_live_rows(h, bad) == EINVAL
            with pytest.raises(RuntimeError):
                eng.set_live_rows(bad)
        assert L.fpc_search_set_live_rows(h, 1) == 0                      # before fpc_search_begin
        eng.search_begin(roots_of(boards, R), 3.0)
        eng.search_set_budget([sims, 0, sims])
        n_live, ptr = eng.search_select()                                # the setting has survived fpc_search_begin:
        enc = _enc_of(backend, ptr, G)
        assert n_live == 2 and enc[0].any() and enc[1].any() and not enc[2].any()
        for v in (0, 1):                                                  # in the middle of a search
            assert L.fpc_search_set_live_rows(h, v) == ESTATE
        # ... and it is still on: the step goes on with two rows
        lg, v = ev(enc[:2])
        lg, v = np.ascontiguousarray(lg, np.float32), np.ascontiguousarray(v, np.float32)
        if backend == "emul":
            eng.search_expand(lg.ctypes.data, v.ctypes.data)
        else:
            import torch
            lg, v = torch.from_numpy(lg).cuda(), torch.from_numpy(v).cuda()
            torch.cuda.synchronize()
            eng.search_expand(lg.data_ptr(), v.data_ptr())
            torch.cuda.synchronize()
        assert L.fpc_search_set_live_rows(h, 0) == ESTATE                 # the results have not been read
        res = eng.search_results()
        assert [int(x) for x in res["sims_done"]] == [1, 0, 1]
        assert L.fpc_search_set_live_rows(h, 0) == 0                      # a finished search
        assert L.fpc_search_set_live_rows(h, 1) == 0
        eng.search_begin(roots_of(boards, R), 3.0)
        assert L.fpc_search_set_live_rows(h, 0) == 0                      # after begin, before the first selection
        n_live, ptr = eng.search_select()
        assert n_live == 3 and _enc_of(backend, ptr, G)[2].any()
    finally:
        eng.close()


# ---- 5. mcts.MCTS.search with args["live_rows"] over an external evaluator ---------------------------------------------
def mcts_external(backend):
    import dropin_cases
    from mcts import MCTS
    budgets = [6, 1, 6, 3]                       # game 1 is idle from the second step on, game 3 from the fourth
    dropin_cases.setup(backend, R)
    from fen_parser import parse_board_args_from_fen
    from four_player_chess_board import FourPlayerChess
    init = parse_board_args_from_fen(FourPlayerChess.start_fen, R)

    class Seen(dropin_cases.Eval):
        def __call__(self, x):
            self.rows = getattr(self, "rows", []) + [int(x.shape[0])]
            out = super().__call__(x)
            assert int(out[0].shape[0]) == int(x.shape[0])
            return out

    out = {}
    for on in (True, False):                     # the handle is process-wide: the last search leaves it switched off
        ev = Seen("hash", R)
        args = {"C": 3.0, "num_searches": max(budgets), "rules": "fixed", "live_rows": on}
        roots = MCTS(FourPlayerChess, ev, args).search([FourPlayerChess(*init) for _ in budgets], budgets=budgets)
        out[on] = ([r._n for r in roots], [r.child_arrays() for r in roots], ev.rows)
    assert out[False][0] == out[True][0] == [1 + b for b in budgets]
    for (fa, va), (fb, vb) in zip(out[False][1], out[True][1]):
        assert np.array_equal(fa, fb) and np.array_equal(va, vb)
    assert out[False][2] == [4] * 6 and out[True][2] == [4, 3, 3, 2, 2, 2]
