"""FPC_RULES_TERMINAL (include/fpc_engine.h): the cases that run both on the wavefront emulator
(tests/test_terminal_emul.py) and on the GPU (tests/test_terminal_gpu.py).  The model is tests/terminal_model.py.
Everything is compared exactly; there is no tolerance in this file."""
import numpy as np
import pytest

import evaluators
import fpc_ffi
import search_model as sm
import terminal_model as tm
from fpc_testlib import gold, make_engine, roots_of
from oracle import orc

INV_OF = {8: 2, 14: 3}
T, TRAINING = 16, 31                     # FPC_RULES_TERMINAL alone, FPC_RULES_TRAINING


# ---- 1. the Q5 golden position --------------------------------------------------------------------------------------
def q5_root():
    """8x8/2, R rook (4,3), R king (7,4), Y king (0,3), B king (4,0), G king (3,7), Red to move"""
    q5 = gold(8)["searches"][-1]["before"][0]
    assert q5["turn"] == 0 and [sorted(sq for sq, _ in x) for x in q5["pl"]] == [[35, 60], [32], [3], [31]]
    return q5


def golden(backend, copies):
    """zero evaluator, 100 simulations, C = 3.  Rules 16: every simulation is completed (the game is alive to the end:
    a game that left the search would complete no further one), root N = 101, the 18 children (born with N = 1) hold
    18 + 99 visits.  Rules 0 on the same handle afterwards: the root is dropped at N = 11, as ever."""
    R, sims = 8, 100
    q5 = q5_root()
    ev = evaluators.make("zero", R)
    eng = make_engine(backend, R, INV_OF[R], max_games=copies, max_sims=sims)
    try:
        for rules, want_n, want_sum in ((T, 101, 117), (0, 11, 27)):
            roots = [fpc_ffi.board_from_lists(R, q5["turn"], q5["pl"]) for _ in range(copies)]
            eng.set_rules(rules)
            res = sm.run_stepwise(eng, backend, roots, sims, 3.0, ev, 1)
            for g in range(copies):
                n = int(res["n_children"][g])
                assert n == 18, (rules, g)
                assert int(res["root_n"][g]) == want_n, (rules, g, int(res["root_n"][g]))
                assert int(res["visits"][g, :n].sum()) == want_sum, (rules, g)
                assert int(res["sims_done"][g]) == want_n - 1, (rules, g)
    finally:
        eng.set_rules(0)
        eng.close()


# ---- 2. + 3. engine == model on near-end positions -------------------------------------------------------------------
#                  R   G  sims  rules   seed     (the seeds are chosen on the CPU, from the model alone, so that the conditions hold)
SHAPES = {("8x8", T): (8, 8, 100, T, 703),
          ("8x8", TRAINING): (8, 8, 100, TRAINING, 700),
          ("14x14", T): (14, 4, 60, T, 701),
          ("14x14", TRAINING): (14, 4, 60, TRAINING, 700)}
_models = {}


def near_end_model(shape, rules, K):
    """(boards, Model after its search, Model.results()) of a shape, computed once and never changed"""
    key = (shape, rules, K)
    if key not in _models:
        R, G, sims, _, seed = SHAPES[(shape, rules)]
        boards = sm.positions(R, G, seed=seed, near_end=True, rules=rules & 15)
        model = tm.Model([orc.clone(b) for b in boards], R, INV_OF[R], 3.0, evaluators.make("hash", R), rules=rules, vl=1.0)
        assert model.search(sims, K) == 0
        _models[key] = (boards, model, model.results())
    return _models[key]


def check_conditions(model, won=False):
    """conditions on the inputs, from the model alone: the search went on after a terminal backup, and the kinds met"""
    assert max(model.backups) >= 2, model.backups
    assert model.counts["lost"] > 0, model.counts
    if won:
        assert model.counts["won"] > 0, model.counts


def engine_vs_model(backend, shape, rules, K, fused):
    R, G, sims, _, _ = SHAPES[(shape, rules)]
    boards, model, want = near_end_model(shape, rules, K)
    check_conditions(model)
    assert any(model.alive)
    if K == 1:                                   # one leaf per step: a game that is alive completes every simulation
        assert all(sd == sims for sd, alive in zip(model.sims_done, model.alive) if alive)
    eng = make_engine(backend, R, INV_OF[R], max_games=G * K, max_sims=sims)
    try:
        eng.set_rules(rules)
        res = sm.run_stepwise(eng, backend, roots_of(boards, R), sims, 3.0, evaluators.make("hash", R), K, vl=1.0, fused=fused)
        sm.compare(eng, res, want, (shape, rules, K, fused))
    finally:
        eng.set_leaves(1)
        eng.set_rules(0)
        eng.close()


# ---- 2b. the legal-only head through fpc_search_run (GPU only: the emulator has no network) ------------------------------------
LEGAL = dict(R=8, hidden=128, dtype=1, layout=2, rules=TRAINING, sims=32, seed=700)
_legal = {}


def legal_case():
    """everything of the case that needs no GPU, computed once: legal_head_cases.search_setup's integer network (its float64
    reference IS the evaluator; the value head is all zero, so the only values in the trees are the terminal ones) on
    twelve near-end roots, and the model's search with policy_head="legal" under rules 31"""
    if not _legal:
        import legal_head_cases as lc
        c = LEGAL
        boards = sm.positions(c["R"], lc.G, seed=c["seed"], near_end=True, rules=c["rules"] & 15)
        m, boards, s, ev = lc.search_setup(c["R"], c["hidden"], c["dtype"], boards=boards, rules=c["rules"] & 15)
        model = tm.Model([orc.clone(b) for b in boards], c["R"], INV_OF[c["R"]], 3.0, ev, rules=c["rules"], policy_head="legal")
        assert model.search(c["sims"], 1) == 0
        check_conditions(model)
        _legal.update(m=m, boards=boards, s=s, model=model, want=model.results())
    return _legal


# ---- 3b. a leaf whose side to move WON ---------------------------------------------------------------------------------
# No seeded near-end position met one (the first legal move of the side to move has to take a king), so by hand: 8x8/2,
# kings at home, R rook (4,4), B rook (0,2) beside the Yellow king, Red to move.  After six of Red's 18 moves -- the
# lowest flat index among them -- Blue's first legal move is rook takes king: GetGameResult says WIN_BG with Blue to move.
WON_ENTRIES = [[60, 0, 5], [32, 1, 5], [3, 2, 5], [31, 3, 5], [36, 0, 3], [2, 1, 3]]


def won_root():
    return orc.board_from_dict(8, 0, [list(e) for e in WON_ENTRIES])


def won_leaf(backend):
    """Two simulations with the zero evaluator: the second one descends to the root's first child (equal priors, the
    lowest index wins), which is such a leaf.  Rules 16 back up +1 at the leaf and -1 at its parent, rules 0 back up -1 and
    +1.  The leaf's W is read from the engine, the root's (not part of the results) from the model the engine equals.
    Then 30 simulations under rules 16 and 31: engine == model with `won`, `lost` and repeated backups."""
    R, INV = 8, 2
    ev = evaluators.make("zero", R)
    eng = make_engine(backend, R, INV, max_games=1, max_sims=30)
    try:
        leaf_w, root_w = {}, {}
        for rules in (T, 0):
            model = tm.Model([won_root()], R, INV, 3.0, ev, rules=rules)
            assert model.search(2, 1) == 0
            assert model.counts["won"] == 1 and model.counts["terminals"] == 1
            eng.set_rules(rules)
            res = sm.run_stepwise(eng, backend, roots_of([won_root()], R), 2, 3.0, ev, 1)
            sm.compare(eng, res, model.results(), ("won leaf", rules))
            assert int(res["visits"][0, 0]) == 2
            leaf_w[rules], root_w[rules] = float(res["w"][0, 0]), model.roots[0].W
            assert model.roots[0].children[0].W == leaf_w[rules]
        assert leaf_w == {T: 1.0, 0: -1.0} and root_w == {T: -1.0, 0: 1.0}
        for rules in (T, TRAINING):
            model = tm.Model([won_root()], R, INV, 3.0, ev, rules=rules)
            assert model.search(30, 1) == 0
            check_conditions(model, won=True)
            eng.set_rules(rules)
            res = sm.run_stepwise(eng, backend, roots_of([won_root()], R), 30, 3.0, ev, 1)
            sm.compare(eng, res, model.results(), ("won leaf, 30 simulations", rules))
            assert int(res["sims_done"][0]) == 30
    finally:
        eng.set_rules(0)
        eng.close()


# ---- 4. budgets -------------------------------------------------------------------------------------------------------
def budgets(backend):
    """G = 4 near-end positions, budgets {0, 7, 30, 100}, K = 3, rules 31.  100 steps of 3 leaves: descent 0 of a step
    never collides (no visit is pending when a step starts) and is made while the game is alive and below its budget, so
    every step completes at least one simulation of such a game -- after 100 steps a game that is alive is AT its budget."""
    R, G, K, rules, steps = 8, 4, 3, TRAINING, 100
    budget = [0, 7, 30, 100]
    boards = sm.positions(R, G, seed=700, near_end=True, rules=rules & 15)
    ev = evaluators.make("hash", R)
    model = tm.Model([orc.clone(b) for b in boards], R, INV_OF[R], 3.0, ev, rules=rules, vl=1.0)
    model.set_budget(budget)
    assert model.search(K * steps, K) == 0
    assert model.counts["terminals"] > 0 and max(model.backups) >= 2 and any(model.alive[1:])
    eng = make_engine(backend, R, INV_OF[R], max_games=G * K, max_sims=max(budget))
    try:
        eng.set_rules(rules)
        eng.set_leaves(K, 1.0)
        eng.search_begin(roots_of(boards, R), 3.0)
        eng.search_set_budget(budget)
        sm.run_steps(eng, backend, K * steps, ev, K, 1.0)
        res = eng.search_results()
        sm.compare(eng, res, model.results(), "budgets")
        for g in range(G):
            assert int(res["sims_done"][g]) <= budget[g], g
            if model.alive[g]:
                assert int(res["sims_done"][g]) == budget[g], g
    finally:
        eng.set_leaves(1)
        eng.set_rules(0)
        eng.close()


# ---- 5. a terminal root -------------------------------------------------------------------------------------------------
def terminal_root(backend):
    """a game begun on a finished position between two live ones: one backup, then it has left the search (19 further steps
    complete nothing of it), no children; fpc_search_play gives -1 / -1 and the root state for it"""
    R, rules, sims = 8, TRAINING, 20
    INV = INV_OF[R]
    live = sm.positions(R, 6, seed=700, near_end=True, rules=rules & 15)
    finished = None
    orc.set_rules(rules & 15)
    try:
        for b in live:
            for fl in sorted(set(m[2] for m in orc.legal_moves(orc.clone(b), R, INV))):
                nb, rc = orc.take_action(orc.clone(b), R, fl)
                if rc == 0 and orc.game_result(orc.clone(nb), R, INV) != 0:
                    finished = nb
                    break
            if finished is not None:
                break
    finally:
        orc.set_rules(0)
    assert finished is not None
    boards = [live[0], finished, live[1]]
    ev = evaluators.make("hash", R)
    model = tm.Model([orc.clone(b) for b in boards], R, INV, 3.0, ev, rules=rules)
    assert model.search(sims, 1) == 0
    assert model.alive == [True, False, True] and model.sims_done == [sims, 1, sims]
    eng = make_engine(backend, R, INV, max_games=3, max_sims=sims)
    try:
        eng.set_rules(rules)
        res = sm.run_stepwise(eng, backend, roots_of(boards, R), sims, 3.0, ev, 1)
        sm.compare(eng, res, model.results(), "terminal root")
        assert [int(x) for x in res["n_children"] > 0] == [1, 0, 1]
        assert int(res["sims_done"][1]) == 1 and int(res["root_n"][1]) == 2
        flats, results, pods = eng.search_play(1.0, [0.3, 0.9, 0.6])
        assert int(flats[1]) == -1 and int(results[1]) == -1 and pods[1].tobytes() == bytes(res["boards"][1])
        assert int(flats[0]) >= 0 and int(flats[2]) >= 0
    finally:
        eng.set_rules(0)
        eng.close()


# ---- 6. reuse -----------------------------------------------------------------------------------------------------------
def reuse(backend):
    """fpc_search_advance after a rules-31 search, then 50 more simulations == the model's advance + search"""
    R, G, rules, sims, more = 8, 6, TRAINING, 40, 50
    INV = INV_OF[R]
    boards = sm.positions(R, G, seed=702, near_end=True, rules=rules & 15)
    ev = evaluators.make("hash", R)
    model = tm.Model([orc.clone(b) for b in boards], R, INV, 3.0, ev, rules=rules)
    eng = make_engine(backend, R, INV, max_games=G, max_sims=sims + more)
    try:
        eng.set_rules(rules)
        res = sm.run_stepwise(eng, backend, roots_of(boards, R), sims, 3.0, ev, 1)
        assert model.search(sims, 1) == 0
        sm.compare(eng, res, model.results(), "before the advance")
        before = model.counts["terminals"]
        assert before > 0
        src, flats = sm.pick_rule(res)
        assert len(src) >= 3
        kept = eng.search_advance(flats, src)
        assert [int(k) for k in kept] == model.advance(src, flats)
        assert int(kept.max()) > 2                                   # condition: a kept root brings a subtree along
        sm.run_steps(eng, backend, more, ev)
        res = eng.search_results()
        assert model.search(more, 1) == 0
        sm.compare(eng, res, model.results(), "after the advance")
        assert model.counts["terminals"] > before and any(model.alive)
    finally:
        eng.set_rules(0)
        eng.close()


# ---- 7. selfplay.play(z_from_result=True) ---------------------------------------------------------------------------------
def selfplay_z(backend):
    """every finished game's z follows its result; the default run gives the Q12 values; entries, moves and results are
    the same in both"""
    import selfplay
    from treereuse_cases import _episode_fns
    R, G, sims, L, rules = 8, 6, 12, 6, TRAINING
    boards = sm.positions(R, G, seed=96, near_end=True, rules=rules & 15)
    ev = evaluators.make("hash", R)
    args = {"temperature": 1.1, "max_game_length": L, "heuristic_weight": 0.5}
    uniforms = np.random.default_rng(17).random((L, G)).tolist()
    eng = make_engine(backend, R, INV_OF[R], max_games=G, max_sims=2 * sims)
    try:
        eng.set_rules(rules)
        search_fn, _ = _episode_fns(eng, backend, ev, sims)
        by_result = selfplay.play(search_fn, eng, roots_of(boards, R), args, uniforms, z_from_result=True)
        q12 = selfplay.play(search_fn, eng, roots_of(boards, R), args, uniforms)
    finally:
        eng.set_rules(0)
        eng.close()
    assert len(by_result) == len(q12) == G
    seen = {"finished": 0, "differs": 0, "both_signs": 0, "stalemate": 0, "unfinished": 0}
    for a, b in zip(by_result, q12):
        assert a.moves == b.moves and a.result == b.result and a.length == b.length and len(a.entries) == len(b.entries)
        for (ba, fa, va), (bb, fb, vb) in zip(a.entries, b.entries):
            assert bytes(ba) == bytes(bb) and np.array_equal(fa, fb) and np.array_equal(va, vb)
        teams = [pod.turn & 1 for pod, _, _ in a.entries]
        if a.result == 0:                                            # max_game_length: the heuristic branch, untouched
            assert a.z == b.z
            seen["unfinished"] += 1
            continue
        seen["finished"] += 1
        mover = a.entries[-1][0].turn & 1                            # Q12: the team that moved last is called the loser
        assert b.z == [1.0 if t != mover else -1.0 for t in teams]
        if a.result == 3:
            assert a.z == [0.0] * len(teams)
            seen["stalemate"] += 1
        else:
            winner = {1: 0, 2: 1}[a.result]
            assert a.z == [1.0 if t == winner else -1.0 for t in teams]
            seen["both_signs"] += len(set(a.z)) == 2
        seen["differs"] += a.z != b.z
    # conditions of the case (the seed is chosen for them): games end on the board, one with entries of both teams, one in a
    # stalemate, one goes on to max_game_length, and the two labellings differ
    assert seen["both_signs"] > 0 and seen["stalemate"] > 0 and seen["unfinished"] > 0 and seen["differs"] > 0, seen
    return seen


# ---- 8. fpc_set_rules' range ------------------------------------------------------------------------------------------------
def rules_range(backend):
    eng = make_engine(backend, 8, 2, max_games=1, max_sims=4)
    try:
        for ok in (16, 31, 15, 0):
            assert eng.L.fpc_set_rules(eng.h, ok) == 0, ok
        for bad in (32, -1):
            assert eng.L.fpc_set_rules(eng.h, bad) == -1, bad        # FPC_EINVAL
            with pytest.raises(RuntimeError, match="bad rule set"):
                eng.set_rules(bad)
        assert (fpc_ffi.RULES_TERMINAL, fpc_ffi.RULES_TRAINING) == (16, 31)
        assert fpc_ffi.RULES_TRAINING == fpc_ffi.RULES_FIXED | fpc_ffi.RULES_TERMINAL and fpc_ffi.RULES_FIXED == 15
    finally:
        eng.close()


def mcts_rules_names():
    """mcts.MCTS: args["rules"] = "training" is 31; the other spellings are what they were"""
    from mcts import MCTS
    for given, want in (("training", 31), ("fixed", 15), ("strict", 0), (16, 16), (31, 31)):
        assert MCTS(None, lambda x: x, {"C": 3.0, "num_searches": 1, "rules": given}).rules == want
