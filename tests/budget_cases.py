"""Per-game simulation budgets (fpc_search_set_budget): the cases that run both on the wavefront emulator
(tests/test_budget_emul.py) and on the GPU (tests/test_budget_gpu.py).  Everything is compared exactly; there is no
tolerance in this file."""
import numpy as np
import pytest

import budget_model as bm
import evaluators
import fpc_ffi
import search_model as sm
from fpc_testlib import make_engine, roots_of
from oracle import orc
from refill_cases import _argmax_flats, _pod
from treereuse_cases import INV_OF, _same_episodes

EINVAL, ECAPACITY, ESTATE = -1, -6, -9

#               R   G  K  rules                evaluator sims plies noise near-end half  seed
CASES = {"A": (8, 8, 1, 0, "hash", 24, 4, False, True, 500),
         "B": (8, 6, 3, 0, "ramp", 20, 3, False, False, 510),
         "C": (14, 6, 2, fpc_ffi.RULES_FIXED, "hash", 20, 3, True, False, 520)}


def _budget_mix(rng, G, K, sims, base, max_sims):
    """one ply's budgets: 0, 1, a value below K, a value that is no multiple of K and the maximum, the rest drawn, in a
    seeded order; each within what the game's kept visits leave of max_sims"""
    odd = next(v for v in (7, 5, 11, 13) if v % K or K == 1)
    mix = [0, 1, max(K - 1, 0), odd, sims]
    mix += [int(x) for x in rng.integers(0, sims + 1, size=G - len(mix))]
    mix = [mix[i] for i in rng.permutation(G)]
    return [min(b, max_sims - base[g]) for g, b in enumerate(mix)]


# ---- 1. engine == model --------------------------------------------------------------------------------------------
def engine_vs_model(backend, case):
    """plies of begin, search, advance_refill with budgets set every ply: engine == model (results, grandchildren,
    sims_done) after every ply.  The rows that are refilled are refill_cases.engine_vs_model's: every row whose game is
    over, whose root was never expanded (budget 0 on a fresh root) or whose picked move ends it, plus row
    (3 * ply + 1) % n regardless."""
    R, G, K, rules, kind, sims, plies, noise, near_half, seed = CASES[case]
    INV = INV_OF[R]
    if near_half:
        a, b = sm.positions(R, G // 2, seed=seed, rules=rules), sm.positions(R, G - G // 2, seed=seed + 1, near_end=True, rules=rules)
        boards = [x for pair in zip(a, b) for x in pair]
    else:
        boards = sm.positions(R, G, seed=seed, rules=rules)
    pool = sm.positions(R, (plies - 1) * G, seed=seed + 50, rules=rules)
    ev = evaluators.make(kind, R)
    model = bm.Model([orc.clone(b) for b in boards], R, INV, 3.0, ev, rules=rules, noise_eps=0.25)
    eng = make_engine(backend, R, INV, max_games=G * K, max_sims=2 * sims)
    rng = np.random.default_rng(seed)
    cond = {"budget0": 0, "idle5": 0, "mid_step": 0, "terminal": 0, "rotation_from_later_row": 0, "mixed": 0}

    def set_noise(n):
        if noise:
            gamma = rng.standard_gamma(0.3, size=(n, fpc_ffi.MAX_MOVES)).astype(np.float32)
            eng.set_root_noise(gamma, 0.25)
            model.set_noise(gamma)

    try:
        eng.set_rules(rules)
        eng.set_leaves(K)
        set_noise(G)
        eng.search_begin(roots_of(boards, R), 3.0)
        base = [0] * G
        for ply in range(plies):
            n = len(base)
            budget = _budget_mix(rng, n, K, sims, base, eng.max_sims)
            eng.search_set_budget(budget)
            model.set_budget(budget)
            run = max(budget)
            first_step, terminals = len(model.steps), model.counts["terminals"]
            sm.run_steps(eng, backend, run, ev, K)
            res = eng.search_results()
            assert model.search(run, K) == 0
            sm.compare(eng, res, model.results(), (case, ply), grand_every=2)
            assert all(int(res["sims_done"][g]) <= budget[g] for g in range(n)), (case, ply, "the gate is exact")
            # ---- conditions
            steps = model.steps[first_step:]
            cond["budget0"] += 0 in budget
            cond["terminal"] += model.counts["terminals"] - terminals
            cond["mid_step"] += sum(bool(s["cut"]) for s in steps)
            idle = [sum(1 for s in steps if s["live"] and g in s["idle"]) for g in range(n)]
            cond["idle5"] += sum(x >= 5 for x in idle)
            if not rules & fpc_ffi.RULES_ROTATION:
                t0 = model.roots[0].state.turn
                cond["rotation_from_later_row"] += sum(1 for s in steps if 0 in s["idle"] and s["live"] and s["turns"][0] != t0)
            if ply + 1 == plies:
                break
            # ---- what the next advance does with every row
            picked = dict(zip(*sm.pick_rule(res)))
            src, flats = [], []
            for g in range(n):
                over = g not in picked
                if not over:
                    orc.set_rules(rules)
                    try:
                        nxt, mrc = orc.take_action(orc.clone(model.roots[g].state), R, picked[g])
                        assert mrc == 0
                        over = orc.game_result(nxt, R, INV) != 0
                    finally:
                        orc.set_rules(0)
                if over or g == (3 * ply + 1) % n:
                    src.append(-1); flats.append(0)
                else:
                    src.append(g); flats.append(picked[g])
            fresh_o = [pool.pop() if s < 0 else None for s in src]
            set_noise(n)
            kept = eng.search_advance_refill(flats, src, fresh=[None if b is None else _pod(b, R) for b in fresh_o])
            assert [int(x) for x in kept] == model.advance_refill(src, flats, fresh_o), (case, ply, "kept visits")
            cond["mixed"] += any(s < 0 for s in src) and any(s >= 0 for s in src)
            base = [int(k) - 1 for k in kept]
    finally:
        eng.close()
    # conditions of the case, not results: if a seed misses one, change the seed (on the emulator)
    need = ["budget0", "idle5", "terminal", "mixed"] + (["mid_step"] if K > 1 else [])
    need += ["rotation_from_later_row"] if not rules & fpc_ffi.RULES_ROTATION else []
    if case != "A":
        need.remove("terminal")                  # the near-end positions are case A's
    assert all(cond[k] > 0 for k in need), cond
    return cond


# ---- 2. independence -----------------------------------------------------------------------------------------------
def independence(backend):
    """FPC_RULES_FIXED: a search does not depend on the batch.  Run with budgets b for max(b) steps, game g has, bit for
    bit, the search of the same root run alone for b[g] simulations -- through two plies with reuse"""
    R, G, sims, rules = 8, 6, 14, fpc_ffi.RULES_FIXED
    INV = INV_OF[R]
    budgets = [[14, 3, 9, 1, 14, 6], [5, 14, 0, 14, 1, 9]]
    boards = sm.positions(R, G, seed=61, rules=rules)
    ev = evaluators.make("hash", R)

    def plies_of(eng, pods, b_of_ply, use_budget):
        out, kept = [], np.ones(len(pods), np.int32)
        eng.set_rules(rules)
        eng.search_begin(pods, 3.0)
        for ply, b in enumerate(b_of_ply):
            if use_budget:
                eng.search_set_budget(b)
            sm.run_steps(eng, backend, max(b), ev)
            res = eng.search_results()
            out.append((kept, res))
            if ply + 1 < len(b_of_ply):
                kept = eng.search_advance(_argmax_flats(res))
        return out

    batch_eng = make_engine(backend, R, INV, max_games=G, max_sims=4 * sims)
    try:
        batch = plies_of(batch_eng, roots_of(boards, R), budgets, True)
    finally:
        batch_eng.close()
    for ply, (kept, res) in enumerate(batch):
        b = np.array(budgets[ply])
        assert np.array_equal(res["sims_done"], b), (ply, "no terminal leaf at these seeds: every game completes its budget")
        assert np.array_equal(res["root_n"], kept + res["sims_done"]), ply
    for g in range(G):
        alone_eng = make_engine(backend, R, INV, max_games=1, max_sims=4 * sims)
        try:
            alone = plies_of(alone_eng, roots_of(boards[g:g + 1], R), [[b[g]] for b in budgets], False)
        finally:
            alone_eng.close()
        for (ka, a), (kb, b) in zip(alone, batch):
            assert int(ka[0]) == int(kb[g])
            sm.same_results(a, b, [0], [g])


# ---- 3. null budgets == today --------------------------------------------------------------------------------------
def null_budgets(backend, K):
    """a search with set_budget(None), and one with every budget >= the simulations run, equals the same search on a twin
    engine that never heard of budgets -- on fresh trees and after an advance"""
    R, G, sims = 8, 5, 12
    INV = INV_OF[R]
    a, b = sm.positions(R, 3, seed=71), sm.positions(R, 2, seed=72, near_end=True)
    boards = a + b
    ev = evaluators.make("hash", R)
    engs = {kind: make_engine(backend, R, INV, max_games=G * K, max_sims=3 * sims) for kind in ("none", "wide", "twin")}
    try:
        for eng in engs.values():
            eng.set_leaves(K)
            eng.search_begin(roots_of(boards, R), 3.0)
        kept = np.ones(G, np.int32)
        for ply in range(2):
            n = len(kept)
            engs["none"].search_set_budget([1] * n)          # set, then cleared again
            engs["none"].search_set_budget(None)
            engs["wide"].search_set_budget([sims + (g % 3) for g in range(n)])
            res = {}
            for kind, eng in engs.items():
                sm.run_steps(eng, backend, sims, ev, K)
                res[kind] = eng.search_results()
            sm.same_results(res["none"], res["twin"])
            sm.same_results(res["wide"], res["twin"])
            assert int(res["twin"]["sims_done"].max()) > sims // 2      # (K > 1: collisions complete nothing)
            if ply == 0:
                src, flats = sm.pick_rule(res["twin"])
                assert len(src) >= 3
                for eng in engs.values():
                    kept = eng.search_advance(flats, src)
    finally:
        for eng in engs.values():
            eng.close()


# ---- 4. capacity ---------------------------------------------------------------------------------------------------
def capacity_per_game(backend):
    """max_sims = S + S // 2, one kept root with many visits beside a fresh row: today's batch-wide rule leaves the fresh
    row less than S; with "per_game" budgets it completes S and the kept row max_sims - base, with no pool overflow"""
    from mcts import budgets_for
    R, S, rules = 8, 16, fpc_ffi.RULES_FIXED
    INV, max_sims = INV_OF[R], S + S // 2
    boards = sm.positions(R, 3, seed=81, rules=rules)
    hash_ev = evaluators.make("hash", R)

    def ev(enc):                                 # peaked priors (the hash logits times 8, still exact in f32): visits concentrate
        logits, v = hash_ev(enc)
        return logits * np.float32(8), v

    eng = make_engine(backend, R, INV, max_games=2, max_sims=max_sims)
    try:
        eng.set_rules(rules)
        eng.search_begin(roots_of(boards[:2], R), 1.0)
        sm.run_steps(eng, backend, max_sims, ev)
        res = eng.search_results()
        kept = eng.search_advance_refill([_argmax_flats(res)[0], 0], [0, -1], fresh=[None, _pod(boards[2], R)])
        base = int(kept[0]) - 1
        assert int(kept[1]) == 1 and base > S // 2, kept           # condition of the case: the kept root has many visits
        assert max_sims - (int(kept.max()) - 1) < S                 # today's rule: everybody gets less than S
        budget = budgets_for(kept, S, max_sims, "per_game")
        assert budget == [max_sims - base, S]
        with pytest.raises(RuntimeError, match="game 0"):           # one more on the kept row does not fit
            eng.search_set_budget([budget[0] + 1, S])
        eng.search_set_budget(budget)
        sm.run_steps(eng, backend, max(budget), ev)                 # S steps: more than the batch-wide rule admits
        res = eng.search_results()                                  # raises on any error bit (pool overflow)
        assert [int(x) for x in res["sims_done"]] == budget
        assert [int(x) for x in res["root_n"]] == [max_sims + 1, S + 1]
    finally:
        eng.close()


def capacity_visit_target(backend):
    """"visit_target" on an engine created with max_sims = S: plies of reuse plus refill with no FPC_ECAPACITY and no
    error bit; every searched root ends with S simulations through it unless Q5 removed it"""
    from mcts import budgets_for
    R, S, G, plies = 8, 16, 5, 4
    INV = INV_OF[R]
    a, b = sm.positions(R, 3, seed=91), sm.positions(R, 2, seed=92, near_end=True)
    boards = [a[0], b[0], a[1], b[1], a[2]]
    pool = sm.positions(R, plies * G, seed=93)
    ev = evaluators.make("hash", R)
    eng = make_engine(backend, R, INV, max_games=G, max_sims=S)
    seen = {"kept_with_visits": 0, "q5": 0, "fresh": 0, "shorter": 0}
    try:
        eng.search_begin(roots_of(boards, R), 3.0)
        kept = np.ones(G, np.int32)
        for ply in range(plies):
            budget = budgets_for(kept, S, eng.max_sims, "visit_target")
            assert all(int(k) - 1 + x <= S for k, x in zip(kept, budget))
            eng.search_set_budget(budget)
            sm.run_steps(eng, backend, max(budget), ev)
            res = eng.search_results()
            for g in range(G):
                if int(res["sims_done"][g]) == budget[g]:
                    assert int(res["root_n"][g]) - 1 == max(S, int(kept[g]) - 1), (ply, g)
                else:                                               # a terminal leaf took the root out of the search (Q5)
                    assert int(res["sims_done"][g]) < budget[g]
                    seen["q5"] += 1
            seen["shorter"] += max(budget) < S
            picked = dict(zip(*sm.pick_rule(res)))
            src = [g if g in picked and g != (2 * ply + 1) % G else -1 for g in range(G)]
            flats = [picked[g] if s >= 0 else 0 for g, s in enumerate(src)]
            kept = eng.search_advance_refill(flats, src, fresh=[None if s >= 0 else _pod(pool.pop(), R) for s in src])
            seen["kept_with_visits"] += int((kept > 1).sum())
            seen["fresh"] += sum(s < 0 for s in src)
    finally:
        eng.close()
    assert seen["kept_with_visits"] > 0 and seen["fresh"] > 0, seen
    return seen


# ---- 5. errors -----------------------------------------------------------------------------------------------------
def errors(backend):
    """every FPC_ESTATE / FPC_EINVAL / FPC_ECAPACITY case; after the refused calls the search continues to what an
    untouched twin gives; budgets are gone after search_begin, search_advance and search_advance_refill"""
    R, G, sims = 8, 5, 12
    INV = INV_OF[R]
    boards = sm.positions(R, G, seed=31)
    fresh = roots_of(sm.positions(R, G, seed=33), R)
    ev = evaluators.make("hash", R)
    eng, twin, idle = (make_engine(backend, R, INV, max_games=G, max_sims=2 * sims) for _ in range(3))
    P = fpc_ffi.C.POINTER(fpc_ffi.C.c_int)

    def raw(e, values, n=None):
        arr = np.ascontiguousarray(values, np.int32)
        return e.L.fpc_search_set_budget(e.h, fpc_ffi.C.cast(arr.ctypes.data, P), len(arr) if n is None else n)

    def both_run(n):
        sm.run_steps(eng, backend, n, ev)
        sm.run_steps(twin, backend, n, ev)
        a, b = eng.search_results(), twin.search_results()
        sm.same_results(a, b)
        return a

    try:
        # no search in progress
        assert raw(idle, [1] * G) == ESTATE
        with pytest.raises(RuntimeError, match="needs a search in progress"):
            idle.search_set_budget([1] * G)
        assert eng.L.fpc_search_set_budget(None, None, G) == EINVAL                  # null engine
        eng.search_begin(roots_of(boards, R), 3.0)
        twin.search_begin(roots_of(boards, R), 3.0)
        # ---- refused before the first selection: nothing is set
        assert raw(eng, [1] * (G - 1)) == EINVAL and raw(eng, [1] * G, G + 1) == EINVAL
        with pytest.raises(RuntimeError, match="n_games"):
            eng.search_set_budget([1] * (G + 1))
        assert raw(eng, [1, 1, -1, 1, 1]) == EINVAL
        with pytest.raises(RuntimeError, match=r"budget\[2\] = -1"):
            eng.search_set_budget([1, 1, -1, 1, 1])
        assert raw(eng, [1, 1, 1, 2 * sims + 1, 2 * sims + 7]) == ECAPACITY
        with pytest.raises(RuntimeError, match="game 3"):
            eng.search_set_budget([1, 1, 1, 2 * sims + 1, 2 * sims + 7])
        eng.search_set_budget([2 * sims] * G)                                        # base 0: all of max_sims fits
        eng.search_set_budget(None)
        # ---- after a selection has been issued; after the results have been read
        sm.run_steps(eng, backend, 3, ev)
        sm.run_steps(twin, backend, 3, ev)
        assert raw(eng, [1] * G) == ESTATE
        with pytest.raises(RuntimeError, match="a selection has been issued"):
            eng.search_set_budget(None)
        res0 = both_run(sims - 3)                                                    # ... and the search went on untouched
        assert int(res0["sims_done"].max()) == sims
        assert raw(eng, [1] * G) == ESTATE
        with pytest.raises(RuntimeError, match="the search is finished"):
            eng.search_set_budget([1] * G)
        # ---- capacity is per game after an advance; budgets are gone after search_advance
        flats = _argmax_flats(res0)
        kept = eng.search_advance(flats)
        assert np.array_equal(kept, twin.search_advance(flats)) and int(kept.max()) > 2
        room = [2 * sims - (int(k) - 1) for k in kept]
        j = int(np.argmax(kept))
        over = list(room)
        over[j] += 1
        assert raw(eng, over) == ECAPACITY
        with pytest.raises(RuntimeError, match="game %d" % j):
            eng.search_set_budget(over)
        eng.search_set_budget(room)                                                  # exactly what every game has room for
        eng.search_set_budget([1] * G)
        after = eng.search_results()                                                 # no simulation was run
        eng.search_set_budget([2] * G)                                               # ... so the results close nothing
        sm.same_results(after, twin.search_results())
        src = [g for g in range(G) if int(after["n_children"][g]) > 0]
        assert len(src) >= 2
        flats = [_argmax_flats(after)[g] for g in src]
        assert np.array_equal(eng.search_advance(flats, src), twin.search_advance(flats, src))
        res1 = both_run(sims // 2)
        assert int(res1["sims_done"].max()) == sims // 2                             # no budget of 1 is in force
        # ---- ... and after search_advance_refill
        n = len(src)
        src2, flats2 = [-1] + list(range(1, n)), [0] + _argmax_flats(res1)[1:]
        ka = eng.search_advance_refill(flats2, src2, fresh=[fresh[0]] + [None] * (n - 1))
        assert np.array_equal(ka, twin.search_advance_refill(flats2, src2, fresh=[fresh[0]] + [None] * (n - 1)))
        eng.search_set_budget([0] * n)
        eng.search_results()
        twin.search_results()
        for e in (eng, twin):
            e.search_advance_refill([0] * G, [-1] * G, fresh=fresh)
        res2 = both_run(sims // 2)
        assert int(res2["sims_done"].min()) > 0
        # ---- ... and after search_begin
        eng.search_begin(roots_of(boards, R), 3.0)
        eng.search_set_budget([2] * G)
        eng.search_begin(roots_of(boards, R), 3.0)
        twin.search_begin(roots_of(boards, R), 3.0)
        res3 = both_run(sims // 2)
        assert int(res3["sims_done"].max()) == sims // 2
    finally:
        eng.close()
        twin.close()
        idle.close()


# ---- 6. the Python surface -----------------------------------------------------------------------------------------
def budgets_for_by_hand():
    from mcts import budgets_for
    kept = [1, 5, 21, 41, 60]
    assert budgets_for(kept, 40, 80, None) is None
    assert budgets_for(kept, 40, 60, "per_game") == [40, 40, 40, 20, 1]
    assert budgets_for(kept, 40, 80, "per_game") == [40, 40, 40, 40, 21]
    assert budgets_for(kept, 40, 40, "visit_target") == [40, 36, 20, 0, 0]
    assert budgets_for(np.array(kept, np.int32), 40, 40, "visit_target") == [40, 36, 20, 0, 0]
    assert budgets_for([], 40, 40, "per_game") == []
    with pytest.raises(ValueError):
        budgets_for(kept, 40, 40, "something")


def mcts_explicit_budgets(backend):
    """MCTS.search(games, budgets=...): game g completes budgets[g] simulations (the start position meets no terminal leaf)
    and has the root the same search gives it with num_searches = budgets[g] (fixed rules: no dependence on the batch)"""
    import dropin_cases
    from mcts import MCTS
    R, budgets = 8, [12, 5, 1]
    dropin_cases.setup(backend, R)
    from fen_parser import parse_board_args_from_fen
    from four_player_chess_board import FourPlayerChess
    init = parse_board_args_from_fen(FourPlayerChess.start_fen, R)
    args = {"C": 3.0, "num_searches": max(budgets), "rules": "fixed"}
    roots = MCTS(FourPlayerChess, dropin_cases.Eval("hash", R), args).search([FourPlayerChess(*init) for _ in budgets], budgets=budgets)
    assert [r._n for r in roots] == [1 + b for b in budgets]
    for root, b in zip(roots, budgets):
        alone = MCTS(FourPlayerChess, dropin_cases.Eval("hash", R), dict(args, num_searches=b)).search([FourPlayerChess(*init)])[0]
        assert alone._n == root._n
        fa, va = alone.child_arrays()
        fr, vr = root.child_arrays()
        assert np.array_equal(fa, fr) and np.array_equal(va, vr)


AZ_ARGS = {"C": 3.0, "num_searches": 64, "num_parallel_games": 2, "temperature": 1.0, "heuristic_weight": 0.02,
           "max_game_length": 3, "replay_buffer_capacity": 100, "validation_buffer_capacity": 20, "refill": True,
           "reuse_tree": True, "sim_budget": "visit_target"}


def alphazero_visit_target(backend):
    """AlphaZero with reuse_tree + refill + sim_budget="visit_target" and an external evaluator plays the episodes of
    selfplay.play driven directly through the C-ABI with the same budgets, on a handle of num_searches simulations"""
    import torch

    import dropin_cases
    import selfplay
    from mcts import budgets_for
    from refill_cases import _alphazero_setup
    az, R, FourPlayerChess, init, model, opt = _alphazero_setup(backend)
    from alphazero import AlphaZero
    G, total, sims, L, seed = AZ_ARGS["num_parallel_games"], 4, AZ_ARGS["num_searches"], AZ_ARGS["max_game_length"], 3
    # the process-wide handle only grows, and dropin_cases.setup injects the emulator's with room to spare: start from a
    # handle of exactly num_searches, so that a request for more would show (on the emulator as a failing fpc_create)
    if az._engine is not None:
        az._engine.close()
    az._engine, az._engine_cap = None, (0, 0)
    if backend == "emul":
        az._engine, az._engine_cap = make_engine(backend, R, INV_OF[R], max_games=64, max_sims=sims), (64, sims)
        az._engine.nn_dtype, az._engine.weights_version = 0, None
    a = AlphaZero(model, opt, FourPlayerChess, dict(AZ_ARGS), init, evaluator=dropin_cases.Eval("hash", R), seed=seed)
    got = a.play(total_games=total)
    assert len(got) == total and max(e.start for e in got) > 0
    assert az.engine().max_sims == sims                            # not 2 * num_searches
    uniforms = torch.rand(L, total, generator=torch.Generator().manual_seed(seed), dtype=torch.float64).tolist()
    start = [FourPlayerChess(*init)._b for _ in range(total)]
    eng = make_engine(backend, R, INV_OF[R], max_games=G, max_sims=sims)
    ev = evaluators.make("hash", R)
    shorter = []
    try:
        def search_fn(pods):
            eng.search_begin(pods, 3.0)
            sm.run_steps(eng, backend, sims, ev)
            return eng.search_results(roots=pods)

        def continue_fn(keep_idx, picks, pods):
            if any(k < 0 for k in keep_idx):
                kept = eng.search_advance_refill(picks, keep_idx, fresh=pods, roots=pods)
            else:
                kept = eng.search_advance(picks, keep_idx, roots=pods)
            budget = budgets_for(kept, sims, eng.max_sims, "visit_target")
            eng.search_set_budget(budget)
            shorter.append(max(budget) < sims)
            sm.run_steps(eng, backend, max(budget), ev)
            res = eng.search_results(roots=pods)
            assert all(int(res["root_n"][g]) - 1 == sims for g in range(len(kept)) if int(res["sims_done"][g]) == budget[g])
            return res

        _same_episodes(got, selfplay.play(search_fn, eng, start[:G], AZ_ARGS, uniforms, continue_fn=continue_fn, refill=start[G:]))
        assert len(shorter) > 0
    finally:
        eng.close()
    # what the three modes ask the handle for
    asked, engine = [], az.engine
    az.engine = lambda min_games=1, min_sims=1, nn_dtype=None: asked.append(min_sims) or engine()
    try:
        for mode in (None, "per_game", "visit_target"):
            AlphaZero(model, opt, FourPlayerChess, dict(AZ_ARGS, sim_budget=mode), init, evaluator=dropin_cases.Eval("hash", R))._engine()
    finally:
        az.engine = engine
    assert asked == [2 * sims, 2 * sims, sims]
