"""FPC_RULES_VISITS and first-play urgency (include/fpc_engine.h): the cases that run both on the wavefront
emulator (tests/test_visits_emul.py) and on the GPU (tests/test_visits_gpu.py).  The model is tests/visits_model.py.
Everything is compared exactly; there is no tolerance in this file."""
import numpy as np

import evaluators
import fpc_ffi
import positions
import search_model as sm
import selfplay
import tuples
import visits_model as vm
from fpc_testlib import make_engine, roots_of
from oracle import orc
from terminal_cases import q5_root

INV_OF = {8: 2, 14: 3}
T, V, TRAINING, SELFPLAY = 16, 32, 31, 63
EINVAL, ECAPACITY = -1, -6


# ---- 1. closed form on the Q5 golden position ------------------------------------------------------------------------
def golden(backend, copies):
    """zero evaluator, 100 simulations, C = 3, rules 16 | 32: every simulation is completed and every one is a backup through
    the root, which was born with N = 0: root N = sims_done = 100, and the 18 children (born with N = 0; the first
    simulation expanded the root) hold 99 visits.  Rules 16 on the same handle afterwards: 101 and 18 + 99, as ever."""
    R, sims = 8, 100
    q5 = q5_root()
    ev = evaluators.make("zero", R)
    eng = make_engine(backend, R, INV_OF[R], max_games=copies, max_sims=sims)
    try:
        for rules, want_n, want_done, want_sum in ((T | V, 100, 100, 99), (T, 101, 100, 117)):
            roots = [fpc_ffi.board_from_lists(R, q5["turn"], q5["pl"]) for _ in range(copies)]
            eng.set_rule_bits(rules)
            res = sm.run_stepwise(eng, backend, roots, sims, 3.0, ev, 1)
            for g in range(copies):
                n = int(res["n_children"][g])
                assert n == 18, (rules, g)
                assert int(res["root_n"][g]) == want_n, (rules, g, int(res["root_n"][g]))
                assert int(res["sims_done"][g]) == want_done, (rules, g)
                assert int(res["visits"][g, :n].sum()) == want_sum, (rules, g)
    finally:
        eng.set_rules(0)
        eng.close()


# ---- 2. - 5. engine == model -------------------------------------------------------------------------------------------
#                        R   G  sims  near-end  seed    (the seeds are chosen on the CPU, from the model alone, so that the conditions hold)
SHAPES = {("8x8", V): (8, 8, 100, False, 800),
          ("8x8", V | 1): (8, 8, 100, False, 800),
          ("8x8", SELFPLAY): (8, 8, 100, True, 700),
          ("14x14", V): (14, 4, 60, False, 800),
          ("14x14", V | 1): (14, 4, 60, False, 800),
          ("14x14", SELFPLAY): (14, 4, 60, True, 700)}
NOISE_EPS, NOISE_SEED = 0.25, 5
_models = {}


def _gamma(G):
    return np.random.default_rng(NOISE_SEED).standard_gamma(0.3, size=(G, fpc_ffi.MAX_MOVES)).astype(np.float32)


def searched_model(shape, rules, K, fpu=None, noise=False):
    """(boards, Model after its search, Model.results()) of a case, computed once and never changed"""
    key = (shape, rules, K, fpu, noise)
    if key not in _models:
        R, G, sims, near_end, seed = SHAPES[(shape, rules)]
        boards = sm.positions(R, G, seed=seed, near_end=near_end, rules=rules & 15)
        model = vm.Model([orc.clone(b) for b in boards], R, INV_OF[R], 3.0, evaluators.make("hash", R), rules=rules, fpu=fpu,
                         vl=1.0, noise_eps=NOISE_EPS)
        if noise:
            model.set_noise(_gamma(G))
        assert model.search(sims, K) == 0
        _models[key] = (boards, model, model.results())
    return _models[key]


def _engine_search(backend, shape, rules, K, fused, fpu=None, noise=False):
    """the engine's search of a case: (engine, results); the caller closes the engine"""
    R, G, sims, _, _ = SHAPES[(shape, rules)]
    boards = searched_model(shape, rules, K, fpu, noise)[0]
    eng = make_engine(backend, R, INV_OF[R], max_games=G * K, max_sims=sims)
    try:
        eng.set_rule_bits(rules)
        if fpu is not None:
            eng.set_fpu(fpc_ffi.FPU_PARENT, fpu)
        if noise:
            eng.set_root_noise(_gamma(G), NOISE_EPS)
        res = sm.run_stepwise(eng, backend, roots_of(boards, R), sims, 3.0, evaluators.make("hash", R), K, vl=1.0, fused=fused)
    except BaseException:
        eng.close()
        raise
    return eng, res


def _close(eng):
    eng.set_leaves(1)
    eng.set_fpu(fpc_ffi.FPU_ZERO, 0.0)
    eng.set_root_noise(None, 0.0)
    eng.set_rules(0)
    eng.close()


def engine_vs_model(backend, shape, rules, K, fused, noise=False):
    """cases 2 - 4.  Condition: some root child was never visited (N = 0) -- born-0 and born-1 trees could otherwise agree in
    shape -- and, the invariant, root N == sims_done for every game"""
    _, model, want = searched_model(shape, rules, K, None, noise)
    assert model.counts["unvisited"] > 0, model.counts
    assert all(o["root_n"] == o["sims_done"] for o in want)
    assert all(sum(n for _, n in o["children"]) == o["root_n"] - 1 for o in want if o["children"] and not o["terminated"])
    eng, res = _engine_search(backend, shape, rules, K, fused, None, noise)
    try:
        sm.compare(eng, res, want, (shape, rules, K, fused, noise))
    finally:
        _close(eng)


def _trees(results):
    return [(o["root_n"], o["children"], o["w"].tolist()) for o in results]


def fpu_vs_model(backend, shape, reduction, K, fused):
    """case 5, rules 63.  Conditions: FPC_FPU_PARENT decided a selection (its argmax is not FPC_FPU_ZERO's at the same node),
    and the trees are not the FPC_FPU_ZERO trees of the same case"""
    _, model, want = searched_model(shape, SELFPLAY, K, reduction)
    assert model.counts["fpu_decided"] > 0, model.counts
    assert _trees(want) != _trees(searched_model(shape, SELFPLAY, K, None)[2])
    eng, res = _engine_search(backend, shape, SELFPLAY, K, fused, reduction)
    try:
        sm.compare(eng, res, want, (shape, "fpu", reduction, K, fused))
    finally:
        _close(eng)


# ---- 6. reuse, refill and budgets over three plies ---------------------------------------------------------------------
def _pick(res):
    """even games play the most-visited root child, odd games a child that was never visited (N = 0) if there is one, else
    the least-visited; games whose root has no child are left out.  {game: (flat, visits)}"""
    out = {}
    for g in range(len(res["n_children"])):
        n = int(res["n_children"][g])
        if n == 0:
            continue
        vis = res["visits"][g, :n]
        k = int(np.argmax(vis)) if g % 2 == 0 else int(np.argmin(vis))      # argmin: the first 0 if there is one
        out[g] = (int(res["flat"][g, k]), int(vis[k]))
    return out


def reuse_refill_budgets(backend):
    """Three plies of S simulations under rules 63 in a handle of S + 10.  Every advance keeps the games whose picked move
    does not end them and refills the other rows and one more; kept_visits == the model's, 0 for a fresh row and for a child
    that was never visited.  base[g] == kept[g]: a budget of max_sims - kept[g] is accepted for every game at once and
    refused with FPC_ECAPACITY when any one game asks for one more.  visit_target budgets (mcts.budgets_for with born = 0)
    then leave every root with exactly S visits."""
    from mcts import budgets_for
    R, G, S, plies, rules, seed = 8, 8, 40, 3, SELFPLAY, 700
    INV, max_sims = INV_OF[R], S + 10
    boards = sm.positions(R, G, seed=seed, near_end=True, rules=rules & 15)
    pool = sm.positions(R, (plies - 1) * G, seed=seed + 50, rules=rules & 15)
    ev = evaluators.make("hash", R)
    model = vm.Model([orc.clone(b) for b in boards], R, INV, 3.0, ev, rules=rules)
    eng = make_engine(backend, R, INV, max_games=G, max_sims=max_sims)
    cond = {"fresh": 0, "unvisited": 0, "visited": 0}
    try:
        eng.set_rule_bits(rules)
        eng.search_begin(roots_of(boards, R), 3.0)
        n_sims = S
        for ply in range(plies):
            sm.run_steps(eng, backend, n_sims, ev)
            res = eng.search_results()
            assert model.search(n_sims, 1) == 0
            sm.compare(eng, res, model.results(), ("reuse", ply), grand_every=3)
            alive = [g for g in range(len(model.roots)) if model.alive[g]]
            assert alive and all(int(res["root_n"][g]) == S for g in alive), (ply, res["root_n"])
            if ply + 1 == plies:
                break
            picked = _pick(res)
            src, flats = [], []
            for g in range(len(res["root_n"])):
                over = g not in picked
                if not over:
                    orc.set_rules(rules & 15)
                    try:
                        nxt, mrc = orc.take_action(orc.clone(model.roots[g].state), R, picked[g][0])
                        assert mrc == 0
                        over = orc.game_result(nxt, R, INV) != 0
                    finally:
                        orc.set_rules(0)
                if over or g == (3 * ply + 1) % G:
                    src.append(-1); flats.append(0)
                    cond["fresh"] += 1
                else:
                    src.append(g); flats.append(picked[g][0])
                    cond["unvisited" if picked[g][1] == 0 else "visited"] += 1
            fresh_o = [pool.pop() if s < 0 else None for s in src]
            kept = eng.search_advance_refill(flats, src, fresh=[None if b is None else roots_of([b], R)[0] for b in fresh_o])
            want_kept = model.advance_refill(src, flats, fresh_o)
            assert [int(k) for k in kept] == want_kept, (ply, "kept visits")
            for g, s in enumerate(src):
                if s < 0 or picked[s][1] == 0:
                    assert int(kept[g]) == 0, (ply, g)
                else:
                    assert int(kept[g]) == picked[s][1] > 0, (ply, g)
            after = eng.search_results()
            sm.compare(eng, after, model.results(), ("reuse", ply, "after the advance"), grand_every=0)
            assert all(int(after["n_children"][g]) == 0 for g in range(G) if int(kept[g]) == 0)
            # base[g] == kept[g]
            room = [max_sims - int(k) for k in kept]
            raw = lambda b: eng.L.fpc_search_set_budget(eng.h, (fpc_ffi.C.c_int * G)(*b), G)
            assert raw(room) == 0
            for g in (int(np.argmax(kept)), int(np.argmin(kept))):
                assert raw([r + (i == g) for i, r in enumerate(room)]) == ECAPACITY, (ply, g)
            budget = budgets_for(kept, S, max_sims, "visit_target", born=0)
            assert budget == [S - int(k) for k in kept]
            eng.search_set_budget(budget)
            model.set_budget(budget)
            n_sims = max(budget)
    finally:
        _close(eng)
    assert all(v > 0 for v in cond.values()), cond
    return cond


# ---- 7. fpc_search_play and tuples on roots whose children have no visit ----------------------------------------------
def play_and_tuples(backend):
    """One simulation (the zero evaluator) under rules 63 expands the root and visits no child.  fpc_search_play with
    u = 0, 0.5, 0.999 picks children 0, nc // 2, nc - 1 (S == 0: uniform over the children), temperature 0 picks child 0,
    and selfplay.sample_move says the same.  The collected tuple holds nc pairs of visit count 0; fpc_replay_batch gives a
    zero pi row, the bits of tuples.dense_pi."""
    from replay_cases import bits, decode
    R, rules, us = 8, SELFPLAY, [0.0, 0.5, 0.999]
    G = len(us)
    turn, entries = positions.start_entries(R)
    boards = [orc.board_from_dict(R, turn, [list(e) for e in entries]) for _ in range(G)]      # the start position, G times
    ev = evaluators.make("zero", R)
    eng = make_engine(backend, R, INV_OF[R], max_games=G, max_sims=4)
    try:
        eng.set_rule_bits(rules)
        res = sm.run_stepwise(eng, backend, roots_of(boards, R), 1, 3.0, ev, 1)
        ncs = [int(n) for n in res["n_children"]]
        assert min(ncs) >= 4
        assert all(int(res["root_n"][g]) == 1 and not res["visits"][g, :ncs[g]].any() for g in range(G))
        flats, results, _ = eng.search_play(1.0, us)
        want_k = [0, ncs[1] // 2, ncs[2] - 1]
        for g in range(G):
            kids = [int(f) for f in res["flat"][g, :ncs[g]]]
            assert int(flats[g]) == kids[want_k[g]], (g, int(flats[g]), kids)
            assert selfplay.sample_move(kids, [0] * ncs[g], 1.0, us[g]) == kids[want_k[g]], g
            assert selfplay.sample_move(kids, [0] * ncs[g], 0, us[g]) == kids[0], g
            assert int(results[g]) >= 0
        flats0, _, _ = eng.search_play(0.0, us)
        assert [int(f) for f in flats0] == [int(res["flat"][g, 0]) for g in range(G)]
        # tuples
        eng.tuples_reserve(G)
        eng.collect_tuples(None, 0)
        arr, n = eng.tuples_read()
        assert n == G
        recs = tuples.records_of(arr, n, R)
        for g, rec in enumerate(recs):
            assert [int(f) for f in rec["flat"]] == [int(f) for f in res["flat"][g, :ncs[g]]], g
            assert len(rec["visits"]) == ncs[g] and not np.asarray(rec["visits"]).any(), g
        eng.replay_reserve(0, G)
        eng.replay_push()
        _, pi, _ = decode(eng, backend, 0, list(range(G)))
        for g, rec in enumerate(recs):
            want = tuples.dense_pi(rec, eng.A).numpy()
            assert not want.any() and want.dtype == np.float32
            assert np.array_equal(bits(pi[g]), bits(want)), g
    finally:
        _close(eng)


# ---- 8. inert switches ----------------------------------------------------------------------------------------------------
def inert(backend):
    """fpc_search_set_fpu(PARENT, 0.25) under rules 31 (every child is born with N = 1: none is ever unvisited) leaves the
    rules-31 results as they are.  fpc_set_rules(64), fpc_set_rule_bits(64) and fpc_search_set_fpu's argument errors return FPC_EINVAL and change
    nothing: the rules-63 search with FPC_FPU_PARENT 0.25 that follows them gives the model's trees of that setting."""
    shape, K = "8x8", 1
    R, G, sims, near_end, seed = SHAPES[(shape, SELFPLAY)]
    boards = sm.positions(R, G, seed=seed, near_end=near_end, rules=15)
    ev = evaluators.make("hash", R)
    eng = make_engine(backend, R, INV_OF[R], max_games=G, max_sims=sims)
    try:
        eng.set_rules(TRAINING)
        off = sm.run_stepwise(eng, backend, roots_of(boards, R), sims, 3.0, ev, K)
        eng.set_fpu(fpc_ffi.FPU_PARENT, 0.25)
        on = sm.run_stepwise(eng, backend, roots_of(boards, R), sims, 3.0, ev, K)
        sm.same_results(off, on)
        ref = vm.Model([orc.clone(b) for b in boards], R, INV_OF[R], 3.0, ev, rules=TRAINING, fpu=0.25)
        assert ref.search(sims, K) == 0 and ref.counts["fpu_decided"] == 0 and ref.counts["unvisited"] == 0
        sm.compare(eng, on, ref.results(), "rules 31, fpu on")
        # refused calls change nothing
        eng.set_rule_bits(SELFPLAY)
        L, h = eng.L, eng.h
        assert L.fpc_set_rules(h, 64) == EINVAL and L.fpc_set_rules(h, -1) == EINVAL
        assert L.fpc_set_rule_bits(h, 64) == EINVAL and L.fpc_set_rule_bits(h, -1) == EINVAL and L.fpc_set_rule_bits(None, 63) == EINVAL
        assert L.fpc_set_rules(h, 32) == EINVAL and L.fpc_set_rules(h, 63) == EINVAL      # fpc_set_rules keeps its range 0..31
        for mode, red in ((2, 0.0), (-1, 0.0), (1, float("nan")), (1, float("inf")), (0, float("-inf"))):
            assert L.fpc_search_set_fpu(h, mode, red) == EINVAL, (mode, red)
        assert L.fpc_search_set_fpu(None, 1, 0.25) == EINVAL
        for ok in (0, 32, 33, 47, 48, 63):
            assert L.fpc_set_rule_bits(h, ok) == 0, ok
        res = sm.run_stepwise(eng, backend, roots_of(boards, R), sims, 3.0, ev, K)
        sm.compare(eng, res, searched_model(shape, SELFPLAY, K, 0.25)[2], "rules 63, fpu 0.25 after the refused calls")
        assert (fpc_ffi.RULES_VISITS, fpc_ffi.RULES_SELFPLAY) == (32, 63)
        assert fpc_ffi.RULES_SELFPLAY == fpc_ffi.RULES_TRAINING | fpc_ffi.RULES_VISITS
        assert (fpc_ffi.FPU_ZERO, fpc_ffi.FPU_PARENT) == (0, 1)
    finally:
        _close(eng)
