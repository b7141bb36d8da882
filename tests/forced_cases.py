"""Forced playouts and policy target pruning at the root (fpc_search_set_forced / fpc_search_targets; include/fpc_engine.h,
DESIGN.md 5.11): the cases that run both on the wavefront emulator (tests/test_forced_emul.py) and on the GPU
(tests/test_forced_gpu.py).  The model is tests/forced_model.py.  Everything is compared exactly; there is no tolerance in this
file."""
import numpy as np

import evaluators
import fpc_ffi
import forced_model as fm
import search_model as sm
import selfplay
import solver_cases as sc
import solver_model as so
from fpc_testlib import make_engine, roots_of
from oracle import orc

R, INV = 8, 2
NO_TERMINAL, SELFPLAY = 47, 63         # both hold FPC_RULES_PUCT | FPC_RULES_VISITS; only 63 holds FPC_RULES_TERMINAL (the solver)
EINVAL, ESTATE = -1, -9
FACTOR, EPS, FPU_RED, C_PUCT = 2.0, 0.25, 0.25, 3.0


def gamma_for(n, seed):
    return np.random.default_rng(seed).standard_gamma(0.3, size=(n, fpc_ffi.MAX_MOVES)).astype(np.float32)


def boards_for(pos, rules, G):
    """G orc boards: the start position G times, or the near-end positions of the solver cases' seeds"""
    if pos == "start":
        import positions
        turn, entries = positions.start_entries(R)
        return [orc.board_from_dict(R, turn, [list(e) for e in entries]) for _ in range(G)]
    return sm.positions(R, G, seed=sc.SHAPES[("8x8", sc.SELFPLAY if rules & 16 else sc.TRAINING)][3], near_end=True, rules=rules & 15)


def targets_equal(eng, model, tag):
    """fpc_search_targets == the model's targets, children in child order, zero past a root's children"""
    got = eng.search_targets()
    for g, want in enumerate(model.targets()):
        assert [int(x) for x in got[g, :len(want)]] == want, (tag, g, "targets", [int(x) for x in got[g, :len(want)]], want)
        assert not got[g, len(want):].any(), (tag, g, "past the children")


def compare_all(eng, res, model, tag, grand_every=1):
    """trees (search_results, grandchildren, sims_done), proofs and targets"""
    sc.compare_all(eng, res, model, tag, grand_every=grand_every)
    targets_equal(eng, model, tag)


def _setup(eng, rules, fpu, solver, factor, gamma):
    eng.set_rule_bits(rules)
    eng.set_solver(solver)
    eng.set_fpu(fpc_ffi.FPU_PARENT if fpu else fpc_ffi.FPU_ZERO, FPU_RED if fpu else 0.0)
    eng.set_forced(factor)
    eng.set_root_noise(gamma, EPS)


def _close(eng):
    eng.set_forced(0.0)
    eng.set_root_noise(None, 0.0)
    sc._close(eng)


def _model(cls, boards, rules, fpu, solver, gamma, **kw):
    model = cls([orc.clone(b) for b in boards], R, INV, C_PUCT, evaluators.make("hash", R), rules=rules, vl=1.0,
                fpu=FPU_RED if fpu else None, solver=solver, noise_eps=EPS, **kw)
    model.set_noise(gamma)
    return model


# ---- 1. engine == model -----------------------------------------------------------------------------------------------
#         pos     rules        fpu    solver  K   G  sims  noise seed   (sizes chosen on the CPU, from the model alone, so that
#                                                                        conditions() holds; under rules 47 the solver is inert)
CASES = [("near", SELFPLAY, False, False, 1, 4, 80, 1),
         ("near", SELFPLAY, False, False, 3, 4, 80, 2),
         ("near", SELFPLAY, True, False, 1, 4, 80, 3),
         ("near", SELFPLAY, True, False, 3, 4, 80, 4),
         ("near", SELFPLAY, False, True, 1, 4, 80, 5),
         ("near", SELFPLAY, False, True, 3, 4, 80, 6),
         ("near", SELFPLAY, True, True, 1, 4, 80, 7),
         ("near", SELFPLAY, True, True, 3, 4, 80, 8),
         ("near", NO_TERMINAL, False, False, 1, 4, 80, 9),
         ("near", NO_TERMINAL, True, True, 3, 4, 80, 10),
         ("start", SELFPLAY, False, False, 1, 3, 64, 11),
         ("start", SELFPLAY, True, True, 3, 3, 64, 12),
         ("start", SELFPLAY, True, False, 1, 3, 64, 13),
         ("start", SELFPLAY, False, True, 3, 3, 64, 14),
         ("start", NO_TERMINAL, True, False, 3, 3, 64, 15),
         ("start", NO_TERMINAL, False, True, 1, 3, 64, 16)]
IDS = ["%s-rules%d-fpu%d-solver%d-K%d" % (c[0], c[1], c[2], c[3], c[4]) for c in CASES]
_models = {}


def searched_model(case):
    """(boards, gamma, Model after its search) of a case, computed once and never changed"""
    if case not in _models:
        pos, rules, fpu, solver, K, G, sims, seed = case
        boards = boards_for(pos, rules, G)
        gamma = gamma_for(G, seed)
        model = _model(fm.Model, boards, rules, fpu, solver, gamma, forced=FACTOR)
        assert model.forced_in_effect() and model.in_effect() == (solver and rules == SELFPLAY)
        assert model.search(sims, K) == 0
        _models[case] = (boards, gamma, model)
    return _models[case]


def conditions():
    """the cap on the inputs, asserted from the model alone: in every case the forced rule decided a selection and the
    pruning took a visit out; across the list a child with visits was pruned to zero"""
    to_zero = 0
    for case in CASES:
        _, _, model = searched_model(case)
        assert model.counts["forced_decided"] >= 1 and model.counts["pruned_visits"] >= 1, (case, model.counts)
        to_zero += model.counts["pruned_to_zero"]
    assert to_zero >= 1
    return to_zero


def engine_vs_model(backend, case, fused):
    pos, rules, fpu, solver, K, G, sims, _ = case
    boards, gamma, model = searched_model(case)
    eng = make_engine(backend, R, INV, max_games=G * K, max_sims=sims)
    try:
        _setup(eng, rules, fpu, solver, FACTOR, gamma)
        res = sm.run_stepwise(eng, backend, roots_of(boards, R), sims, C_PUCT, evaluators.make("hash", R), K, vl=1.0, fused=fused)
        compare_all(eng, res, model, (case, fused))
        assert sc._alive(res) == model.alive or not rules & 16, (case, "alive")
    finally:
        _close(eng)


# ---- 2. reuse -----------------------------------------------------------------------------------------------------------
REUSE = dict(case=CASES[6], more=40, useed=11, gseed=31)


def reuse(backend, refill):
    """After the search every game that can go on is advanced on the model's pick at temperature 1 -- fpc_search_advance, or
    fpc_search_advance_refill with two fresh rows between the kept ones -- with new root noise; then 40 more simulations.
    Condition: the forced rule decides a selection at a NEW root that arrived with children (its kept counts are what the
    rule reads), and the targets after the second search are pruned."""
    c = REUSE
    pos, rules, fpu, solver, K, G, sims, _ = c["case"]
    ev = evaluators.make("hash", R)
    boards = boards_for(pos, rules, G)
    gamma = gamma_for(G, c["case"][7])
    model = _model(fm.Model, boards, rules, fpu, solver, gamma, forced=FACTOR)
    assert model.search(sims, 1) == 0
    u = np.random.default_rng(c["useed"]).random(G)
    keep = [g for g in range(G) if model.roots[g].children]
    flats = {g: model.roots[g].children[model.pick(g, 1.0, float(u[g]))].flat for g in keep}
    fresh_o = sm.positions(R, 2, seed=750, rules=rules & 15)
    if refill:
        src = keep[:2] + [-1] + keep[2:] + [-1]
        fresh = [None if s >= 0 else fresh_o.pop() for s in src]
    else:
        src, fresh = list(keep), None
    fl = [flats[s] if s >= 0 else 0 for s in src]
    n_new = len(src)
    gamma2 = gamma_for(n_new, c["gseed"])
    eng = make_engine(backend, R, INV, max_games=max(G, n_new), max_sims=sims + c["more"])
    try:
        _setup(eng, rules, fpu, solver, FACTOR, gamma)
        res = sm.run_stepwise(eng, backend, roots_of(boards, R), sims, C_PUCT, ev, 1)
        compare_all(eng, res, model, "reuse: before the advance", grand_every=0)
        eng.set_root_noise(gamma2, EPS)
        model.set_noise(gamma2)
        if refill:
            kept = eng.search_advance_refill(fl, src, fresh=[None if b is None else roots_of([b], R)[0] for b in fresh])
            want_kept = model.advance_refill(src, fl, fresh)
        else:
            kept = eng.search_advance(fl, src)
            want_kept = model.advance(src, fl)
        assert [int(k) for k in kept] == want_kept, "kept visits"
        targets_equal(eng, model, "reuse: after the advance, before any selection")
        arrived = [g for g in range(n_new) if model.roots[g].children and model.status(model.roots[g]) == so.UNKNOWN]
        assert arrived                                                                 # condition
        before = model.counts["forced_decided"]
        sm.run_steps(eng, backend, c["more"], ev)
        res = eng.search_results()
        assert model.search(c["more"], 1) == 0
        assert model.counts["forced_decided"] > before and model.counts["pruned_visits"] >= 1, model.counts      # conditions
        compare_all(eng, res, model, "reuse: 40 more simulations", grand_every=2)
    finally:
        _close(eng)


# ---- 3. tuples and play -------------------------------------------------------------------------------------------------
def _tuples_equal(eng, model, tag):
    """one fpc_collect_tuples of the finished search: the records' sparse pi holds (flat, target) of every root child"""
    G = len(model.roots)
    eng.tuples_reserve(G)
    eng.collect_tuples(None, 0)
    arr, n = eng.tuples_read()
    assert n == G
    for g, want in enumerate(model.targets()):
        kids = model.roots[g].children
        assert int(arr[g].n) == len(kids), (tag, g)
        assert [int(arr[g].flat[k]) for k in range(len(kids))] == [c.flat for c in kids], (tag, g, "flat")
        assert [int(arr[g].visits[k]) for k in range(len(kids))] == want, (tag, g, "visits")
        assert not any(arr[g].visits[k] for k in range(len(kids), len(arr[g].visits))), (tag, g, "past the children")
    eng.tuples_reserve(0)


def _uniform_that_tells(flats, visits, tgt):
    """a uniform for which the draw at temperature 1 from the targets is not the draw from the stored visits, or None"""
    for j in range(400):
        x = (j + 0.5) / 400
        if selfplay.sample_move(flats, tgt, 1.0, x) != selfplay.sample_move(flats, visits, 1.0, x):
            return x
    return None


def tuples_and_play(backend, case):
    """fpc_collect_tuples holds the targets; fpc_search_play at temperature 1 and 0 == the model's pick (the solver's pick for
    a proven root, else the draw from the targets), result / next == today's calls on the picked move.  Wherever the
    pruning changed a root's counts the uniform is one for which the draw from the stored visits picks differently."""
    from play_cases import _check_moves
    pos, rules, fpu, solver, K, G, sims, _ = case
    boards, gamma, model = searched_model(case)
    u = list(np.random.default_rng(23).random(G))
    told = 0
    for g, tgt in enumerate(model.targets()):
        kids = model.roots[g].children
        if kids and not (model.in_effect() and model.status(model.roots[g]) in (so.WIN, so.DRAW)):
            x = _uniform_that_tells([c.flat for c in kids], [c.N for c in kids], tgt)
            if x is not None:
                u[g], told = x, told + 1
    assert told >= 1                                                                   # condition
    eng = make_engine(backend, R, INV, max_games=G * K, max_sims=sims)
    try:
        _setup(eng, rules, fpu, solver, FACTOR, gamma)
        res = sm.run_stepwise(eng, backend, roots_of(boards, R), sims, C_PUCT, evaluators.make("hash", R), K, vl=1.0)
        compare_all(eng, res, model, ("play", case), grand_every=0)
        _tuples_equal(eng, model, ("tuples", case))
        live = [g for g in range(G) if model.roots[g].children]
        for T in (1.0, 0.0):
            want = [model.roots[g].children[model.pick(g, T, u[g])].flat if g in live else -1 for g in range(G)]
            flats, results, pods = eng.search_play(T, u)
            assert [int(f) for f in flats] == want, (case, T)
            if len(live) == G:
                _check_moves(eng, res, flats, results, pods, ("play", case, T))
            if T == 0.0:                             # the argmax is unchanged in outcome: T_b = N_b is still the first largest
                drawn = [g for g in live if not (model.in_effect() and model.status(model.roots[g]) in (so.WIN, so.DRAW))]
                assert [int(res["flat"][g, int(np.argmax(res["visits"][g]))]) for g in drawn] == [want[g] for g in drawn]
        res2 = eng.search_results()                  # nothing was written into the tree
        sm.same_results(res, res2)
    finally:
        _close(eng)


def proven_root_case():
    """the case of the list in which some root is proven WIN or DRAW with the solver in effect (condition: there is one)"""
    for case in CASES:
        if case[3] and case[1] == SELFPLAY and case[4] == 1:
            _, _, model = searched_model(case)
            if any(st in (so.WIN, so.DRAW) and model.roots[g].children for g, st in enumerate(model.proofs()[0])):
                return case
    raise AssertionError("no case with a root proven WIN or DRAW")


# ---- 4. the self-play loop --------------------------------------------------------------------------------------------
def selfplay_loop(backend):
    """selfplay.play from the start position under rules 63 with root noise and forcing on: the host path with targets=True
    and the device path play the same games and record the same entries -- the pruned counts -- and, condition, not the
    entries of the host path without the flag"""
    from treereuse_cases import _episode_fns
    G, sims, L, rules = 3, 32, 2, SELFPLAY
    boards = boards_for("start", rules, G)
    ev = evaluators.make("hash", R)
    args = {"temperature": 1.0, "max_game_length": L, "heuristic_weight": 0.5}
    uniforms = np.random.default_rng(5).random((L, G)).tolist()
    eng = make_engine(backend, R, INV, max_games=G, max_sims=sims)
    try:
        _setup(eng, rules, True, False, FACTOR, gamma_for(G, 41))
        search_fn, _ = _episode_fns(eng, backend, ev, sims)
        host = selfplay.play(search_fn, eng, roots_of(boards, R), args, uniforms, targets=True)
        dev = selfplay.play(search_fn, eng, roots_of(boards, R), args, uniforms, device_play=True, targets=True)
        plain = selfplay.play(search_fn, eng, roots_of(boards, R), args, uniforms)
    finally:
        _close(eng)
    from treereuse_cases import _same_episodes
    _same_episodes(host, dev)
    first = [(e.entries[0][1].tolist(), e.entries[0][2].tolist()) for e in host]
    raw = [(e.entries[0][1].tolist(), e.entries[0][2].tolist()) for e in plain]
    assert [f for f, _ in first] == [f for f, _ in raw] and any(sum(t) < sum(v) for (_, t), (_, v) in zip(first, raw))


# ---- 5. off means off -----------------------------------------------------------------------------------------------------
OFF = [(0.0, SELFPLAY), (FACTOR, 0), (FACTOR, 15), (FACTOR, 31)]


def off_means_off(backend, factor, rules):
    """factor 0 under rules 63, factor 2 under rules 0, 15 and 31 (no FPC_RULES_VISITS, or no FPC_RULES_PUCT either): trees,
    tuples and play are solver_model.Model's with the stored visits, and fpc_search_targets reports the stored visits"""
    G, sims = 4, 40
    ev = evaluators.make("hash", R)
    boards = boards_for("near", rules, G)
    gamma = gamma_for(G, 51)
    ref = _model(so.Model, boards, rules, True, True, gamma)
    assert ref.search(sims, 1) == 0
    eng = make_engine(backend, R, INV, max_games=G, max_sims=sims)
    try:
        _setup(eng, rules, True, True, factor, gamma)
        res = sm.run_stepwise(eng, backend, roots_of(boards, R), sims, C_PUCT, ev, 1)
        sc.compare_all(eng, res, ref, ("off means off", factor, rules))
        got = eng.search_targets()
        assert np.array_equal(got, res["visits"]), (factor, rules)
        eng.tuples_reserve(G)
        eng.collect_tuples(None, 0)
        arr, n = eng.tuples_read()
        u = list(np.random.default_rng(7).random(G))
        for T in (1.0, 0.0):
            flats, _, _ = eng.search_play(T, u)
            for g in range(G):
                nc = int(res["n_children"][g])
                assert [int(arr[g].visits[k]) for k in range(nc)] == [int(v) for v in res["visits"][g, :nc]], (factor, rules, g)
                kids = ref.roots[g].children
                want = kids[ref.pick(g, T, u[g])].flat if kids else -1
                assert int(flats[g]) == want, (factor, rules, T, g)
    finally:
        _close(eng)


# ---- 6. refusals ----------------------------------------------------------------------------------------------------------
def refusals(backend):
    boards = boards_for("start", SELFPLAY, 2)
    eng = make_engine(backend, R, INV, max_games=2, max_sims=8)
    try:
        L, h = eng.L, eng.h
        out = np.zeros((2, 4), np.int32)
        assert L.fpc_search_targets(h, 4, out.ctypes.data) == ESTATE                     # before any search, as fpc_search_results
        for bad in (-1.0, -1e-300, float("nan"), float("inf"), float("-inf")):
            assert L.fpc_search_set_forced(h, bad) == EINVAL, bad
        assert L.fpc_search_set_forced(None, 2.0) == EINVAL
        eng.set_rule_bits(SELFPLAY)
        eng.search_begin(roots_of(boards, R), C_PUCT)
        assert not eng.search_targets().any()                                            # childless roots: all zero
        assert L.fpc_search_set_forced(h, 2.0) == 0                                      # after begin, before the first selection
        eng.search_select()
        assert L.fpc_search_set_forced(h, 0.0) == ESTATE and L.fpc_search_set_forced(h, 2.0) == ESTATE
        assert L.fpc_search_targets(h, -1, out.ctypes.data) == EINVAL
        assert L.fpc_search_targets(h, 4, out.ctypes.data) == 0                          # does not finish the search ...
        assert L.fpc_search_set_forced(h, 0.0) == ESTATE                                 # ... the window is still open
        eng.search_results()
        assert L.fpc_search_set_forced(h, 0.0) == 0 and L.fpc_search_set_forced(h, 2.0) == 0
        assert L.fpc_search_set_forced(h, -2.0) == EINVAL                                # no state changed: still 2
    finally:
        _close(eng)


# ---- 7. fpc_search_run on the internal network (GPU only: the emulator has no network) ------------------------------------
RUN = dict(R=8, hidden=128, dtype=1, layout=2, rules=SELFPLAY, sims=48, seed=700, gseed=61)
_run = {}


def run_case(policy_head):
    """everything of the case that needs no GPU, computed once: solver_cases.RUN's shape -- legal_head_cases.search_setup's
    integer network (its float64 reference IS the evaluator) on twelve near-end roots -- and the FORCED model's search with
    the full or the legal-only head under rules 63 with root noise, FPU and the solver on"""
    import legal_head_cases as lc
    c = RUN
    if "setup" not in _run:
        boards = sm.positions(c["R"], lc.G, seed=c["seed"], near_end=True, rules=c["rules"] & 15)
        _run["setup"] = lc.search_setup(c["R"], c["hidden"], c["dtype"], boards=boards, rules=c["rules"] & 15)
        _run["gamma"] = gamma_for(lc.G, c["gseed"])
    if policy_head not in _run:
        m, boards, s, ev = _run["setup"]
        model = fm.Model([orc.clone(b) for b in boards], c["R"], INV, C_PUCT, ev, rules=c["rules"], policy_head=policy_head,
                         fpu=FPU_RED, solver=True, noise_eps=EPS, forced=FACTOR)
        model.set_noise(_run["gamma"])
        assert model.search(c["sims"], 1) == 0
        assert model.counts["forced_decided"] >= 1 and model.counts["pruned_visits"] >= 1, model.counts
        _run[policy_head] = model
    m, boards, s, _ = _run["setup"]
    return m, boards, s, _run["gamma"], _run[policy_head]
