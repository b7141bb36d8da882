"""The MCTS solver (fpc_search_set_solver / fpc_search_proofs; include/fpc_engine.h): the cases that run both
on the wavefront emulator (tests/test_solver_emul.py) and on the GPU (tests/test_solver_gpu.py).  The model is
tests/solver_model.py.  Everything is compared exactly; there is no tolerance in this file."""
import numpy as np

import evaluators
import fpc_ffi
import search_model as sm
import selfplay
import solver_model as so
import terminal_model as tm
import visits_model as vm
from fpc_testlib import make_engine, roots_of
from oracle import orc
from terminal_cases import won_root

INV_OF = {8: 2, 14: 3}
TRAINING, SELFPLAY = 31, 63
EINVAL, ESTATE = -1, -9


def proofs_equal(eng, model, tag):
    """fpc_search_proofs == the model's statuses, roots and children in child order, zero past a root's children"""
    root, child = eng.search_proofs()
    want_r, want_c = model.proofs()
    assert [int(x) for x in root] == want_r, (tag, "root proofs", [int(x) for x in root], want_r)
    for g, kids in enumerate(want_c):
        assert [int(x) for x in child[g, :len(kids)]] == kids, (tag, g, "child proofs")
        assert not child[g, len(kids):].any(), (tag, g, "past the children")


def compare_all(eng, res, model, tag, grand_every=1):
    """trees (sm.compare: sims_done included), alive and proofs"""
    sm.compare(eng, res, model.results(), tag, grand_every=grand_every)
    rc, raw = sm.results_raw(eng)
    assert rc == 0, (tag, rc)
    assert [int(x) for x in raw["sims_done"]] == model.sims_done, (tag, "sims_done")
    proofs_equal(eng, model, tag)


def _close(eng):
    eng.set_leaves(1)
    eng.set_live_rows(False)
    eng.set_solver(False)
    eng.set_fpu(fpc_ffi.FPU_ZERO, 0.0)
    eng.set_rules(0)
    eng.close()


# ---- 1. by hand: terminal_cases.won_root ------------------------------------------------------------------------------
def _root_children_by_hand(R, INV, rules):
    """won_root's root children judged with the oracle alone, in the order of operations of a search (GetGameResult and
    GetLegalMoves on the root, then each move made on that state): (flats ascending, value of each child for ITS side to
    move: +1.0 / -1.0 / 0.0 where the game is over there, None where it goes on)"""
    orc.set_rules(rules & 15)
    try:
        root = won_root()
        assert orc.game_result(root, R, INV) == 0
        flats = sorted(set(m[2] for m in orc.legal_moves(root, R, INV)))
        vals = []
        for fl in flats:
            nb, rc = orc.take_action(root, R, fl)
            assert rc == 0
            res = orc.game_result(nb, R, INV)
            vals.append(None if res == 0 else tm.terminal_value(res, nb.turn))
    finally:
        orc.set_rules(0)
    return flats, vals


def by_hand(backend, rules):
    """won_root, the zero evaluator, 30 simulations, rules 31 and 63.  Six of Red's 18 moves are answered by a move that
    takes a king (children 0, 2, 3, 4, 11, 12: the game is over there and won by the side to move).  With the solver on,
    every one of them that the search reaches is proven WIN by its first visit and never visited again: N = born + 1
    (2 under rules 31, 1 under rules 63).
    What the position does NOT allow, though the issue that asked for this case expected it: the root does not stay
    unknown, and not all six are reached.  Child 10 is a position LOST for its side to move (Red's move wins on the spot), so
    its first visit -- simulation 12: the root's expansion, ten children, then this one -- proves the root WIN.  From
    then on the game idles: sims_done == 12, children 11.. keep N = born, status unknown.  With the switch off the king
    takers get no second visit either, because child 10 (q = +1) draws every later simulation: N = born + 19.  That is the
    difference asserted from the model here: child 10 has one visit with the solver and nineteen without."""
    R, INV, sims = 8, 2, 30
    ev = evaluators.make("zero", R)
    flats, vals = _root_children_by_hand(R, INV, rules)
    takers = [i for i, v in enumerate(vals) if v == 1.0]
    assert takers == [0, 2, 3, 4, 11, 12] and len(flats) == 18 and vals.index(-1.0) == 10 and vals.count(-1.0) == 1
    born = 0 if rules & 32 else 1
    off = so.Model([won_root()], R, INV, 3.0, ev, rules=rules, solver=False)
    on = so.Model([won_root()], R, INV, 3.0, ev, rules=rules, solver=True)
    assert off.search(sims, 1) == 0 and on.search(sims, 1) == 0
    assert [c.flat for c in on.roots[0].children] == flats
    assert off.roots[0].children[10].N == born + 19 and on.roots[0].children[10].N == born + 1      # conditions, from the model
    assert off.sims_done == [sims] and on.sims_done == [12] and on.counts["idle_proven"] == sims - 12
    eng = make_engine(backend, R, INV, max_games=1, max_sims=sims)
    try:
        eng.set_rule_bits(rules)
        eng.set_solver(True)
        res = sm.run_stepwise(eng, backend, roots_of([won_root()], R), sims, 3.0, ev, 1)
        compare_all(eng, res, on, ("by hand", rules))
        root, child = eng.search_proofs()
        assert int(res["n_children"][0]) == 18 and int(res["sims_done"][0]) == 12
        assert int(root[0]) == so.WIN and int(child[0, 10]) == so.LOSS and int(res["visits"][0, 10]) == born + 1
        for i in takers:
            if i < 10:                           # reached before the root was proven: one backup each, proven WIN
                assert int(child[0, i]) == so.WIN and int(res["visits"][0, i]) == born + 1, (rules, i)
            else:                                # never reached
                assert int(child[0, i]) == so.UNKNOWN and int(res["visits"][0, i]) == born, (rules, i)
        assert [int(x) for x in child[0, :18]].count(so.WIN) == 4
        # the switch off on the same handle: child 10 takes the nineteen later simulations
        eng.set_solver(False)
        res = sm.run_stepwise(eng, backend, roots_of([won_root()], R), sims, 3.0, ev, 1)
        sm.compare(eng, res, off.results(), ("by hand, switch off", rules))
        assert int(res["visits"][0, 10]) == born + 19 and int(res["sims_done"][0]) == sims
    finally:
        _close(eng)


# ---- 2. engine == model on near-end positions -------------------------------------------------------------------------
#                             R   G  sims  seed    (seeds chosen on the CPU, from the solver model alone; they are the seeds of
#                                                   terminal_cases / visits_cases, and conditions() holds for them)
SHAPES = {("8x8", TRAINING): (8, 8, 100, 700),
          ("8x8", SELFPLAY): (8, 8, 100, 703),
          ("14x14", SELFPLAY): (14, 4, 60, 700)}
CASES2 = [(shape, rules, K) for (shape, rules) in SHAPES for K in (1, 4)]
_models = {}


def near_end_boards(shape, rules):
    R, G, _, seed = SHAPES[(shape, rules)]
    return sm.positions(R, G, seed=seed, near_end=True, rules=rules & 15)


def searched_model(shape, rules, K, solver=True):
    """(boards, Model after its search) of a case, computed once and never changed"""
    key = (shape, rules, K, solver)
    if key not in _models:
        R, G, sims, _ = SHAPES[(shape, rules)]
        boards = near_end_boards(shape, rules)
        model = so.Model([orc.clone(b) for b in boards], R, INV_OF[R], 3.0, evaluators.make("hash", R), rules=rules, vl=1.0,
                         solver=solver)
        assert model.search(sims, K) == 0
        model.check_invariants()
        _models[key] = (boards, model)
    return _models[key]


def conditions():
    """what the cases of 2 must exercise between them, asserted from the solver model alone"""
    roots, proven, counts = set(), set(), {"proven_backups_interior": 0, "excluded": 0, "idle_while_expanding": 0}
    for shape, rules, K in CASES2:
        _, model = searched_model(shape, rules, K)
        roots |= set(model.proofs()[0])
        proven |= set(model.counts["proven"])
        for k in counts:
            counts[k] += model.counts[k]
    assert {so.WIN, so.LOSS, so.DRAW} <= roots, roots                                  # a root proven each way
    assert (so.LOSS, "scan") in proven and (so.DRAW, "scan") in proven, proven         # the scan, both outcomes
    assert (so.WIN, "loss_child") in proven, proven
    assert counts["proven_backups_interior"] > 0 and counts["excluded"] > 0, counts   # a backup from a proven NON-terminal node
    assert counts["idle_while_expanding"] > 0, counts                                  # a game idles while another expands
    return roots, proven, counts


def engine_vs_model(backend, shape, rules, K, fused):
    R, G, sims, _ = SHAPES[(shape, rules)]
    boards, model = searched_model(shape, rules, K)
    eng = make_engine(backend, R, INV_OF[R], max_games=G * K, max_sims=sims)
    try:
        eng.set_rule_bits(rules)
        eng.set_solver(True)
        res = sm.run_stepwise(eng, backend, roots_of(boards, R), sims, 3.0, evaluators.make("hash", R), K, vl=1.0, fused=fused)
        compare_all(eng, res, model, (shape, rules, K, fused))
        assert _alive(res) == model.alive, (shape, rules, K, "alive")
    finally:
        _close(eng)


def _alive(res):
    """The C-ABI reports no alive flag.  fpc_search_results raised no error, and under FPC_RULES_TERMINAL only a terminal
    root takes a game out of the search: the game whose root has no child after its one completed backup.  (A game that idles
    on a proven root HAS children and stays alive; sims_done, compared exactly, shows that it went on or stopped as the
    model's did.)"""
    return [not (int(res["n_children"][g]) == 0 and int(res["sims_done"][g]) >= 1) for g in range(len(res["root_n"]))]


# ---- 3. reuse -----------------------------------------------------------------------------------------------------------
REUSE = dict(shape="8x8", rules=SELFPLAY, sims=100, more=40, useed=11)


def _reuse_model():
    """the model's 8x8 search, its picks at temperature 1 and the plan of both advances"""
    c = REUSE
    R, G, _, _ = SHAPES[(c["shape"], c["rules"])]
    boards = near_end_boards(c["shape"], c["rules"])
    model = so.Model([orc.clone(b) for b in boards], R, INV_OF[R], 3.0, evaluators.make("hash", R), rules=c["rules"], solver=True)
    assert model.search(c["sims"], 1) == 0
    u = np.random.default_rng(c["useed"]).random(G)
    picks = [model.pick(g, 1.0, float(u[g])) for g in range(G)]
    assert all(p is not None for p in picks)
    flats = [model.roots[g].children[picks[g]].flat for g in range(G)]
    return boards, model, flats


def reuse(backend, refill):
    """After the 8x8 search every game is advanced on its model pick -- fpc_search_advance, or fpc_search_advance_refill with
    two fresh rows between the kept ones.  fpc_search_proofs == the model BEFORE any selection (the statuses of the old
    second level are now the root children's), then 40 more simulations.  Condition: a new root arrives proven with
    children; it completes nothing (sims_done == 0) and its tree is not touched."""
    c = REUSE
    R, G, _, _ = SHAPES[(c["shape"], c["rules"])]
    INV = INV_OF[R]
    ev = evaluators.make("hash", R)
    boards, model, flats = _reuse_model()
    fresh_o = sm.positions(R, 2, seed=750, rules=c["rules"] & 15)
    if refill:
        src = [0, 1, -1, 2, 3, 4, -1, 5, 6, 7]
        fl = [flats[s] if s >= 0 else 0 for s in src]
        fresh = [None if s >= 0 else fresh_o.pop() for s in src]
    else:
        src, fl, fresh = None, flats, None
    n_new = len(fl)
    eng = make_engine(backend, R, INV, max_games=n_new, max_sims=c["sims"] + c["more"])
    try:
        eng.set_rule_bits(c["rules"])
        eng.set_solver(True)
        res = sm.run_stepwise(eng, backend, roots_of(boards, R), c["sims"], 3.0, ev, 1)
        compare_all(eng, res, model, "reuse: before the advance", grand_every=0)
        if refill:
            kept = eng.search_advance_refill(fl, src, fresh=[None if b is None else roots_of([b], R)[0] for b in fresh])
            want_kept = model.advance_refill(src, fl, fresh)
        else:
            kept = eng.search_advance(fl, src)
            want_kept = model.advance(src, fl)
        assert [int(k) for k in kept] == want_kept, "kept visits"
        proofs_equal(eng, model, "reuse: after the advance, before any selection")
        want_r, want_c = model.proofs()
        arrived = [g for g in range(n_new) if want_r[g] != so.UNKNOWN and model.roots[g].children]
        assert arrived, want_r                                                         # condition
        assert any(any(k) for k in want_c), "a second-level status became visible"
        before = {g: model.results()[g] for g in arrived}
        sm.run_steps(eng, backend, c["more"], ev)
        res = eng.search_results()
        assert model.search(c["more"], 1) == 0
        model.check_invariants()
        compare_all(eng, res, model, "reuse: 40 more simulations", grand_every=2)
        for g in arrived:
            assert int(res["sims_done"][g]) == 0 and model.results()[g]["children"] == before[g]["children"], g
    finally:
        _close(eng)


# ---- 4. live rows and budgets -------------------------------------------------------------------------------------------
def live_rows_and_budgets(backend):
    """8x8, rules 63, K = 2, per-game budgets, the solver on: with fpc_search_set_live_rows(1) the trees and proofs are those
    of the switch off (and the model's), and *n_live of every step is the model's live count"""
    import live_rows_cases as lc
    shape, rules, K = "8x8", SELFPLAY, 2
    R, G, sims, _ = SHAPES[(shape, rules)]
    budget = [100, 30, 100, 7, 100, 0, 60, 100]
    sched = sm.schedule(sims, K)
    boards = near_end_boards(shape, rules)
    ev = evaluators.make("hash", R)
    model = so.Model([orc.clone(b) for b in boards], R, INV_OF[R], 3.0, ev, rules=rules, vl=1.0, solver=True)
    model.set_budget(budget)
    assert model.search(sims, K) == 0
    assert model.counts["idle_proven"] > 0 and model.counts["proven_backups"] > 0
    assert any(s["idle"] for s in model.steps) and any(s["proven_idle"] for s in model.steps)
    eng = make_engine(backend, R, INV_OF[R], max_games=G * K, max_sims=sims)
    try:
        eng.set_rule_bits(rules)
        eng.set_solver(True)
        runs = {}
        for on in (False, True):
            eng.set_leaves(K, 1.0)
            eng.search_begin(roots_of(boards, R), 3.0)
            runs[on] = lc.one_ply(eng, backend, on, sched, budget, ev)
            compare_all(eng, runs[on][0], model, ("live rows", on))
            assert [n for n, _ in runs[on][2]] == [len(s["live"]) for s in model.steps], ("n_live per step", on)
            runs[on] = runs[on] + (eng.search_proofs(),)
        lc.same_search(runs[False][:3], runs[True][:3])
        assert all(np.array_equal(a, b) for a, b in zip(runs[False][3], runs[True][3]))
    finally:
        _close(eng)


# ---- 5. play ------------------------------------------------------------------------------------------------------------
def _other_uniform(visits, forced):
    """a uniform inside the interval of a child other than `forced` at temperature 1 (weights = visits), or None"""
    total = float(sum(int(v) for v in visits))
    c = 0.0
    for k, v in enumerate(visits):
        if k != forced and int(v) > 0:
            return (c + 0.5 * int(v)) / total
        c += int(v)
    return None


def play(backend, rules):
    """fpc_search_play on the finished 8x8 search, temperatures 1 and 0: flat == model.pick, result / next == today's calls
    on the picked move.  For every game with a root proven WIN or DRAW the uniform lies inside the interval of ANOTHER
    child: today's draw picks differently (asserted from the model).  selfplay.sample_move with the proofs gives the same."""
    from play_cases import _check_moves
    shape = "8x8"
    R, G, sims, _ = SHAPES[(shape, rules)]
    boards, model = searched_model(shape, rules, 1)
    want_r, want_c = model.proofs()
    u = list(np.random.default_rng(23).random(G))
    forced_games = []
    for g in range(G):
        kids = model.roots[g].children
        if want_r[g] in (so.WIN, so.DRAW):
            forced = model.pick(g, 1.0, 0.5)
            assert want_c[g][forced] == (so.LOSS if want_r[g] == so.WIN else so.DRAW)
            ug = _other_uniform([c.N for c in kids], forced)
            if ug is not None:
                u[g] = ug
                today = selfplay.sample_move([c.flat for c in kids], [c.N for c in kids], 1.0, ug)
                assert today != kids[forced].flat                                      # the rule overrides the draw
                forced_games.append(g)
    assert forced_games                                                                # condition
    eng = make_engine(backend, R, INV_OF[R], max_games=G, max_sims=sims)
    try:
        eng.set_rule_bits(rules)
        eng.set_solver(True)
        res = sm.run_stepwise(eng, backend, roots_of(boards, R), sims, 3.0, evaluators.make("hash", R), 1)
        compare_all(eng, res, model, ("play", rules), grand_every=0)
        root, child = eng.search_proofs()
        for T in (1.0, 0.0):
            want = [model.roots[g].children[model.pick(g, T, u[g])].flat for g in range(G)]
            flats, results, pods = eng.search_play(T, u)
            assert [int(f) for f in flats] == want, (rules, T)
            _check_moves(eng, res, flats, results, pods, ("play", rules, T))
            host = [selfplay.sample_move(res["flat"][g, :int(res["n_children"][g])], res["visits"][g, :int(res["n_children"][g])], T,
                                         u[g], root_proof=root[g], child_proof=child[g]) for g in range(G)]
            assert host == want, (rules, T, "host path")
        # the switch off: today's draw, from the same tree
        eng.set_solver(False)
        flats, _, _ = eng.search_play(1.0, u)
        for g in range(G):
            kids = model.roots[g].children
            assert int(flats[g]) == selfplay.sample_move([c.flat for c in kids], [c.N for c in kids], 1.0, u[g]), g
    finally:
        _close(eng)


# ---- 6. off means off -----------------------------------------------------------------------------------------------------
def off_means_off(backend):
    """one handle, 40 simulations: a search with the solver on, then fpc_search_set_solver(0) and the same search again ==
    visits_model.Model bit for bit (and the proofs read all zero, begin having cleared them); the solver ON under rules 16
    and 15 likewise.  Condition: the solver's trees of this search are not the trees of the switch off."""
    shape, rules, sims = "8x8", SELFPLAY, 40
    R, G, _, seed = SHAPES[(shape, rules)]
    ev = evaluators.make("hash", R)
    eng = make_engine(backend, R, INV_OF[R], max_games=G, max_sims=sims)
    try:
        trees = {}
        for on, rl in ((True, rules), (False, rules), (True, 16), (True, 15)):
            eng.set_rule_bits(rl)
            eng.set_solver(on)
            b = sm.positions(R, G, seed=seed, near_end=True, rules=rl & 15)
            if on and rl == rules:
                ref = so.Model([orc.clone(x) for x in b], R, INV_OF[R], 3.0, ev, rules=rl, solver=True)
            else:
                ref = vm.Model([orc.clone(x) for x in b], R, INV_OF[R], 3.0, ev, rules=rl)
            assert ref.search(sims, 1) == 0
            res = sm.run_stepwise(eng, backend, roots_of(b, R), sims, 3.0, ev, 1)
            sm.compare(eng, res, ref.results(), ("off means off", on, rl))
            root, child = eng.search_proofs()
            if on and rl == rules:
                proofs_equal(eng, ref, "solver on")
                assert any(ref.proofs()[0])
            else:
                assert not root.any() and not child.any(), (on, rl)
            trees[(on, rl)] = _trees(ref)
        assert trees[(True, rules)] != trees[(False, rules)]
    finally:
        _close(eng)


def _trees(model):
    return [(o["root_n"], o["children"], o["w"].tolist()) for o in model.results()]


# ---- 7. refusals ----------------------------------------------------------------------------------------------------------
def refusals(backend):
    R = 8
    boards = near_end_boards("8x8", SELFPLAY)[:2]
    eng = make_engine(backend, R, INV_OF[R], max_games=2, max_sims=8)
    try:
        L, h = eng.L, eng.h
        root = np.zeros(2, np.uint8)
        assert L.fpc_search_proofs(h, 4, root.ctypes.data, None) == ESTATE               # before any search, as fpc_search_results
        assert L.fpc_search_set_solver(h, 2) == EINVAL and L.fpc_search_set_solver(h, -1) == EINVAL
        assert L.fpc_search_set_solver(None, 1) == EINVAL
        eng.set_rule_bits(SELFPLAY)
        eng.search_begin(roots_of(boards, R), 3.0)
        root, child = eng.search_proofs()                                                # never switched on: all zero
        assert not root.any() and not child.any()
        assert L.fpc_search_set_solver(h, 1) == 0                                        # after begin, before the first selection
        eng.search_select()
        assert L.fpc_search_set_solver(h, 0) == ESTATE and L.fpc_search_set_solver(h, 1) == ESTATE
        assert L.fpc_search_proofs(h, -1, root.ctypes.data, None) == EINVAL
        eng.search_results()
        assert L.fpc_search_set_solver(h, 0) == 0 and L.fpc_search_set_solver(h, 1) == 0
        assert (fpc_ffi.PROOF_UNKNOWN, fpc_ffi.PROOF_WIN, fpc_ffi.PROOF_LOSS, fpc_ffi.PROOF_DRAW) == (0, 1, 2, 3)
    finally:
        _close(eng)


# ---- 8. fpc_search_run on the internal network (GPU only: the emulator has no network) ------------------------------------
RUN = dict(R=8, hidden=128, dtype=1, layout=2, rules=TRAINING, sims=32, seed=700)
_run = {}


def run_case(policy_head):
    """everything of the case that needs no GPU, computed once: terminal_cases.legal_case's setup -- legal_head_cases.
    search_setup's integer network (its float64 reference IS the evaluator) on twelve near-end roots -- and the SOLVER
    model's search with the full or the legal-only head under rules 31"""
    if "setup" not in _run:
        import legal_head_cases as lc
        c = RUN
        boards = sm.positions(c["R"], lc.G, seed=c["seed"], near_end=True, rules=c["rules"] & 15)
        _run["setup"] = lc.search_setup(c["R"], c["hidden"], c["dtype"], boards=boards, rules=c["rules"] & 15)
    if policy_head not in _run:
        c = RUN
        m, boards, s, ev = _run["setup"]
        model = so.Model([orc.clone(b) for b in boards], c["R"], INV_OF[c["R"]], 3.0, ev, rules=c["rules"], policy_head=policy_head,
                         solver=True)
        assert model.search(c["sims"], 1) == 0
        model.check_invariants()
        assert model.counts["proven"] and model.counts["idle_proven"] + model.counts["proven_backups"] > 0, model.counts
        _run[policy_head] = model
    m, boards, s, _ = _run["setup"]
    return m, boards, s, _run[policy_head]


# ---- 5b. the self-play loop -------------------------------------------------------------------------------------------
def selfplay_loop(backend):
    """selfplay.play on near-end positions under rules 63 with the solver on: the host path (solver=True: proven_pick from
    fpc_search_proofs) and the device path (fpc_search_play) play the same games, and -- condition -- not the games of the
    host path without the rule (some proven win or draw was played against the draw)"""
    from treereuse_cases import _episode_fns
    R, G, sims, L, rules = 8, 8, 24, 3, SELFPLAY
    boards = near_end_boards("8x8", rules)
    ev = evaluators.make("hash", R)
    args = {"temperature": 1.0, "max_game_length": L, "heuristic_weight": 0.5}
    uniforms = np.random.default_rng(5).random((L, G)).tolist()
    eng = make_engine(backend, R, INV_OF[R], max_games=G, max_sims=sims)
    try:
        eng.set_rule_bits(rules)
        eng.set_solver(True)
        search_fn, _ = _episode_fns(eng, backend, ev, sims)
        host = selfplay.play(search_fn, eng, roots_of(boards, R), args, uniforms, solver=True)
        dev = selfplay.play(search_fn, eng, roots_of(boards, R), args, uniforms, device_play=True)
        plain = selfplay.play(search_fn, eng, roots_of(boards, R), args, uniforms)
    finally:
        _close(eng)
    assert [e.moves for e in host] == [e.moves for e in dev] and [e.result for e in host] == [e.result for e in dev]
    assert [e.moves for e in host] != [e.moves for e in plain]
