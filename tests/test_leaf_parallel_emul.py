"""Leaf-parallel search (fpc_search_set_leaves) on the wavefront emulator (CPU): the product's tree kernels, driven
through the step-wise C-ABI with K leaves per game per step, against the plain-Python model of the semantics
(tests/search_model.py), bit for bit: root N, children, visits, f32 priors, f64 value sums, sims_done, second-level
visits and the root state, piece-list order included."""
import numpy as np
import pytest

import evaluators
import fpc_ffi
import search_model as sm
from engine_cases import _compare_search
from fpc_testlib import make_engine, roots_of
from oracle import orc

INV_OF = {8: 2, 14: 3}


def _engine_vs_model(R, boards_o, sims, K, kind="hash", rules=0, noise=False, vl=1.0, fused=True, seed=0):
    INV = INV_OF[R]
    G = len(boards_o)
    ev = evaluators.make(kind, R)
    gamma = None
    if noise:
        gamma = np.random.default_rng(seed).standard_gamma(0.3, size=(G, fpc_ffi.MAX_MOVES)).astype(np.float32)
    rc, model, counts = sm.search([orc.clone(b) for b in boards_o], R, INV, sims, 3.0, ev, K, vl=vl, rules=rules,
                                  noise=gamma, noise_eps=0.25)
    kmax = max(sm.schedule(sims, K))
    eng = make_engine("emul", R, INV, max_games=G * kmax, max_sims=sims)
    try:
        eng.set_rules(rules)
        eng.set_root_noise(gamma, 0.25)
        roots = roots_of(boards_o, R)
        if rc == -3:
            with pytest.raises(RuntimeError, match="policy mass"):
                sm.run_stepwise(eng, "emul", roots, sims, 3.0, ev, K, vl=vl, fused=fused)
            return "policy-error", counts
        assert rc == 0
        res = sm.run_stepwise(eng, "emul", roots, sims, 3.0, ev, K, vl=vl, fused=fused)
        sm.compare(eng, res, model, (R, K, kind, rules, sims))
        assert all(int(x) <= sims for x in res["sims_done"])
    finally:
        eng.close()
    return "ok", counts


@pytest.mark.parametrize("R,K,sims,kind", [
    (8, 2, 21, "hash"), (8, 3, 20, "ramp"), (8, 4, 18, "hashinf1"),
    (14, 2, 13, "hash"), (14, 3, 11, "ramp"), (14, 4, 10, "hash"),
])
def test_engine_equals_model_midgame(R, K, sims, kind):
    boards = sm.positions(R, 6 if R == 8 else 4, seed=100 + 7 * K + R)
    assert sims % K != 0 or K == 4          # most cases end with a partial step
    status, _ = _engine_vs_model(R, boards, sims, K, kind=kind, fused=(K != 3))
    assert status == "ok"


@pytest.mark.parametrize("R,K", [(8, 2), (8, 3), (14, 2)])
def test_engine_equals_model_near_end(R, K):
    """positions a few plies before the end of a game: terminal leaves during leaf-parallel steps"""
    boards = sm.positions(R, 6, seed=5 + K, near_end=True)
    status, counts = _engine_vs_model(R, boards, 17, K, kind="hash")
    assert status == "ok"


@pytest.mark.parametrize("R", [8, 14])
def test_fixed_rules_with_root_noise(R):
    boards = sm.positions(R, 4, seed=41 + R, rules=15)
    status, _ = _engine_vs_model(R, boards, 14, 3, kind="hash", rules=15, noise=True, vl=0.5)
    assert status == "ok"


def test_hashinf_both_refuse():
    """every legal logit -inf somewhere: the model and the engine both end the search with the policy error"""
    statuses = [_engine_vs_model(8, sm.positions(8, 4, seed=seed), 12, 2, kind="hashinf")[0] for seed in range(3, 9)]
    assert "policy-error" in statuses, statuses


def test_collisions_and_terminals_met():
    """the cases of this file meet both kinds of dead row: a collision and a terminal leaf inside a leaf-parallel step"""
    status, counts = _engine_vs_model(8, sm.positions(8, 6, seed=7, near_end=True), 17, 2, kind="hash")
    assert status == "ok" and counts["collisions"] > 0 and counts["terminals"] > 0, counts


@pytest.mark.parametrize("sched,fused", [((1, 2, 2, 2, 2, 2), True), ((1, 2, 2, 2, 2, 2), False), ((1, 1, 3, 3, 1, 2, 4), True),
                                         ((2, 1, 1, 3, 2, 1), False)])
def test_leaves_changed_during_search(sched, fused):
    """set_leaves between the steps of a running search, including 1 -> K while a one-leaf selection is pending
    (that selection holds no pending visits: it is expanded as one leaf per game, the next one is leaf-parallel)"""
    boards = sm.positions(8, 6, seed=61)
    status, _ = _engine_vs_model(8, boards, sum(sched), list(sched), kind="hash", fused=fused)
    assert status == "ok"


def test_set_leaves_one_equals_oracle():
    R, INV = 8, 2
    boards = sm.positions(R, 5, seed=77)
    ev = evaluators.make("hash", R)
    rc, oref = orc.search([orc.clone(b) for b in boards], R, INV, 12, 3.0, ev)
    assert rc == 0
    eng = make_engine("emul", R, INV, max_games=10, max_sims=12)
    try:
        eng.set_leaves(2)
        eng.set_leaves(1)
        res = sm.run_stepwise(eng, "emul", roots_of(boards, R), 12, 3.0, ev, 1)
        _compare_search(res, oref, "leaves=1")
    finally:
        eng.close()


def test_argument_validation():
    R, INV = 8, 2
    eng = make_engine("emul", R, INV, max_games=8, max_sims=8)
    try:
        for bad in ((0, 1.0), (9, 1.0), (2, float("nan")), (2, -0.5), (2, float("inf"))):
            with pytest.raises(RuntimeError):
                eng.set_leaves(*bad)
        eng.set_leaves(fpc_ffi.MAX_LEAVES, 0.0)
        boards = roots_of(sm.positions(R, 2, seed=1), R)
        with pytest.raises(RuntimeError, match="max_games"):      # 8 leaves x 2 games > 8 rows
            eng.search_begin(boards, 3.0)
        eng.set_leaves(4)
        eng.search_begin(boards, 3.0)                              # 4 x 2 = 8 rows: fits
        with pytest.raises(RuntimeError, match="max_games"):      # during the search: 5 x 2 > 8
            eng.set_leaves(5)
        eng.set_leaves(3)
        eng.search_results()
        # after the results the setting may change freely, but every call that selects checks that the rows fit
        eng.set_leaves(8)
        with pytest.raises(RuntimeError, match="max_games"):
            eng.search_select()
        with pytest.raises(RuntimeError, match="max_games"):
            eng.search_run(2)
        eng.set_leaves(2)
        eng.search_select()
    finally:
        eng.close()


def test_mcts_dropin_external_evaluator():
    """mcts.MCTS with leaves_per_step = 2 and an external evaluator reproduces the model through the drop-in surface"""
    import torch

    import dropin_cases
    from four_player_chess_board import FourPlayerChess
    from mcts import MCTS
    R, INV = 8, 2
    az = dropin_cases.setup("emul", R)
    boards = sm.positions(R, 5, seed=19)
    ev = evaluators.make("hash", R)
    sims = 9
    rc, model, _ = sm.search([orc.clone(b) for b in boards], R, INV, sims, 3.0, ev, 2)
    assert rc == 0

    rows = []

    class Ev:
        device = "cpu"

        def __call__(self, enc):
            rows.append(enc.shape[0])
            lg, v = ev(enc.numpy())
            return torch.from_numpy(np.ascontiguousarray(lg)), torch.from_numpy(np.ascontiguousarray(v)).view(-1, 1)

    games = [FourPlayerChess._wrap(fb) for fb in roots_of(boards, R)]
    mc = MCTS(FourPlayerChess, Ev(), {"num_searches": sims, "C": 3.0, "leaves_per_step": 2})
    roots = mc.search(games)
    for g, (root, o) in enumerate(zip(roots, model)):
        assert root.GetVisitCount() == o["root_n"], g
        got = [[c.GetMoveMade().GetFlatIndex(), c.GetVisitCount()] for c in root.GetChildren()]
        assert got == o["children"], g
    assert rows == [2 * len(boards)] * 4 + [len(boards)]      # [k*G, 24, R, R]: four steps of 2 leaves, then 1
    # the handle is process-wide: the next search with the default setting is one leaf per game again
    MCTS(FourPlayerChess, Ev(), {"num_searches": 3, "C": 3.0}).search(games[:2])
