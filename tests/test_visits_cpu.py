"""FPC_RULES_VISITS above the engine: mcts.budgets_for with and without the bit, MCTS's new args, selfplay.sample_move's
branch for a root none of whose children has a visit, tuples.dense_pi on such a record, and the check that keeps
tests/visits_model.py honest: with the bit clear and first-play urgency off it is terminal_model.Model."""
import numpy as np

import evaluators
import search_model as sm
import selfplay
import terminal_model as tm
import tuples
import visits_model as vm
from mcts import MCTS, budgets_for
from oracle import orc


def test_budgets_for_with_and_without_the_bit():
    kept, S, M = [1, 5, 41, 90], 40, 80
    assert budgets_for(kept, S, M, "per_game") == [40, 40, 40, 0]
    assert budgets_for(kept, S, M, "visit_target") == [40, 36, 0, 0]
    assert budgets_for(kept, S, M, "per_game", born=1) == budgets_for(kept, S, M, "per_game")
    kept0 = [0, 4, 40, 89]                                   # the same roots under the bit: N counts the simulations
    assert budgets_for(kept0, S, M, "per_game", born=0) == [40, 40, 40, 0]
    assert budgets_for(kept0, S, M, "visit_target", born=0) == [40, 36, 0, 0]
    assert budgets_for([0, 50], S, M, "per_game", born=0) == [40, 30]
    assert budgets_for(kept0, S, M, None, born=0) is None


def test_mcts_args():
    def mk(**kw):
        return MCTS(None, lambda x: x, dict({"C": 3.0, "num_searches": 1}, **kw))
    assert mk(rules="selfplay").rules == 63 and mk(rules="selfplay").born == 0
    assert mk(rules="training").rules == 31 and mk(rules="training").born == 1
    assert mk(rules=33).born == 0 and mk().born == 1
    assert mk().fpu is None and mk(fpu=None).fpu is None and mk(fpu=0.25).fpu == 0.25 and mk(fpu=0).fpu == 0.0


def test_sample_move_without_a_visit():
    flats = [11, 22, 33, 44, 55]
    zero = [0] * 5
    for u, k in ((0.0, 0), (0.19, 0), (0.2, 1), (0.5, 2), (0.999, 4)):
        assert selfplay.sample_move(flats, zero, 1.0, u) == flats[k], u
        assert selfplay.sample_move(flats, zero, 0.5, u) == flats[k], u
    assert selfplay.sample_move(flats, zero, 0, 0.7) == 11
    assert selfplay.sample_move(flats, [0, 0, 3, 0, 0], 1.0, 0.0) == 33          # a visit anywhere: the draw as it was
    assert selfplay.sample_move(flats, [0, 2, 0, 2, 0], 1.0, 0.5) == 44


def test_dense_pi_without_a_visit():
    rec = {"flat": np.array([3, 9], np.int64), "visits": np.array([0, 0], np.int64)}
    pi = tuples.dense_pi(rec, 16)
    assert pi.dtype.is_floating_point and pi.shape == (16,) and not pi.numpy().any()
    rec = {"flat": np.array([3, 9], np.int64), "visits": np.array([1, 3], np.int64)}
    assert tuples.dense_pi(rec, 16).numpy().tolist() == [0.25 if i == 3 else 0.75 if i == 9 else 0.0 for i in range(16)]


def test_model_with_the_bit_clear_is_the_terminal_model():
    R, INV, G, sims = 8, 2, 4, 40
    for rules, K in ((31, 1), (31, 3), (16, 1)):
        boards = sm.positions(R, G, seed=700, near_end=True, rules=rules & 15)
        ev = evaluators.make("hash", R)
        a = tm.Model([orc.clone(b) for b in boards], R, INV, 3.0, ev, rules=rules)
        b = vm.Model([orc.clone(b) for b in boards], R, INV, 3.0, ev, rules=rules)
        assert a.search(sims, K) == 0 and b.search(sims, K) == 0
        assert a.counts["terminals"] > 0
        ra, rb = a.results(), b.results()
        for x, y in zip(ra, rb):
            assert (x["root_n"], x["terminated"], x["sims_done"], x["children"], x["grand"]) == \
                   (y["root_n"], y["terminated"], y["sims_done"], y["children"], y["grand"])
            assert np.array_equal(x["priors"], y["priors"]) and np.array_equal(x["w"], y["w"])
        assert b.counts["unvisited"] == 0 and b.counts["fpu_decided"] == 0
        assert {k: b.counts[k] for k in a.counts} == a.counts and a.backups == b.backups
