"""Subtree reuse (fpc_search_advance) on the MI355X: k_tree_advance and the tree kernels against the plain-Python model
with persistent trees (tests/search_model.py) at the full case sizes, the structural, dropping, budget and error
checks of tests/treereuse_cases.py, the fused fpc_search_run after every advance against the step-wise C-ABI fed by
fpc_nn_forward (k_towerc and k_towerw), the legal-only head through the plies, and the self-play loop.  Everything is
compared exactly."""
import numpy as np
import pytest

import fpc_ffi
import search_model as sm
import treereuse_cases as tc
from fpc_testlib import make_engine
from test_nn_gpu import INV_OF, _model, _positions

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("case", [1, 2, 3])
def test_engine_equals_model(case):
    tc.engine_vs_model("gpu", case)


def test_leaf_parallel_after_games_moved():
    """K = 2 through three plies with game 0 dropped at the first advance: every game continues in another region"""
    tc.engine_vs_model("gpu", 2, G=9, drop_first=True)


def test_structure_right_after_the_advance():
    tc.structure("gpu")


def test_dropping_games():
    tc.dropping("gpu")


def test_budget():
    tc.budget("gpu")


def test_errors():
    tc.errors("gpu")


def test_selfplay_loop():
    tc.selfplay_loop("gpu")


def _net_engine(R, hidden, dtype, G, sims, rules=0, legal=False):
    import weights
    eng = make_engine("gpu", R, INV_OF[R], max_games=G, max_sims=2 * sims, nn_dtype=dtype)
    eng.load_weights(weights.export_weights(_model(R, 2, hidden, seed=5), dtype))
    eng.set_rules(rules)
    eng.set_policy_mode(legal)
    return eng


def _room(eng, kept, sims):
    return min(sims, eng.max_sims - (int(kept.max()) - 1))


@pytest.mark.parametrize("R,hidden,kernel", [(14, 128, "k_towerc"), (8, 256, "k_towerw")])
def test_fused_equals_stepwise(R, hidden, kernel):
    """after every advance fpc_search_run == the step-wise loop fed by fpc_nn_forward, bit for bit"""
    import torch
    G, plies, sims = 12, 3, 20
    fused, step = _net_engine(R, hidden, 1, G, sims), _net_engine(R, hidden, 1, G, sims)

    def ev(enc):
        n = enc.shape[0]
        x = torch.from_numpy(np.ascontiguousarray(enc)).cuda()
        lg = torch.empty(n, step.A, device="cuda")
        va = torch.empty(n, device="cuda")
        torch.cuda.synchronize()
        step.nn_forward(x.data_ptr(), n, lg.data_ptr(), va.data_ptr())
        return lg.cpu().numpy(), va.cpu().numpy()

    try:
        assert fused.L.fpc_nn_kernel(fused.h).decode() == kernel
        boards = _positions(R, G)
        fused.search_begin([fpc_ffi.clone_board(b) for b in boards], 3.0)
        step.search_begin([fpc_ffi.clone_board(b) for b in boards], 3.0)
        n, stats, expanded = sims, {"visited": 0, "unvisited": 0}, 0
        for ply in range(plies):
            fused.search_run(n)
            sm.run_steps(step, "gpu", n, ev)
            a, b = fused.search_results(), step.search_results()
            sm.same_results(a, b)
            assert int(a["sims_done"].sum()) > len(a["root_n"]) * n // 2
            if ply + 1 == plies:
                break
            src, flats = sm.pick_rule(a, stats)
            ka, kb = fused.search_advance(flats, src), step.search_advance(flats, src)
            assert np.array_equal(ka, kb)
            after = fused.search_results()
            sm.same_results(after, step.search_results())
            expanded += int((after["n_children"] > 0).sum())
            n = _room(fused, ka, sims)
        assert stats["visited"] > 0 and stats["unvisited"] > 0 and expanded > 0, (stats, expanded)
    finally:
        fused.close()
        step.close()


def test_legal_head_through_the_plies():
    """FPC_POLICY_LEGAL is not bit-comparable with the step-wise full head; what holds exactly is that under
    FPC_RULES_FIXED a game's fused search does not depend on the batch: with a strict subsequence of the games advanced,
    every survivor has the search it has when all are advanced, through the plies (k_towerw, 8x8, hidden 256)"""
    R, hidden, G, plies, sims = 8, 256, 12, 3, 20
    sub = [0, 3, 4, 7, 10, 11]
    out, used = [], []                        # simulations per ply: what max_sims leaves room for when all games go on
    for only in (None, sub):
        eng = _net_engine(R, hidden, 1, G, sims, rules=fpc_ffi.RULES_FIXED, legal=True)
        try:
            assert eng.L.fpc_nn_kernel(eng.h).decode() == "k_towerw"
            eng.search_begin(_positions(R, G), 3.0)
            eng.search_run(sims)
            res, runs = eng.search_results(), []
            src, flats = sm.pick_rule(res)
            assert src == list(range(G))
            for _ply in range(1, plies):
                if only is not None:
                    src, flats, only = [src[i] for i in only], [flats[i] for i in only], None
                kept = eng.search_advance(flats, src)
                if len(used) < _ply:
                    used.append(_room(eng, kept, sims))
                eng.search_run(used[_ply - 1])
                res = eng.search_results()
                assert (res["root_n"] == kept + res["sims_done"]).all() and int(res["n_children"].min()) > 0
                runs.append(res)
                src = list(range(len(kept)))
                flats = [int(res["flat"][g, int(np.argmax(res["visits"][g, :res["n_children"][g]]))]) for g in src]
            out.append(runs)
        finally:
            eng.close()
    for a, b in zip(*out):
        sm.same_results(a, b, sub, None)


def test_alphazero_reuse_tree():
    tc.alphazero_reuse_tree("gpu")
