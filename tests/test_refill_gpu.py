"""Refill (fpc_search_advance_refill) on the MI355X: k_tree_advance with fresh rows among the kept ones against the
plain-Python model (tests/refill_model.py), the all-fresh, independence, error, self-play-loop and AlphaZero cases of
tests/refill_cases.py, and the fused fpc_search_run after every refilling advance against the step-wise C-ABI fed by
fpc_nn_forward (k_towerc and k_towerw).  Everything is compared exactly."""
import numpy as np
import pytest

import fpc_ffi
import refill_cases as rc
import search_model as sm
from test_nn_gpu import _positions
from test_tree_reuse_gpu import _net_engine, _room

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("case", ["A", "B", "C"])
def test_engine_equals_model(case):
    rc.engine_vs_model("gpu", case)


def test_all_rows_fresh_is_search_begin():
    rc.all_fresh("gpu")


def test_independence():
    rc.independence("gpu")


def test_errors():
    rc.errors("gpu")


@pytest.mark.parametrize("reuse", [False, True])
def test_selfplay_loop(reuse):
    rc.selfplay_loop("gpu", reuse)


def test_loop_positions():
    rc.loop_positions("gpu")


def test_alphazero_refill():
    rc.alphazero_refill("gpu")


def test_alphazero_refill_device_replay_and_play():
    rc.alphazero_refill_device("gpu")


@pytest.mark.parametrize("R,hidden,kernel", [(14, 128, "k_towerc"), (8, 256, "k_towerw")])
def test_fused_equals_stepwise(R, hidden, kernel):
    """after every search_advance_refill (three rows refilled per advance) fpc_search_run == the step-wise loop fed by
    fpc_nn_forward, bit for bit"""
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
        boards = _positions(R, G + 3 * (plies - 1))
        pool = boards[G:]
        fused.search_begin([fpc_ffi.clone_board(b) for b in boards[:G]], 3.0)
        step.search_begin([fpc_ffi.clone_board(b) for b in boards[:G]], 3.0)
        n, expanded = sims, 0
        for ply in range(plies):
            fused.search_run(n)
            sm.run_steps(step, "gpu", n, ev)
            a, b = fused.search_results(), step.search_results()
            sm.same_results(a, b)
            assert int(a["sims_done"].sum()) > len(a["root_n"]) * n // 2
            if ply + 1 == plies:
                break
            picked = dict(zip(*sm.pick_rule(a)))
            refilled = [(5 * ply + 4 * j + 1) % G for j in range(3)]        # three distinct rows, other ones every ply
            src = [g if g in picked and g not in refilled else -1 for g in range(G)]
            flats = [picked[g] if s >= 0 else 0 for g, s in enumerate(src)]
            fresh = [None] * G
            for g in range(G):
                if src[g] < 0:
                    fresh[g] = pool[(3 * ply + g) % len(pool)]
            assert sum(s < 0 for s in src) >= 3 and len(set(refilled)) == 3
            ka, kb = fused.search_advance_refill(flats, src, fresh=fresh), step.search_advance_refill(flats, src, fresh=fresh)
            assert np.array_equal(ka, kb) and all(int(ka[g]) == 1 for g in refilled)
            after = fused.search_results()
            sm.same_results(after, step.search_results())
            expanded += int((after["n_children"] > 0).sum())
            n = _room(fused, ka, sims)
        assert expanded > 0
    finally:
        fused.close()
        step.close()
