"""Refill (fpc_search_advance_refill) on the wavefront emulator (CPU): the product's k_tree_advance with fresh rows among
the kept ones, driven ply by ply through the step-wise C-ABI, against the plain-Python model (tests/refill_model.py), and
the Python surface above it (selfplay.play(refill=...), MCTS.continue_search, AlphaZero args["refill"]).  The cases are
those of tests/test_refill_gpu.py; everything is compared exactly."""
import pytest

import refill_cases as rc


@pytest.mark.parametrize("case", ["A", "B", "C"])
def test_engine_equals_model(case):
    rc.engine_vs_model("emul", case)


def test_all_rows_fresh_is_search_begin():
    rc.all_fresh("emul")


def test_independence():
    rc.independence("emul")


def test_errors():
    rc.errors("emul")


@pytest.mark.parametrize("reuse", [False, True])
def test_selfplay_loop(reuse):
    rc.selfplay_loop("emul", reuse)


def test_loop_positions():
    rc.loop_positions("emul")


def test_alphazero_refill():
    rc.alphazero_refill("emul")


def test_alphazero_refill_device_replay_and_play():
    rc.alphazero_refill_device("emul")
