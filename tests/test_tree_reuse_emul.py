"""Subtree reuse (fpc_search_advance) on the wavefront emulator (CPU): the product's k_tree_advance and tree kernels,
driven ply by ply through the step-wise C-ABI, against the plain-Python model with persistent trees
(tests/search_model.py), bit for bit.  The cases are those of tests/test_tree_reuse_gpu.py with fewer games."""
import pytest

import treereuse_cases as tc


@pytest.mark.parametrize("case,G", [(1, 4), (2, 4), (3, 2)])
def test_engine_equals_model(case, G):
    tc.engine_vs_model("emul", case, G=G)


def test_leaf_parallel_after_games_moved():
    """K = 2 through three plies with game 0 dropped at the first advance: every game continues in another region"""
    tc.engine_vs_model("emul", 2, G=5, drop_first=True)


def test_structure_right_after_the_advance():
    tc.structure("emul")


def test_dropping_games():
    tc.dropping("emul")


def test_budget():
    tc.budget("emul")


def test_errors():
    tc.errors("emul")


def test_selfplay_loop():
    tc.selfplay_loop("emul")


def test_alphazero_reuse_tree():
    tc.alphazero_reuse_tree("emul")
