"""fpc_search_play / k_play_ply on the GPU (tests/play_cases.py holds the cases)."""
import pytest

import play_cases as pc

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("case", [1, 2, 3, 4])
def test_picks_equal_the_model_and_moves_equal_todays_calls(case):
    pc.picks_and_moves("gpu", case)


def test_boundaries_of_the_draw():
    pc.boundaries("gpu")


@pytest.mark.parametrize("R,rules", [(8, 0), (14, 15)])
def test_more_than_64_children(R, rules):
    pc.many_children("gpu", R, rules)


def test_the_tree_is_untouched():
    pc.tree_untouched("gpu")


def test_dead_and_childless_games():
    pc.dead_games("gpu")


def test_errors():
    pc.errors("gpu")


@pytest.mark.parametrize("reuse", [False, True])
def test_selfplay_loop(reuse, monkeypatch):
    pc.selfplay_loop("gpu", reuse, monkeypatch)


def test_alphazero_device_play(monkeypatch):
    pc.alphazero_device_play("gpu", monkeypatch)
