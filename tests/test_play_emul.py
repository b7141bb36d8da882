"""fpc_search_play / k_play_ply on the wavefront emulator: the product's kernel source and host code on the CPU
(tests/play_cases.py holds the cases; tests/test_play_gpu.py runs them on the GPU at their full sizes)."""
import pytest

import play_cases as pc

EMUL_G = {1: 4, 2: 2, 3: 4, 4: 4}


@pytest.mark.parametrize("case", [1, 2, 3, 4])
def test_picks_equal_the_model_and_moves_equal_todays_calls(case):
    pc.picks_and_moves("emul", case, EMUL_G[case])


def test_boundaries_of_the_draw():
    pc.boundaries("emul", 4)


@pytest.mark.parametrize("R,rules", [(8, 0), (14, 15)])
def test_more_than_64_children(R, rules):
    pc.many_children("emul", R, rules)


def test_the_tree_is_untouched():
    pc.tree_untouched("emul", 4)


def test_dead_and_childless_games():
    pc.dead_games("emul", 4)


def test_errors():
    pc.errors("emul")


@pytest.mark.parametrize("reuse", [False, True])
def test_selfplay_loop(reuse, monkeypatch):
    pc.selfplay_loop("emul", reuse, monkeypatch, G=3)


def test_alphazero_device_play(monkeypatch):
    pc.alphazero_device_play("emul", monkeypatch)
