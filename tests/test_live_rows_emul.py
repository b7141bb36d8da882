"""Live-row numbering (fpc_search_set_live_rows) on the wavefront emulator (CPU): k_live_rows, the compact encodings of
finish_select, k_softmax_partials over n_live rows and the expansion's inv[row] indirection -- the product's kernel source --
driven through the step entry points, the switch on against the switch off and against the plain-Python model
(tests/terminal_model.py), and the Python surface above it (Engine.set_live_rows, MCTS args["live_rows"]).  The cases are
those of tests/test_live_rows_gpu.py's first half (tests/live_rows_cases.py); everything is compared exactly."""
import pytest

import live_rows_cases as lr


@pytest.mark.parametrize("name", list(lr.PATTERNS))
def test_layout(name):
    lr.layout("emul", name)


@pytest.mark.parametrize("rules", [0, 31], ids=["strict", "training"])
def test_two_leaves_near_end_on_equals_off_equals_model(rules):
    lr.near_end("emul", rules)


def test_reuse_with_refill():
    lr.reuse("emul")


def test_state_rules():
    lr.state_rules("emul")


def test_mcts_search_with_live_rows_over_an_external_evaluator():
    lr.mcts_external("emul")
