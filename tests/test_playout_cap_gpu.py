"""Playout cap randomization (fpc_search_set_fast_rows, FPC_TUPLE_FAST, fpc_replay_batch_w) on the MI355X:
the FORCE instances of select_game under a mixed fast-row mask, k_root_targets, k_collect_tuples, k_play_ply and
k_replay_decode's weight column, driven through the C-ABI, against the plain-Python model (tests/playout_cap_model.py) and
against the engine's own unmasked searches.  The cases are those of tests/test_playout_cap_emul.py; everything is compared
exactly."""
import pytest

import playout_cap_cases as pc

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("fused", [True, False], ids=["fused", "unfused"])
@pytest.mark.parametrize("case", pc.CASES, ids=pc.IDS)
def test_engine_equals_model_under_a_mixed_mask(case, fused):
    pc.engine_vs_model("gpu", case, fused)


@pytest.mark.parametrize("case", [pc.CASES[1], pc.CASES[3], pc.CASES[7], pc.CASES[9]], ids=[pc.IDS[1], pc.IDS[3], pc.IDS[7], pc.IDS[9]])
def test_rows_are_those_of_the_unmasked_searches(case):
    pc.row_independence("gpu", case)


@pytest.mark.parametrize("case", [pc.CASES[0], pc.CASES[2], pc.CASES[8]], ids=[pc.IDS[0], pc.IDS[2], pc.IDS[8]])
def test_tuples_carry_the_flag_and_replay_decodes_the_weight(case):
    pc.tuples_and_replay("gpu", case)


def test_replay_weights_at_14x14():
    pc.replay_14x14("gpu")


@pytest.mark.parametrize("case", [pc.CASES[1], pc.CASES[6]], ids=[pc.IDS[1], pc.IDS[6]])
def test_play_draws_from_the_rows_own_counts(case):
    pc.play("gpu", case)


def test_play_with_a_proven_root():
    pc.play("gpu", pc.proven_root_case(), need_told=False)       # its condition is the proven root


def test_mask_lifetime_over_three_plies():
    pc.lifetime("gpu")


def test_errors_leave_the_state_unchanged():
    pc.errors("gpu")
