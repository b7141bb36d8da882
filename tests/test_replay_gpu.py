"""Device-resident replay store and batched decode (fpc_replay_*) on the GPU (product library): tests/replay_cases.py."""
import pytest

import fpc_ffi
import replay_cases as rc

pytestmark = pytest.mark.gpu


def test_reference_training_batch_decodes_to_the_recorded_tensors_and_losses():
    assert rc.case_golden("gpu") == 16


@pytest.mark.parametrize("R,rules", [(8, 0), (14, 0), (14, fpc_ffi.RULES_FIXED)])
def test_decode_equals_the_per_sample_path_bit_for_bit(R, rules):
    assert rc.case_matches_per_sample_path("gpu", R, rules) >= 83


def test_ring_semantics_are_replay_buffers():
    assert rc.case_ring_semantics("gpu", gathered=True) == 2


def test_errors_leave_the_rings_alone():
    assert rc.case_errors("gpu")


def test_device_replay_buffer_samples_what_replay_buffer_samples():
    assert rc.case_device_buffer_sample("gpu")
