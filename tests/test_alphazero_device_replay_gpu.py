"""AlphaZero with args["device_replay"] on the GPU: the rings hold what the host buffers hold, entry for entry, and give the
same batches bit for bit (tests/replay_cases.py)."""
import pytest

import replay_cases as rc

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("reuse", [False, True])
def test_device_replay_equals_host_replay(reuse):
    assert rc.case_alphazero_equivalence("gpu", reuse)
