"""AlphaZero with args["device_replay"] on the wavefront emulator: the rings hold what the host buffers hold, entry for entry, and give the
same batches bit for bit (tests/replay_cases.py)."""
import pytest

import replay_cases as rc


@pytest.mark.parametrize("reuse", [False, True])
def test_device_replay_equals_host_replay(reuse):
    assert rc.case_alphazero_equivalence("emul", reuse)
