"""The opt-in int8 policy Linear on the CPU: weights.quantize_fc against an independent numpy restatement
of its spec, the version-4 blob's layout against the pair-order formula, the default export against the bytes of the
commit before the option existed, and the proof that the cases of tests/test_fc8_gpu.py can fail."""
import hashlib

import numpy as np
import pytest
import torch

import fc8_cases as f8
import tower_probe as tp
import weights
import weights_cases as wc


# ---------------------------------------------------------------------------------------------------------------------
# 1. quantize_fc against the spec
# ---------------------------------------------------------------------------------------------------------------------
def _spec_matrix():
    rng = np.random.default_rng(5)
    w = (rng.standard_normal((24, 64)) * 0.3).astype(np.float32)
    w[1] = 0.0                                                      # a zero row
    w[2] = (rng.standard_normal(64) * 2.0 ** -110).astype(np.float32)   # below the floor 127 * 2^-100: s = 1, q = 0
    w[3] = np.float32(127.0 * 2.0 ** -100) * rng.uniform(-1, 1, 64).astype(np.float32)
    w[3, 0] = np.float32(127.0 * 2.0 ** -100)                       # exactly at the floor: quantised like any other row
    # exact ties: max 127 * 2^-3 -> s = 2^-3; w = (k + 0.5) * s rounds to the even neighbour
    w[4] = 0.0
    w[4, 0] = 127.0 / 8.0
    w[4, 1:9] = (np.array([0, 1, 2, 3, -1, -2, -3, 125]) + 0.5) / 8.0
    w[4, 9] = -126.5 / 8.0
    # rows whose maximum is negative
    w[5] = -np.abs(w[5])
    w[6] = np.abs(w[6])
    w[6, 7] = -3.0
    w[7] = 0.0
    w[7, 5] = -1e30                                                 # one huge negative entry, the rest zero
    return w


def test_quantize_fc_is_the_spec_bit_for_bit():
    w = _spec_matrix()
    q, s = weights.quantize_fc(torch.from_numpy(w))
    qs, ss = f8.quantize_spec(w)
    assert q.dtype == torch.int8 and s.dtype == torch.float32
    assert np.array_equal(q.numpy(), qs)
    assert np.array_equal(s.numpy().view(np.uint32), ss.view(np.uint32))
    assert int(q.min()) >= -127 and int(q.max()) <= 127
    # the rows the matrix was built for
    assert not q[1].any() and s[1] == 1.0 and not q[2].any() and s[2] == 1.0
    assert s[3] != 1.0 and int(q[3, 0]) == 127
    assert s[4] == 0.125 and q[4, :10].tolist() == [127, 0, 2, 2, 4, 0, -2, -2, 126, -126]
    assert int(q[5].min()) == -127 and int(q[5].max()) <= 0
    assert int(q[6, 7]) == -127 and int(q[7, 5]) == -127
    # a larger random matrix, and one of subnormal magnitudes around the floor
    rng = np.random.default_rng(6)
    for scale in (1.0, 1e-3, 2.0 ** -95, 2.0 ** -99):
        w = (rng.standard_normal((96, 200)) * scale).astype(np.float32)
        q, s = weights.quantize_fc(torch.from_numpy(w))
        qs, ss = f8.quantize_spec(w)
        assert np.array_equal(q.numpy(), qs) and np.array_equal(s.numpy().view(np.uint32), ss.view(np.uint32)), scale


@pytest.mark.parametrize("bad", [float("nan"), float("inf"), -float("inf")])
def test_quantize_fc_refuses_non_finite_weights(bad):
    w = _spec_matrix()
    w[9, 3] = bad
    with pytest.raises(ValueError, match="policy Linear"):
        weights.quantize_fc(torch.from_numpy(w))
    m = wc.model(8, 1, 64)
    import copy
    m2 = copy.deepcopy(m)
    with torch.no_grad():
        m2.policyHead[4].weight[11, 17] = bad
    with pytest.raises(ValueError, match="policy Linear"):
        weights.export_weights(m2, 1, 2, fc_weights="int8")


# ---------------------------------------------------------------------------------------------------------------------
# 2. export layout
# ---------------------------------------------------------------------------------------------------------------------
PARENT_SHA256_R8_H64_B1_FP16_LAYOUT2 = "afa0075be42b7c199ff83069417aae1b872fb7fa65c07bea33e7e8b6a8dc68e9"


def test_default_export_is_the_parents_bytes():
    """export_weights without the new argument: the sha256 of weights_cases.model(8, 1, 64) exported as fp16, layout 2,
    recorded from the commit before fc_weights existed"""
    m = wc.model(8, 1, 64)
    blob = weights.export_weights(m, 1, 2)
    assert len(blob) == 43160132
    assert hashlib.sha256(blob).hexdigest() == PARENT_SHA256_R8_H64_B1_FP16_LAYOUT2
    assert weights.export_weights(m, 1, 2, fc_weights="w16") == blob
    assert f8.header_of(blob)[1] == 3 and blob[40:64] == b"\0" * 24


@pytest.mark.parametrize("R", [8, 9])
def test_int8_export_layout(R):
    """the version-4 policy-fc section decoded by the pair-order formula == quantize_fc of the permuted, padded weight;
    R = 8: no padding; R = 9: A = 6480, Kp = 6656, Np = 6528, padding on both axes"""
    m = wc.model(R, 1, 64)
    blob = weights.export_weights(m, 1, fc_weights="int8")
    w16 = weights.export_weights(m, 1)
    A, Np, Kp = f8.geometry(R)
    if R == 9:
        assert (A, Np, Kp) == (6480, 6528, 6656)
    else:
        assert A == Np == Kp == 4608
    assert f8.header_of(blob) == (b"FPCW", 4, R, 64, 1, 1, 8 * R + 8, Np, Kp, 2, 1) and blob[44:64] == b"\0" * 20
    off = f8.fc_offset(64, 1)
    assert blob[64:off] == w16[64:off]                              # the convolutions are the 16-bit export's
    fw = m.policyHead[4].weight.detach()
    q, s = weights.quantize_fc(fw)
    want = np.zeros((Np, Kp), np.int8)
    want[:A, :A] = tp.engine_order(q.numpy(), R)
    got = f8.decode_pairs(blob[off:off + Np * Kp], Np, Kp)
    assert np.array_equal(got, want)
    assert int(got.min()) >= -127
    sc = np.frombuffer(blob, np.float32, Np, off + Np * Kp)
    assert np.array_equal(sc[:A].view(np.uint32), s.numpy().view(np.uint32)) and (sc[A:] == 1.0).all()
    # bias, value Linear and value bias: the 16-bit export's sections, moved
    tail16 = w16[off + 2 * Np * Kp:]
    assert blob[off + Np * Kp + 4 * Np:] == tail16
    assert len(blob) == len(w16) - Np * Kp + 4 * Np
    # the fixture's rows 5..36 are scaled by 1e-36, below the floor of 127 * 2^-100: zeros under a scale of 1; every
    # other row reaches +-127
    assert not got[5:37].any() and (sc[5:37] == 1.0).all()
    assert (np.abs(got[37:A, :A]).max(axis=1) == 127).all()


def test_int8_export_refuses_bf16_and_layout_1():
    m = wc.model(8, 1, 64)
    with pytest.raises(ValueError, match="fp16"):
        weights.export_weights(m, 0, 2, fc_weights="int8")
    with pytest.raises(ValueError, match="fc_layout 2"):
        weights.export_weights(m, 1, 1, fc_weights="int8")
    with pytest.raises(ValueError, match="fc_weights"):
        weights.export_weights(m, 1, 2, fc_weights="fp8")


def test_tail8_is_an_export():
    """Tail8 + splice8 (numpy alone) == export_weights(..., fc_weights="int8") of the same network, every byte: q with a
    +-127 in every row and power-of-two scales quantises back to itself"""
    R = 8
    A = f8.geometry(R)[0]
    rng = np.random.default_rng(3)
    q = rng.integers(-127, 128, size=(A, A), dtype=np.int8)
    q[np.arange(A), rng.integers(0, A, size=A)] = rng.choice(np.array([-127, 127], np.int8), size=A)
    scale = np.exp2(-(np.arange(A) % 4)).astype(np.float32)
    bias = rng.integers(-5, 6, size=A)
    p = tp.prepare(tp.linear_case(R, 1, 37))
    m = p["net"]
    import net
    full = net.ResNet(tp.Spec(R), 3, 128, "cpu").eval()
    full.load_state_dict({k: v for k, v in m.state_dict().items() if "policyHead.4" not in k and "valueHead.4" not in k}, strict=False)
    for (c, b), (c2, b2) in zip(tp._convs(m), tp._convs(full)):
        b2.eps = b.eps
    vw, vb = tp.value_vector(R)
    with torch.no_grad():
        full.policyHead[4].weight.copy_(torch.from_numpy(q.astype(np.float32) * scale[:, None]))
        full.policyHead[4].bias.copy_(torch.from_numpy(bias.astype(np.float32)))
        full.valueHead[4].weight.copy_(torch.from_numpy(vw).view(1, -1))
        full.valueHead[4].bias.fill_(float(vb))
    want = weights.export_weights(full, 1, 2, fc_weights="int8")
    got = f8.splice8(m, f8.Tail8(R, q, scale, bias))
    assert got == want


# ---------------------------------------------------------------------------------------------------------------------
# 5. the cases can fail
# ---------------------------------------------------------------------------------------------------------------------
def test_single_faults_of_the_int8_linear_change_a_logit():
    """the dense case of test_fc8_gpu.py (8x8, 256 rows, q over the whole int8 range, scales 2^-(n mod 4)): each single
    fault of k_fcw8's own decomposition makes check_exact raise; no fragment product of the case is dead"""
    R = 8
    p = tp.prepare(tp.linear_case(R, 1, 256))
    q, scale, bias = f8.dense_case(R)
    policy = p["ref"]["policy"]
    f8.conditions8(policy.reshape(policy.shape[0], -1), q, scale, bias)
    want = f8.expected8(policy, q, scale, bias)
    tp.check_exact(want.astype(np.float32), want, "the reference against itself")
    for name in f8.MUTATIONS8:
        with pytest.raises(AssertionError, match="elements differ"):
            tp.check_exact(f8.mutated8(policy, R, q, scale, bias, name).astype(np.float32), want, name)
    dead, total = f8.dead_fragment_products8(policy, R, q)
    assert dead == 0 and total == 16 * (4608 // 16) * (4608 // 32), (dead, total)


# ---------------------------------------------------------------------------------------------------------------------
# the Python surface
# ---------------------------------------------------------------------------------------------------------------------
def test_mcts_fc_weights_argument():
    """args["fc_weights"]: "w16" by default, "int8" opt-in and only with fp16 operands; anything else is refused"""
    from mcts import MCTS
    m = wc.model(8, 1, 64)
    assert MCTS(None, m, {"nn_dtype": 1}).fc_weights == "w16"
    assert MCTS(None, m, {"nn_dtype": 1, "fc_weights": "int8"}).fc_weights == "int8"
    with pytest.raises(ValueError, match="fp16"):
        MCTS(None, m, {"nn_dtype": 0, "fc_weights": "int8"})
    with pytest.raises(ValueError, match="fc_weights"):
        MCTS(None, m, {"nn_dtype": 1, "fc_weights": "fp8"})


def test_mcts_syncs_int8_weights_through_both_paths():
    """sync_weights hands the option to the host export and to the device pack"""
    from mcts import MCTS
    m = wc.model(8, 1, 64)

    class Eng:
        host_memory, device, calls = True, 0, []

        def load_weights(self, blob):
            self.calls.append(("host", f8.header_of(blob)[1], f8.header_of(blob)[10]))

        def load_weights_device(self, model, fc_layout=None, fc_weights=None):
            self.calls.append(("device", fc_weights))

    e = Eng()
    MCTS(None, m, {"nn_dtype": 1, "fc_weights": "int8"}).sync_weights(e)
    MCTS(None, m, {"nn_dtype": 1}).sync_weights(Eng())
    assert e.calls[0] == ("host", 4, 1) and e.calls[1] == ("host", 3, 0)
