"""The int8 policy Linear's device pack on the wavefront emulator (CPU): k_fc_rowmax + k_pack_fc8 run from the product's
source (csrc/fpc_pack.h) and must reproduce weights.export_weights(..., fc_weights="int8") byte for byte; the refusals of
fpc_set_fc_weight_type and of the three pack entry points leave a 16-bit pack as it was."""
import copy
import ctypes as C

import pytest
import torch

import weights
import weights_cases as wc
from fpc_testlib import make_engine


def _engine(R, dtype=1):
    return make_engine("emul", R, wc.INV_OF[R], max_games=1, max_sims=1, nn_dtype=dtype)


@pytest.mark.parametrize("R", [8, 9])
def test_int8_pack_bytes(R):
    """R = 8: no padding in the Linear; R = 9: A = 6480, Kp = 6656, Np = 6528 -- padding on both axes, an RR tail of one"""
    m = wc.model(R, 1, 64)
    ref = weights.export_weights(m, 1, 2, fc_weights="int8")
    eng = _engine(R)
    eng.set_fc_weight_type("int8")
    assert eng.weights_blob_size(64, 1, 2) == len(ref)
    assert eng.weights_blob_size(64, 1, 0) == len(ref)                 # layout 0 resolves to 2 on these boards
    got = eng.weights_pack(m, 2)
    wc.assert_same_blob(got, ref, "int8 pack, R=%d" % R)
    assert eng.weights_pack(m, None, fc_weights="int8") == ref
    # back to 16 bit on the same engine: the parent's bytes
    eng.set_fc_weight_type("w16")
    wc.case_bytes(eng, R, 1, 64, 1, 2)
    eng.close()


def test_int8_refusals_leave_the_16_bit_pack_as_it_was():
    m = wc.model(8, 1, 64)
    n = C.c_uint64()
    eng = _engine(8, 1)
    L = eng.L
    assert L.fpc_set_fc_weight_type(eng.h, 2) == wc.EINVAL
    assert L.fpc_set_fc_weight_type(eng.h, -1) == wc.EINVAL
    assert L.fpc_set_fc_weight_type(None, 1) == wc.EINVAL
    with pytest.raises(ValueError):
        eng.set_fc_weight_type("fp8")
    wc.case_bytes(eng, 8, 1, 64, 1, 2)                                 # the refused types changed nothing
    # fc_layout 1 with int8
    eng.set_fc_weight_type("int8")
    src, keep = wc.raw_src(eng, m)
    cap = eng.weights_blob_size(64, 1, 2)
    buf = torch.zeros(cap + 64, dtype=torch.uint8)
    ptr = (buf.data_ptr() + 63) & ~63
    assert L.fpc_weights_blob_size(eng.h, 64, 1, 1, C.byref(n)) == wc.EWEIGHTS
    assert b"fc_layout 1" in L.fpc_last_error(eng.h) and b"int8" in L.fpc_last_error(eng.h)
    assert L.fpc_weights_pack(eng.h, C.byref(src), 1, ptr, cap, C.byref(n)) == wc.EWEIGHTS
    assert L.fpc_load_weights_device(eng.h, C.byref(src), 1) == wc.EWEIGHTS
    assert b"fc_layout 1" in L.fpc_last_error(eng.h)
    assert not buf.any(), "a refused pack wrote into the blob"
    assert L.fpc_weights_blob_size(eng.h, 64, 1, 3, C.byref(n)) == wc.EINVAL       # still the argument error it was
    eng.set_fc_weight_type("w16")
    wc.case_bytes(eng, 8, 1, 64, 1, 1)
    # a planted NaN / infinity: FPC_EWEIGHTS, the message names the policy Linear, nothing written
    for bad in (float("nan"), float("inf")):
        m2 = copy.deepcopy(m)
        with torch.no_grad():
            m2.policyHead[4].weight[4000, 4607] = bad
        src2, keep2 = wc.raw_src(eng, m2)
        eng.set_fc_weight_type("int8")
        assert L.fpc_weights_pack(eng.h, C.byref(src2), 2, ptr, cap, C.byref(n)) == wc.EWEIGHTS
        assert b"policy Linear" in L.fpc_last_error(eng.h) and b"non-finite" in L.fpc_last_error(eng.h)
        assert not buf.any(), "a refused pack wrote into the blob"
        with pytest.raises(RuntimeError, match="policy Linear"):
            eng.weights_pack(m2, 2)
        eng.set_fc_weight_type("w16")
        wc.case_bytes(eng, 8, 1, 64, 1, 2)
        del keep2
    wc.case_bytes(eng, 8, 1, 64, 1, 2)
    eng.close()
    # a bf16 engine
    eng = _engine(8, 0)
    eng.set_fc_weight_type("int8")
    src, keep = wc.raw_src(eng, m)
    assert eng.L.fpc_weights_blob_size(eng.h, 64, 1, 2, C.byref(n)) == wc.EWEIGHTS
    assert b"bf16" in eng.L.fpc_last_error(eng.h)
    assert eng.L.fpc_weights_pack(eng.h, C.byref(src), 2, ptr, cap, C.byref(n)) == wc.EWEIGHTS
    assert eng.L.fpc_load_weights_device(eng.h, C.byref(src), 0) == wc.EWEIGHTS
    assert not buf.any()
    eng.set_fc_weight_type("w16")
    wc.case_bytes(eng, 8, 1, 64, 0, 2)
    eng.close()


def test_fc_kernel_name_is_empty_without_a_network():
    eng = _engine(8, 1)
    assert eng.nn_fc_kernel() == ""
    eng.close()
