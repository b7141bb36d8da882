"""Device-side weight pack on the wavefront emulator (CPU): k_pack_conv / k_pack_fc / k_pack_misc run from the product's
source (csrc/fpc_pack.h, integer f32 -> 16-bit rounding in this build) and must reproduce weights.export_weights byte
for byte."""
import ctypes as C

import pytest

import weights_cases as wc
from fpc_testlib import make_engine


def _engine(R, dtype):
    return make_engine("emul", R, wc.INV_OF[R], max_games=1, max_sims=1, nn_dtype=dtype)


@pytest.mark.parametrize("dtype", [0, 1])
@pytest.mark.parametrize("layout", [1, 2])
def test_pack_bytes_r8(dtype, layout):
    """R = 8, hidden 64, 1 block (Np = Kp = 4608: no padding in the Linear, hidden padded 64 -> 128 in the convolutions)"""
    eng = _engine(8, dtype)
    assert wc.case_bytes(eng, 8, 1, 64, dtype, layout) > 0
    eng.close()


def test_pack_bytes_r9_padding_and_tail():
    """R = 9: A = 6480, Kp = 6656, Np = 6528 (layout 2) -- padding on both axes of the Linear, an RR tail of one position"""
    geo = wc.geometry(9, 64, 1, 2)
    assert (geo["A"], geo["Kp"], geo["Np"]) == (6480, 6656, 6528) and wc.geometry(9, 64, 1, 1)["Np"] == 6656 and 81 % 16 == 1
    eng = _engine(9, 0)
    wc.case_bytes(eng, 9, 1, 64, 0, 2)
    eng.close()


@pytest.mark.parametrize("dtype", [0, 1])
def test_pack_follows_the_f32_spec_where_the_host_sqrt_does_not(dtype, monkeypatch):
    """unshifted variances, some planted where torch's CPU sqrt is one unit off: pack == numpy op-by-op fold"""
    eng = _engine(8, dtype)
    wc.case_spec_bytes(eng, 8, 1, 64, dtype, 2, monkeypatch)
    eng.close()


def test_default_layout_is_the_exporters():
    """fc_layout 0 = weights.default_fc_layout(R), in the size and in the packed header"""
    import struct
    import weights
    eng = _engine(8, 1)
    m = wc.model(8, 1, 64)
    lay = weights.fcw_split(8) and 2 or 1
    assert eng.weights_blob_size(64, 1, 0) == eng.weights_blob_size(64, 1, lay)
    src, keep = wc.raw_src(eng, m)
    import torch
    cap = eng.weights_blob_size(64, 1, 0)
    buf = torch.zeros(cap + 64, dtype=torch.uint8)
    ptr = (buf.data_ptr() + 63) & ~63
    assert eng.L.fpc_weights_pack(eng.h, C.byref(src), 0, ptr, cap, None) == 0
    off = ptr - buf.data_ptr()
    assert struct.unpack("<4s9i24x", buf[off:off + 64].numpy().tobytes())[9] == lay
    eng.close()


def test_load_weights_device_has_no_network_here():
    eng = _engine(8, 1)
    m = wc.model(8, 1, 64)
    src, keep = wc.raw_src(eng, m)
    assert eng.L.fpc_load_weights_device(eng.h, C.byref(src), 1) == wc.EWEIGHTS
    assert b"only in the gfx950 build" in eng.L.fpc_last_error(eng.h)
    with pytest.raises(RuntimeError, match="only in the gfx950 build"):
        eng.load_weights_device(m)
    eng.close()


def test_refusals():
    eng = _engine(8, 1)
    m = wc.model(8, 1, 64)
    for name, rc in wc.einval_cases(eng, m):
        assert rc == wc.EINVAL, (name, rc)
    n = C.c_uint64()
    assert eng.L.fpc_weights_blob_size(eng.h, 64, 1, 3, C.byref(n)) == wc.EINVAL
    assert eng.L.fpc_weights_blob_size(eng.h, 64, 1, 1, None) == wc.EINVAL
    assert eng.L.fpc_load_weights_device(eng.h, None, 1) == wc.EINVAL
    assert eng.L.fpc_weights_pack_ms(eng.h, None) == wc.EINVAL
    # a shape fpc_load_weights would refuse: FPC_EWEIGHTS with its message
    m96 = wc.model(8, 1, 96)
    src, keep = wc.raw_src(eng, m96)
    assert eng.L.fpc_weights_blob_size(eng.h, 96, 1, 1, C.byref(n)) == wc.EWEIGHTS
    assert eng.L.fpc_load_weights_device(eng.h, C.byref(src), 1) == wc.EWEIGHTS
    assert b"hidden must be a multiple of 64" in eng.L.fpc_last_error(eng.h)
    # the engine still packs after every refusal
    wc.case_bytes(eng, 8, 1, 64, 1, 1)
    eng.close()


def test_pack_ms_needs_timing():
    eng = _engine(8, 1)
    ms = C.c_float()
    assert eng.L.fpc_weights_pack_ms(eng.h, C.byref(ms)) == -9            # FPC_ESTATE: nothing has been timed
    eng.set_timing(True)
    wc.case_bytes(eng, 8, 1, 64, 1, 2)
    assert eng.weights_pack_ms() >= 0.0
    eng.close()
