"""The residual tower, the policy conv and the value conv ELEMENT BY ELEMENT through probe heads (tests/tower_probe.py,
DESIGN.md 5.2): the policy head of the network is built so that the dense logits fpc_nn_forward returns are the tower's
16-bit activations themselves, and they are held against a float64 reference -- bit for bit on integer networks
(family A), within the measured noise of one more fp32 summation order on dense ones (family B) -- for every tower
kernel the engine can run: k_towerc, k_towerw<128> / <256> on one and two wave rows, k_tower, and k_conv3x3 per layer --
the path of every other hidden width: hidden 64 on every board of 8..14 a side, hidden 192 .. 512 in steps of 64 at 8x8."""
import copy

import numpy as np
import pytest

import tower_probe as tp
import weights
from fpc_testlib import make_engine

pytestmark = pytest.mark.gpu

INV_OF = {8: 2, 9: 2, 10: 2, 11: 3, 12: 3, 13: 3, 14: 3}


def _engine(R, rows, dtype, knobs, monkeypatch):
    if knobs:                                    # developer knobs are read only under FPC_DEV_KNOBS=1
        monkeypatch.setenv("FPC_DEV_KNOBS", "1")
        for k, v in knobs.items():
            monkeypatch.setenv(k, v)
    else:
        monkeypatch.delenv("FPC_DEV_KNOBS", raising=False)
    return make_engine("gpu", R, INV_OF[R], max_games=rows, max_sims=4, nn_dtype=dtype)


def _run(eng, blob, x_dev, kernel):
    import torch
    eng.load_weights(blob)
    assert (eng.L.fpc_nn_kernel(eng.h) or b"").decode() == kernel
    n = x_dev.shape[0]
    lg = torch.full((n, eng.A), float("nan"), device="cuda")
    va = torch.full((n,), float("nan"), device="cuda")
    eng.nn_forward(x_dev.data_ptr(), n, lg.data_ptr(), va.data_ptr())
    torch.cuda.synchronize()
    return lg.cpu().numpy(), va.cpu().numpy()


@pytest.mark.parametrize("case", tp.CASES, ids=tp.case_id)
def test_tower_elements_through_probe_heads(case, monkeypatch):
    """Tower probes at every channel offset, then the policy-conv probe, then the value.
    Family A: bit for bit (the value: bounded like family B's, against tanh of the float64 pre-activation).  Family B: largest distance from the float64 reference <= max(2 roundings, 2 x the CPU fp32
    order's), share of elements more than one rounding away <= 2 x the CPU's; both figures printed per case."""
    import torch
    kernel, R, hidden, blocks, dtype, family, knobs, rows = case
    p = tp.prepare(case)
    ref, m = p["ref"], p["net"]
    A_ch, RR = 8 * R + 8, R * R
    ident = tp.tail(R, dtype, weights.default_fc_layout(R), "identity")
    x_dev = torch.from_numpy(p["x"]).cuda()
    eng = _engine(R, rows, dtype, knobs, monkeypatch)
    what = tp.case_id(case)
    try:
        offs, _ = tp.probe_offsets(R, hidden)
        tower = np.full(ref["tower"].shape, np.nan, np.float32)
        for c0 in offs:
            pm = copy.deepcopy(m)
            width = tp.set_tower_probe(pm, c0)
            lg, va = _run(eng, tp.splice(pm, ident), x_dev, kernel)
            lg = lg.reshape(rows, A_ch, R, R)
            assert not lg[:, width:].any(), (what, c0, "output channels past the probe's width are not zero")
            if family == "A":
                tp.check_exact(lg[:, :width], ref["tower"][:, c0:c0 + width], "%s tower channels %d..%d" % (what, c0, c0 + width - 1))
            tower[:, c0:c0 + width] = lg[:, :width]
        if family == "B":
            tp.check_bounded(tower, ref["tower"], p["cpu"]["tower"], dtype, what + " tower")
        lg, va = _run(eng, tp.splice(m, ident), x_dev, kernel)
        lg = lg.reshape(rows, A_ch, R, R)
        if family == "A":
            tp.check_exact(lg, ref["policy"], what + " policy conv")
            assert np.isfinite(va).all()
        else:
            tp.check_bounded(lg, ref["policy"], p["cpu"]["policy"], dtype, what + " policy conv")
        # the value, both families: tanh of the float64 reference's pre-activation (family A: the value conv's output is the
        # reference's integers, what remains is the value Linear's own indexing -- q / R, q % R on every board -- and sum)
        vk = "value" if kernel == "k_conv3x3" else "value_unrounded"     # the towers never round the value conv's output
        dv = float(np.abs(va.astype(np.float64) - p["ref_value"][vk]).max())
        lim = max(p["value_floor"], 2.0 * p["cpu"][vk])
        print("%s %s: CPU f32 order %.3e, kernel %.3e, bound %.3e" % (what, vk, p["cpu"][vk], dv, lim))
        assert dv <= lim, (what, "value", dv, lim)
    finally:
        eng.close()


@pytest.mark.parametrize("R,hidden,kernel,dtype,layout", [(8, 128, "k_towerw", 1, 2), (8, 128, "k_towerw", 1, 1), (8, 128, "k_towerw", 0, 2),
                                                          (8, 128, "k_towerw", 0, 1), (14, 128, "k_towerc", 1, 2), (14, 128, "k_towerc", 1, 1)])
def test_permutation_linear_index_by_index(R, hidden, kernel, dtype, layout, monkeypatch):
    """A permutation matrix with entries +-2^k behind a dense (family B) policy conv: logit i must be scale[i] times
    policy activation perm[i], EXACTLY -- the NCHW -> NHWC input permutation, the fragment order and the padding to
    Np / Kp of both Linear layouts, index by index.  The activations are the engine's own, read through the identity
    Linear of the same layout (held against the reference by the test above), 37 and 300 rows (two Linear row tiles)."""
    import torch
    for rows in (37, 300) if R == 8 else (37,):
        case = (kernel, R, hidden, 2, dtype, "B", {}, rows)
        p = tp.prepare(case)
        x_dev = torch.from_numpy(p["x"]).cuda()
        eng = _engine(R, rows, dtype, {}, monkeypatch)
        try:
            plain, _ = _run(eng, tp.splice(p["net"], tp.tail(R, dtype, layout, "identity")), x_dev, kernel)
            tp.check_bounded(plain.reshape(p["ref"]["policy"].shape), p["ref"]["policy"], p["cpu"]["policy"], dtype,
                             "identity Linear layout %d %s R=%d rows=%d" % (layout, tp.FMT[dtype]["name"], R, rows))
            got, _ = _run(eng, tp.splice(p["net"], tp.tail(R, dtype, layout, "perm")), x_dev, kernel)
            assert (plain != 0).mean() > 0.2
            tp.check_exact(got, tp.expected_logits(plain.astype(np.float64), "perm", R), "permutation Linear layout %d" % layout)
        finally:
            eng.close()
