"""The policy Linear's stage loop and split-K reduce on the MI355X, held by what must not depend on how pieces are issued
(k_fcw / k_fcw8: one M0 write per group of LDS-DMA pieces, every piece addressed through the instruction's immediate;
k_fc_reduce: all of a column's slabs requested before the first is added; csrc/fpc_fc.h).

A random, non-integer network (weights_cases.model) through fpc_nn_forward's dense logits:
  * three forwards of the same 256 rows give identical bits;
  * a forward of 37 of those rows and one of a single row (tower_probe.linear_rows: windows that do not start at row 0)
    give those rows' bits again -- rows are independent in k_fcw and in the reduce, so a piece that lands late, or in
    another place than the fragment reads expect it, shows up as a difference here.
Shapes: 8x8 (9 stages per block, an odd count; 8 slabs per column = LOGIT_MAX_SLABS), 9x9 (13 stages), fp16 and bf16;
int8 weights at 8x8 (k_fcw8); fc_layout 1 at 10x10 (k_fc16's long / short slab mix through the same reduce).
The 14x14 shape is held element by element by tests/test_linear_probe_gpu.py."""
import numpy as np
import pytest

import tower_probe as tp
import weights
import weights_cases as wc
from fpc_testlib import make_engine
from legal_head_cases import INV_OF

pytestmark = pytest.mark.gpu

ROWS = 256


def _inputs(R):
    rng = np.random.default_rng(700 + R)
    return (rng.random((ROWS, 24, R, R)) < 0.1).astype(np.float32)


def _forward(eng, x, n):
    """fpc_nn_forward of n rows into n + 1 rows of NaN; the logits' and values' bits"""
    import torch
    x_dev = torch.from_numpy(np.ascontiguousarray(x)).cuda()
    lg = torch.full((n + 1, eng.A), float("nan"), device="cuda")
    va = torch.full((n + 1,), float("nan"), device="cuda")
    eng.nn_forward(x_dev.data_ptr(), n, lg.data_ptr(), va.data_ptr())
    torch.cuda.synchronize()
    lg, va = lg.cpu().numpy(), va.cpu().numpy()
    assert np.isnan(lg[n]).all() and np.isnan(va[n]), "the row behind the last was written"
    return lg[:n].view(np.uint32), va[:n].view(np.uint32)


def _same(got, want, what):
    bad = np.nonzero(got != want)
    assert bad[0].size == 0, "%s: %d words differ, first at %s" % (what, bad[0].size, tuple(int(b[0]) for b in bad))


@pytest.mark.parametrize("R,dtype,layout,fcw,kernel,stages,slabs", [
    (8, 1, 2, "w16", "k_fcw", 9, 8),
    (8, 0, 2, "w16", "k_fcw", 9, 8),
    (9, 1, 2, "w16", "k_fcw", 13, 8),
    (9, 0, 2, "w16", "k_fcw", 13, 8),
    (8, 1, 2, "int8", "k_fcw8", 9, 8),
    (10, 1, 1, "w16", "k_fc16", None, None),
], ids=["8x8-fp16", "8x8-bf16", "9x9-fp16", "9x9-bf16", "8x8-int8", "10x10-layout1"])
def test_same_bits_across_repeats_and_row_counts(R, dtype, layout, fcw, kernel, stages, slabs):
    A = (8 * R + 8) * R * R
    if layout == 2:
        sk = weights.fcw_split(R)
        assert sk == slabs and ((A + 511) // 512 * 512) // 64 // sk == stages
    blob = weights.export_weights(wc.model(R, 1, 128), dtype, fc_layout=layout, fc_weights=fcw)
    x = _inputs(R)
    eng = make_engine("gpu", R, INV_OF[R], max_games=ROWS, max_sims=4, nn_dtype=dtype)
    try:
        eng.load_weights(blob)
        del blob
        assert eng.nn_fc_kernel() == kernel
        lg, va = _forward(eng, x, ROWS)
        f = lg.view(np.float32)
        assert np.isfinite(f).all() and np.isfinite(va.view(np.float32)).all()
        # a network that says something: non-integer logits that differ from row to row and from column to column
        assert (f != np.rint(f)).mean() > 0.9 and f.std(axis=1).min() > 0
        assert not np.array_equal(lg[0], lg[1]) and not np.array_equal(lg[:, 0], lg[:, 1])
        for rep in (2, 3):
            lg2, va2 = _forward(eng, x, ROWS)
            _same(lg2, lg, "%s, forward %d of the same %d rows" % (kernel, rep, ROWS))
            _same(va2, va, "values, forward %d" % rep)
        for n in (37, 1):
            sel = tp.linear_rows(ROWS, n)
            lgn, _ = _forward(eng, x[sel], n)
            _same(lgn, lg[sel], "%s, %d rows against the same rows of %d" % (kernel, n, ROWS))
    finally:
        eng.close()
