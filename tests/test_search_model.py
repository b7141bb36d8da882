"""The plain-Python search model (tests/search_model.py) with one leaf per game against the oracle's C++ orc_search,
bit for bit, with no engine in between: the model the leaf-parallel and tree-reuse tests hold the engine against is
itself held to the oracle, which the golden vectors pin to the reference."""
import numpy as np
import pytest

import evaluators
import search_model as sm
from oracle import orc


@pytest.mark.parametrize("R,INV", [(8, 2), (14, 3)])
def test_one_leaf_model_equals_oracle(R, INV):
    boards = sm.positions(R, 5, seed=77)
    ev = evaluators.make("hash", R)
    rc, oref = orc.search([orc.clone(b) for b in boards], R, INV, 12, 3.0, ev)
    assert rc == 0
    model = sm.Model([orc.clone(b) for b in boards], R, INV, 3.0, ev)
    assert model.search(12) == 0
    got = model.results()
    assert len(got) == len(oref)
    for g, (m, o) in enumerate(zip(got, oref)):
        for k in ("root_n", "children", "sims_done", "terminated"):
            assert m[k] == o[k], (g, k)
        assert np.array_equal(m["priors"], o["priors"]), (g, "priors")
        assert np.array_equal(m["w"], o["w"]), (g, "value sums")
        a, b = m["board"], o["board"]
        assert orc.lists_of(a) == orc.lists_of(b) and bytes(a.sq) == bytes(b.sq) and a.turn == b.turn, (g, "root state")
        assert list(a.king) == list(b.king) and list(a.castle) == list(b.castle), (g, "root state")
