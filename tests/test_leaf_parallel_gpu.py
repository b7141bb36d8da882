"""Leaf-parallel search (fpc_search_set_leaves) on the MI355X: the product kernels against the plain-Python model
(tests/search_model.py), the fused fpc_search_run against the step-wise C-ABI fed by fpc_nn_forward (k_towerc and
k_towerw, both policy heads, strict and fixed rules with root noise, partial last steps), more than 256 rows, and the
reference-default shape end to end."""
import numpy as np
import pytest

import evaluators
import fpc_ffi
import search_model as sm
from fpc_testlib import make_engine, roots_of
from oracle import orc
from test_nn_gpu import INV_OF, _model, _positions

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("R,G,sims,K,kind", [(8, 48, 100, 2, "hash"), (8, 64, 120, 3, "ramp"), (14, 48, 101, 2, "hash")])
def test_engine_equals_model(R, G, sims, K, kind):
    INV = INV_OF[R]
    boards = sm.positions(R, G, seed=200 + K)
    ev = evaluators.make(kind, R)
    rc, model, counts = sm.search([orc.clone(b) for b in boards], R, INV, sims, 3.0, ev, K)
    assert rc == 0 and counts["collisions"] > 0
    eng = make_engine("gpu", R, INV, max_games=G * K, max_sims=sims)
    res = sm.run_stepwise(eng, "gpu", roots_of(boards, R), sims, 3.0, ev, K)
    sm.compare(eng, res, model, (R, G, K, kind), grand_every=7)
    eng.close()


def _fused_vs_stepwise(R, G, blocks, hidden, dtype, rules, K, sims, noise=False):
    import torch
    import weights
    m = _model(R, blocks, hidden, seed=5)
    eng = make_engine("gpu", R, INV_OF[R], max_games=G * K, max_sims=sims, nn_dtype=dtype)
    eng.load_weights(weights.export_weights(m, dtype))
    eng.set_rules(rules)
    if noise:
        eng.set_root_noise(np.random.default_rng(9).standard_gamma(0.3, size=(G, fpc_ffi.MAX_MOVES)).astype(np.float32), 0.25)
    boards = _positions(R, G)
    roots_a = [fpc_ffi.clone_board(b) for b in boards]
    eng.set_leaves(K)
    eng.search_begin(roots_a, 3.0)
    eng.search_run(sims)
    res_a = eng.search_results(roots=roots_a)

    def ev(enc):
        n = enc.shape[0]
        x = torch.from_numpy(np.ascontiguousarray(enc)).cuda()
        lg = torch.empty(n, eng.A, device="cuda")
        va = torch.empty(n, device="cuda")
        torch.cuda.synchronize()
        eng.nn_forward(x.data_ptr(), n, lg.data_ptr(), va.data_ptr())
        return lg.cpu().numpy(), va.cpu().numpy()

    roots_b = [fpc_ffi.clone_board(b) for b in boards]
    res_b = sm.run_stepwise(eng, "gpu", roots_b, sims, 3.0, ev, K)
    for k in ("root_n", "n_children", "sims_done", "flat", "visits", "prior", "w"):
        assert np.array_equal(res_a[k], res_b[k]), k
    for a, b in zip(roots_a, roots_b):
        assert bytes(a) == bytes(b)
    assert int(res_a["sims_done"].sum()) > G * sims // 2 and int(res_a["sims_done"].max()) <= sims
    kernel = eng.L.fpc_nn_kernel(eng.h).decode()
    eng.set_leaves(1)
    eng.close()
    return kernel


@pytest.mark.parametrize("R,hidden,dtype,rules,K,sims,kernel", [
    (14, 128, 1, 0, 2, 23, "k_towerc"),
    (14, 128, 1, 15, 3, 20, "k_towerc"),
    (8, 256, 1, 0, 3, 25, "k_towerw"),
    (8, 256, 0, 15, 2, 21, "k_towerw"),
    (14, 256, 1, 0, 2, 15, "k_towerw"),
])
def test_fused_equals_stepwise(R, hidden, dtype, rules, K, sims, kernel):
    got = _fused_vs_stepwise(R, 12, 2, hidden, dtype, rules, K, sims, noise=bool(rules))
    assert got == kernel


def test_fused_equals_stepwise_more_than_256_rows():
    _fused_vs_stepwise(8, 100, 2, 256, 1, 0, 3, 10)


@pytest.mark.parametrize("R,hidden,rules", [(8, 256, 0), (14, 128, 15)])
def test_legal_head_with_leaves(R, hidden, rules):
    """FPC_POLICY_LEGAL with K = 2: the legal-only head's kernels (k_policy_gemv over the rows, k_expand_legal(_select)_multi)
    against the full head at the same K -- the same priors up to f32 rounding, the same searches up to near-ties"""
    import weights
    m = _model(R, 2, hidden, seed=23)
    G, K, sims = 24, 2, 31
    boards = _positions(R, G)
    out = {}
    for mode in (False, True):
        eng = make_engine("gpu", R, INV_OF[R], max_games=G * K, max_sims=sims, nn_dtype=1)
        eng.load_weights(weights.export_weights(m, 1))
        eng.set_rules(rules)
        eng.set_policy_mode(mode)
        eng.set_leaves(K)
        runs = []
        for s in (K, sims):
            roots = [fpc_ffi.clone_board(b) for b in boards]
            eng.search_begin(roots, 3.0)
            eng.search_run(s)
            runs.append(eng.search_results(roots=roots))
        out[mode] = runs
        eng.close()
    (f1, f2), (l1, l2) = out[False], out[True]
    assert (f1["n_children"] == l1["n_children"]).all() and (f1["flat"] == l1["flat"]).all()
    assert np.abs(f1["prior"] - l1["prior"]).max() < 2e-5 and np.abs(f1["w"] - l1["w"]).max() == 0.0
    same = sum(1 for g in range(G) if (f2["visits"][g] == l2["visits"][g]).all())
    assert same >= G - 3, same
    assert (f2["sims_done"] == l2["sims_done"]).sum() >= G - 3


def test_reference_default_shape():
    """the reference's shipped default, ResNet(15,256) with 100 games x 50 searches at 8x8, with 2 leaves per step"""
    import weights
    R, G, K, sims = 8, 100, 2, 50
    m = _model(R, 15, 256, seed=1)
    eng = make_engine("gpu", R, INV_OF[R], max_games=G * K, max_sims=sims, nn_dtype=1)
    eng.load_weights(weights.export_weights(m, 1))
    eng.set_leaves(K)
    roots = _positions(R, G)
    eng.search_begin(roots, 3.0)
    eng.search_run(sims)
    res = eng.search_results(roots=roots)
    assert int(res["sims_done"].max()) <= sims and int(res["sims_done"].sum()) > G * sims // 2
    assert (res["root_n"] == 1 + res["sims_done"]).all()
    assert (res["n_children"] > 0).all()
    eng.close()


def test_explicit_single_leaf_is_identical():
    """with the internal network, set_leaves(1) gives exactly the search of an engine that never heard of it"""
    import weights
    R, G, sims = 8, 16, 30
    m = _model(R, 2, 256, seed=2)
    res = []
    for explicit in (False, True):
        eng = make_engine("gpu", R, INV_OF[R], max_games=2 * G, max_sims=sims, nn_dtype=1)
        eng.load_weights(weights.export_weights(m, 1))
        if explicit:
            eng.set_leaves(2)
            eng.set_leaves(1, 3.0)
        roots = _positions(R, G)
        eng.search_begin(roots, 3.0)
        eng.search_run(sims)
        res.append(eng.search_results(roots=roots))
        eng.close()
    for k in ("root_n", "n_children", "sims_done", "flat", "visits", "prior", "w"):
        assert np.array_equal(res[0][k], res[1][k]), k


def _legal_search(m, R, boards, sims, rules, k_begin, k_run, hidden_dtype=1):
    import weights
    G = len(boards)
    eng = make_engine("gpu", R, INV_OF[R], max_games=G * max(k_begin, k_run), max_sims=sims, nn_dtype=hidden_dtype)
    eng.load_weights(weights.export_weights(m, hidden_dtype))
    eng.set_rules(rules)
    eng.set_policy_mode(True)
    eng.set_leaves(k_begin)
    roots = [fpc_ffi.clone_board(b) for b in boards]
    eng.search_begin(roots, 3.0)
    eng.set_leaves(k_run)
    eng.search_run(sims)
    res = eng.search_results(roots=roots)
    eng.close()
    return res, roots


@pytest.mark.parametrize("R,hidden,rules", [(8, 256, 0), (14, 128, 15)])
def test_legal_head_multi_kernels_one_leaf_bit_exact(R, hidden, rules):
    """the legal head's leaf-parallel kernels (k_select_multi, k_policy_gemv over the rows, k_expand_legal(_select)_multi)
    driven with one leaf per step give exactly the one-leaf kernels' search"""
    m = _model(R, 2, hidden, seed=29)
    boards = _positions(R, 20)
    a, ra = _legal_search(m, R, boards, 24, rules, 1, 1)
    b, rb = _legal_search(m, R, boards, 24, rules, 2, 1)          # begun leaf-parallel, run with K = 1
    for k in ("root_n", "n_children", "sims_done", "flat", "visits", "prior", "w"):
        assert np.array_equal(a[k], b[k]), k
    assert [bytes(x) for x in ra] == [bytes(x) for x in rb]


@pytest.mark.parametrize("R,hidden,K", [(8, 256, 2), (14, 128, 3)])
def test_legal_head_rows_are_per_game_bit_exact(R, hidden, K):
    """FPC_RULES_FIXED rotates every row by its own side to move, so a game's leaf-parallel search cannot depend on the
    other games of the batch: the games reversed (every row index changes), and a batch of the first games alone, must
    give each game's search bit for bit -- any mix-up of rows k*G + g in the legal head's kernels shows here"""
    m = _model(R, 2, hidden, seed=31)
    G, sims = 18, 3 * K + 1
    boards = _positions(R, G)
    a, _ = _legal_search(m, R, boards, sims, 15, K, K)
    b, _ = _legal_search(m, R, boards[::-1], sims, 15, K, K)
    c, _ = _legal_search(m, R, boards[:5], sims, 15, K, K)
    for k in ("root_n", "n_children", "sims_done", "flat", "visits", "prior", "w"):
        assert np.array_equal(a[k], b[k][::-1]), k
        assert np.array_equal(a[k][:5], c[k]), k
    assert int(a["sims_done"].sum()) > G * sims // 2
