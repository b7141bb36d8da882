"""Playout cap randomization (fpc_search_set_fast_rows, FPC_TUPLE_FAST, fpc_replay_batch_w; include/fpc_engine.h, DESIGN.md
5.12): the cases that run both on the wavefront emulator (tests/test_playout_cap_emul.py) and on the GPU
(tests/test_playout_cap_gpu.py).  The model is tests/playout_cap_model.py; the shapes, the evaluator and the constants are
those of tests/forced_cases.py.  Everything is compared exactly; there is no tolerance in this file."""
import ctypes as C

import numpy as np

import evaluators
import forced_cases as fc
import fpc_ffi
import playout_cap_model as pm
import search_model as sm
import selfplay
import solver_cases as sc
import solver_model as so
import tuples
from fpc_testlib import make_engine, roots_of

R, INV = fc.R, fc.INV
NO_TERMINAL, SELFPLAY = fc.NO_TERMINAL, fc.SELFPLAY
EINVAL, ESTATE = fc.EINVAL, fc.ESTATE
FACTOR, C_PUCT = fc.FACTOR, fc.C_PUCT
MASKS = {4: [0, 1, 0, 1], 3: [1, 0, 0]}

#         pos     rules        fpu    solver  K   G  sims  noise seed   (seeds chosen on the CPU, from the model alone, so that
#                                                                        conditions() holds; under rules 47 the solver is inert)
CASES = [("near", SELFPLAY, False, False, 1, 4, 80, 101),
         ("near", SELFPLAY, True, False, 3, 4, 80, 4),
         ("near", SELFPLAY, False, True, 3, 4, 80, 6),
         ("near", SELFPLAY, True, True, 1, 4, 80, 101),
         ("near", NO_TERMINAL, False, False, 3, 4, 80, 100),
         ("near", NO_TERMINAL, True, True, 1, 4, 80, 100),
         ("start", SELFPLAY, False, False, 1, 3, 64, 11),
         ("start", SELFPLAY, True, True, 3, 3, 64, 12),
         ("start", NO_TERMINAL, True, False, 3, 3, 64, 15),
         ("start", NO_TERMINAL, False, True, 1, 3, 64, 16)]
IDS = ["%s-rules%d-fpu%d-solver%d-K%d" % (c[0], c[1], c[2], c[3], c[4]) for c in CASES]
_models = {}


def mask_of(case):
    return MASKS[case[5]]


def searched_model(case):
    """(boards, gamma, mask, Model after its search under the mixed mask) of a case, computed once and never changed"""
    if case not in _models:
        pos, rules, fpu, solver, K, G, sims, seed = case
        boards = fc.boards_for(pos, rules, G)
        gamma = fc.gamma_for(G, seed)
        model = fc._model(pm.Model, boards, rules, fpu, solver, gamma, forced=FACTOR)
        model.set_fast(mask_of(case))
        assert model.forced_in_effect() and model.in_effect() == (solver and rules == SELFPLAY)
        assert model.search(sims, K) == 0
        _models[case] = (boards, gamma, mask_of(case), model)
    return _models[case]


def _kids(model, g):
    """game g's tree through the second level: what fpc_search_results and fpc_search_grandchildren report"""
    return [(c.flat, c.N, c.W, [(x.flat, x.N) for x in c.children]) for c in model.roots[g].children]


def all_full_model(case):
    """the model's search of the same inputs without a mask: every row forced and pruned"""
    key = ("all full", case)
    if key not in _models:
        pos, rules, fpu, solver, K, G, sims, seed = case
        model = fc._model(pm.Model, fc.boards_for(pos, rules, G), rules, fpu, solver, fc.gamma_for(G, seed), forced=FACTOR)
        assert model.search(sims, K) == 0
        _models[key] = model
    return _models[key]


def conditions():
    """the cap on the inputs, asserted from the model alone.  In every case: on some FULL row the forced rule decided a
    selection and the pruning took a visit out; on some FAST row the rule, had it been applied, would have chosen another
    child at some root selection (withheld), that row's tree is not the row's tree in the all-full search of the same
    inputs -- so the gate is observable -- and its target is its stored counts."""
    for case in CASES:
        _, _, mask, model = searched_model(case)
        tg = model.targets()
        full = [g for g, m in enumerate(mask) if not m]
        fast = [g for g, m in enumerate(mask) if m]
        assert any(model.decided[g] >= 1 and sum(c.N for c in model.roots[g].children) > sum(tg[g]) for g in full), (case, model.decided)
        assert any(model.withheld[g] >= 1 for g in fast), (case, model.withheld)
        assert all(tg[g] == [c.N for c in model.roots[g].children] for g in fast), case
        assert all(model.decided[g] == 0 for g in fast), case
        forced = all_full_model(case)
        assert any(_kids(model, g) != _kids(forced, g) for g in fast), case
        assert all(_kids(model, g) == _kids(forced, g) for g in full), case
    return len(CASES)


def _begin_masked(eng, boards, sims, K, mask):
    eng.set_leaves(sm.schedule(sims, K)[0], 1.0)
    roots = roots_of(boards, R)
    eng.search_begin(roots, C_PUCT)
    if mask is not None:
        eng.search_set_fast_rows(mask)
    return roots


def _search(eng, backend, boards, sims, K, mask, fused=True):
    roots = _begin_masked(eng, boards, sims, K, mask)
    sm.run_steps(eng, backend, sims, evaluators.make("hash", R), K, 1.0, fused)
    return eng.search_results(roots=roots)


# ---- 1. engine == model -----------------------------------------------------------------------------------------------
def engine_vs_model(backend, case, fused):
    pos, rules, fpu, solver, K, G, sims, _ = case
    boards, gamma, mask, model = searched_model(case)
    eng = make_engine(backend, R, INV, max_games=G * K, max_sims=sims)
    try:
        fc._setup(eng, rules, fpu, solver, FACTOR, gamma)
        res = _search(eng, backend, boards, sims, K, mask, fused)
        fc.compare_all(eng, res, model, (case, fused))
        assert sc._alive(res) == model.alive or not rules & 16, (case, "alive")
    finally:
        fc._close(eng)


# ---- 2. row independence, engine against engine -----------------------------------------------------------------------
def _snapshot(eng, res):
    return res, eng.search_targets().copy(), [a.copy() for a in eng.search_proofs()]


def row_independence(backend, case):
    """every rule set used holds FPC_RULES_ROTATION: under the mixed mask game g is bit for bit game g of the no-mask search
    (a full row) or of the factor = 0 search (a fast row), the gamma rows being the same in all three"""
    pos, rules, fpu, solver, K, G, sims, _ = case
    assert rules & 4                                                                   # FPC_RULES_ROTATION
    boards, gamma, mask, _ = searched_model(case)
    eng = make_engine(backend, R, INV, max_games=G * K, max_sims=sims)
    try:
        fc._setup(eng, rules, fpu, solver, FACTOR, gamma)
        mixed = _snapshot(eng, _search(eng, backend, boards, sims, K, mask))
        full = _snapshot(eng, _search(eng, backend, boards, sims, K, None))
        eng.set_forced(0.0)
        plain = _snapshot(eng, _search(eng, backend, boards, sims, K, None))
        differs = 0
        for g in range(G):
            ref = plain if mask[g] else full
            other = full if mask[g] else plain
            sm.same_results(mixed[0], ref[0], [g], [g])
            assert np.array_equal(mixed[1][g], ref[1][g]), (case, g, "targets")
            assert mixed[2][0][g] == ref[2][0][g] and np.array_equal(mixed[2][1][g], ref[2][1][g]), (case, g, "proofs")
            n = int(mixed[0]["n_children"][g])
            differs += (not np.array_equal(mixed[0]["visits"][g, :n], other[0]["visits"][g, :n]) or
                        not np.array_equal(mixed[1][g], other[1][g]))
        assert differs >= 1, case                    # the two references are not the same search
    finally:
        fc._close(eng)


# ---- 4 + 5. tuples and replay -------------------------------------------------------------------------------------------
def decode_w(eng, backend, ring, slots, weights=True):
    """replay_batch(..., w=) into NaN-filled outputs (an element the kernel leaves out shows), back as numpy"""
    n, A = len(slots), eng.A
    shapes = ((n, 24, eng.R, eng.R), (n, A), (n,), (n,))[:4 if weights else 3]
    if backend == "emul":
        out = [np.full(s, np.nan, np.float32) for s in shapes]
        eng.replay_batch(ring, slots, *out[:3], **({"w": out[3]} if weights else {}))
        return out
    import torch
    out = [torch.full(s, float("nan"), dtype=torch.float32, device="cuda") for s in shapes]
    torch.cuda.synchronize()
    eng.replay_batch(ring, slots, *out[:3], **({"w": out[3]} if weights else {}))
    return [o.cpu().numpy() for o in out]


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.int32)


def _records_bytes(arr, n, clear_flags):
    raw = bytearray(bytes(memoryview(arr).cast("B"))[:n * C.sizeof(fpc_ffi.Tuple)])
    if clear_flags:
        for i in range(n):
            raw[i * C.sizeof(fpc_ffi.Tuple) + fpc_ffi.Tuple.flags.offset] = 0
    return bytes(raw)


def _replay_equal(eng, backend, ring, recs, slots, tag):
    """replay_batch(..., w=) of the slots: w is 0.0 / 1.0 by flag; enc, pi, z are plain replay_batch's and dense_pi's bits"""
    enc, pi, z, w = decode_w(eng, backend, ring, slots)
    enc0, pi0, z0 = decode_w(eng, backend, ring, slots, weights=False)
    assert np.array_equal(bits(enc), bits(enc0)) and np.array_equal(bits(pi), bits(pi0)) and np.array_equal(bits(z), bits(z0)), tag
    for i, s in enumerate(slots):
        r = recs[s]
        want_w = np.float32(0.0 if r["fast"] else 1.0)
        assert bits(w[i:i + 1])[0] == bits(want_w.reshape(1))[0], (tag, i, "w")
        want_pi = tuples.dense_pi(r, eng.A).numpy() if len(r["flat"]) else np.zeros(eng.A, np.float32)
        assert np.array_equal(bits(pi[i]), bits(want_pi)), (tag, i, "pi")
        assert bits(z[i:i + 1])[0] == bits(np.float32(r["z"]).reshape(1))[0], (tag, i, "z")


def tuples_and_replay(backend, case):
    """fpc_collect_tuples after the mixed search: flags by mask, visits T_k on full rows and N_k on fast rows; with forcing
    off only the flag differs from the records of the same search without a mask; the records go through a ring and
    fpc_replay_batch_w"""
    pos, rules, fpu, solver, K, G, sims, _ = case
    boards, gamma, mask, model = searched_model(case)
    eng = make_engine(backend, R, INV, max_games=G * K, max_sims=sims)
    try:
        fc._setup(eng, rules, fpu, solver, FACTOR, gamma)
        res = _search(eng, backend, boards, sims, K, mask)
        fc.compare_all(eng, res, model, ("tuples", case), grand_every=0)
        eng.tuples_reserve(G)
        eng.collect_tuples(None, 0)
        eng.tuples_set_z(list(range(G)), np.linspace(-1.0, 1.0, G, dtype=np.float32), np.linspace(0.5, -0.5, G, dtype=np.float32))
        arr, n = eng.tuples_read()
        assert n == G
        tg = model.targets()
        pruned = 0
        for g in range(G):
            kids = model.roots[g].children
            assert int(arr[g].flags) == (fpc_ffi.TUPLE_FAST if mask[g] else 0), (case, g, "flags")
            assert int(arr[g].n) == len(kids) and [int(arr[g].flat[k]) for k in range(len(kids))] == [c.flat for c in kids], (case, g)
            assert [int(arr[g].visits[k]) for k in range(len(kids))] == tg[g], (case, g, "visits")
            if mask[g]:
                assert tg[g] == [c.N for c in kids], (case, g)
            else:
                pruned += sum(c.N for c in kids) - sum(tg[g])
        assert pruned >= 1, case                                                        # condition: T_k is not N_k on a full row
        recs = tuples.records_of(arr, n, R)
        assert [r["fast"] for r in recs] == [bool(m) for m in mask]
        eng.replay_reserve(0, G + 1)
        eng.replay_push()
        _replay_equal(eng, backend, 0, recs, list(range(G)), (case, "in order"))
        _replay_equal(eng, backend, 0, recs, [G - 1, 0, 0, 1, G - 1], (case, "any order"))
        assert tuples.weights_of(recs).view(-1).tolist() == [0.0 if m else 1.0 for m in mask]
        # forcing off: only the flag differs from today's records
        eng.set_forced(0.0)
        for m in (mask, None):
            _search(eng, backend, boards, sims, K, m)
            eng.tuples_reset()
            eng.collect_tuples(None, 0)
            a, cnt = eng.tuples_read()
            if m is not None:
                assert [int(a[g].flags) for g in range(G)] == mask
                masked = _records_bytes(a, cnt, True)
            else:
                assert not any(int(a[g].flags) for g in range(G))
                assert _records_bytes(a, cnt, False) == masked, case
        eng.tuples_reserve(0)
    finally:
        fc._close(eng)


def replay_14x14(backend):
    """fpc_replay_batch_w at 14x14 / INV 3 (A = 23520) on records loaded with fpc_replay_load alone: n = 0, n = 256, a zero
    visit sum, some flagged and some not"""
    import replay_cases as rc
    RR, INV3 = 14, 3
    eng = make_engine(backend, RR, INV3, max_games=4, max_sims=4)
    try:
        assert eng.A == 23520
        recs = rc.edge_records(RR)
        zero = dict(recs[5])
        zero["visits"] = np.zeros_like(zero["visits"])
        recs.append(zero)
        for k, r in enumerate(recs):
            r["fast"] = k % 3 != 1
        ns = [len(r["flat"]) for r in recs]
        assert 0 in ns and 256 in ns and not recs[-1]["visits"].any() and len(recs[-1]["flat"]) > 0
        assert {r["fast"] for r in recs} == {True, False}
        n = len(recs)
        eng.replay_reserve(1, n)
        eng.replay_load(1, tuples.tuples_of(recs), n)
        back, cnt = eng.replay_read(1)
        assert [r["fast"] for r in tuples.records_of(back, cnt, RR)] == [r["fast"] for r in recs]      # the flag travels
        _replay_equal(eng, backend, 1, recs, list(range(n)), "14x14 in order")
        _replay_equal(eng, backend, 1, recs, [(7 * i + 3) % n for i in range(2 * n + 1)], "14x14 any order")
        enc, _, _, _ = decode_w(eng, backend, 1, list(range(n)))
        for i, r in enumerate(recs):
            assert np.array_equal(bits(enc[i]), bits(eng.encode([rc.board_of_rec(r)])[0])), i
        dev = None if backend == "emul" else "cuda"
        a = tuples.dense_batch_device(eng, recs, device=dev, weights=True)
        b = tuples.dense_batch(eng, recs, weights=True)
        for x, y in zip(a, b):
            assert np.array_equal(bits(x.cpu().numpy()), bits(y.numpy()))
        ptr = a[0].data_ptr()
        one = (C.c_int * 1)(0)
        assert eng.L.fpc_replay_batch_w(eng.h, 1, one, 1, ptr, a[1].data_ptr(), a[2].data_ptr(), None) == EINVAL     # null w_dev
        assert eng.L.fpc_replay_batch_w(None, 1, one, 1, ptr, ptr, ptr, ptr) == EINVAL
    finally:
        eng.close()


# ---- 6. play --------------------------------------------------------------------------------------------------------------
def play(backend, case, need_told=True):
    """fpc_search_play at temperatures 1 and 0 == selfplay.sample_move on T_k for a full row and on N_k for a fast row, with
    the solver's proofs where it is in effect (a proven root overrides the draw); result / next == today's calls"""
    from play_cases import _check_moves
    pos, rules, fpu, solver, K, G, sims, _ = case
    boards, gamma, mask, model = searched_model(case)
    tg = model.targets()
    u = list(np.random.default_rng(23).random(G))
    told = 0
    for g in range(G):
        kids = model.roots[g].children
        if kids and not mask[g] and not (model.in_effect() and model.status(model.roots[g]) in (so.WIN, so.DRAW)):
            x = fc._uniform_that_tells([c.flat for c in kids], [c.N for c in kids], tg[g])
            if x is not None:
                u[g], told = x, told + 1
    assert told >= 1 or not need_told                # condition: on a full row the draw from T_k is not the draw from N_k
    eng = make_engine(backend, R, INV, max_games=G * K, max_sims=sims)
    try:
        fc._setup(eng, rules, fpu, solver, FACTOR, gamma)
        res = _search(eng, backend, boards, sims, K, mask)
        fc.compare_all(eng, res, model, ("play", case), grand_every=0)
        rp, cp = eng.search_proofs()
        live = [g for g in range(G) if model.roots[g].children]
        for T in (1.0, 0.0):
            want = []
            for g in range(G):
                n = int(res["n_children"][g])
                counts = tg[g] if not mask[g] else [int(v) for v in res["visits"][g, :n]]
                want.append(selfplay.sample_move(res["flat"][g, :n], counts, T, u[g], rp[g], cp[g, :n]) if n else -1)
            assert want == [model.roots[g].children[model.pick(g, T, u[g])].flat if g in live else -1 for g in range(G)]
            flats, results, pods = eng.search_play(T, u)
            assert [int(f) for f in flats] == want, (case, T)
            if len(live) == G:
                _check_moves(eng, res, flats, results, pods, ("play", case, T))
        sm.same_results(res, eng.search_results())   # nothing was written into the tree
    finally:
        fc._close(eng)


def proven_root_case():
    """a case of the list in which, with the solver in effect, some root with children is proven WIN or DRAW"""
    for case in CASES:
        if case[3] and case[1] == SELFPLAY:
            _, _, _, model = searched_model(case)
            if any(st in (so.WIN, so.DRAW) and model.roots[g].children for g, st in enumerate(model.proofs()[0])):
                return case
    raise AssertionError("no case with a root proven WIN or DRAW")


# ---- 7. lifetime and errors -------------------------------------------------------------------------------------------------
LIFE = dict(case=CASES[3], more=32, useed=11, gseeds=(31, 32))


def lifetime(backend):
    """three plies with reuse: begin under the case's mask, fpc_search_advance under the complementary mask, then
    fpc_search_advance_refill with two fresh rows under a third; after every begin / advance the mask is gone (the targets
    right after it are the no-mask targets) until it is set again, and the engine equals the model at every ply"""
    c = LIFE
    pos, rules, fpu, solver, K, G, sims, seed = c["case"]
    ev = evaluators.make("hash", R)
    boards = fc.boards_for(pos, rules, G)
    gamma = fc.gamma_for(G, seed)
    model = fc._model(pm.Model, boards, rules, fpu, solver, gamma, forced=FACTOR)
    mask = mask_of(c["case"])
    model.set_fast(mask)
    assert model.search(sims, 1) == 0
    rng = np.random.default_rng(c["useed"])
    eng = make_engine(backend, R, INV, max_games=G + 2, max_sims=sims + 2 * c["more"])
    try:
        fc._setup(eng, rules, fpu, solver, FACTOR, gamma)
        res = _search(eng, backend, boards, sims, 1, mask)
        fc.compare_all(eng, res, model, "lifetime: ply 0", grand_every=0)
        for ply, refill in ((1, False), (2, True)):
            n_old = len(model.roots)
            u = rng.random(n_old)
            keep = [g for g in range(n_old) if model.roots[g].children]
            assert len(keep) >= 2
            flats = {g: model.roots[g].children[model.pick(g, 1.0, float(u[g]))].flat for g in keep}
            if refill:
                fresh_o = sm.positions(R, 2, seed=750, rules=rules & 15)
                src = keep[:1] + [-1] + keep[1:] + [-1]
                fresh = [None if s >= 0 else fresh_o.pop() for s in src]
            else:
                src, fresh = list(keep), None
            fl = [flats[s] if s >= 0 else 0 for s in src]
            n_new = len(src)
            gamma2 = fc.gamma_for(n_new, c["gseeds"][ply - 1])
            eng.set_root_noise(gamma2, fc.EPS)
            model.set_noise(gamma2)
            if refill:
                kept = eng.search_advance_refill(fl, src, fresh=[None if b is None else roots_of([b], R)[0] for b in fresh])
                want_kept = model.advance_refill(src, fl, fresh)
            else:
                kept = eng.search_advance(fl, src)
                want_kept = model.advance(src, fl)
            assert [int(k) for k in kept] == want_kept, (ply, "kept visits")
            assert model.fast is None
            fc.targets_equal(eng, model, "lifetime: the advance has cleared the mask")     # pruned on every row again
            new_mask = [(g + ply) & 1 for g in range(n_new)]
            eng.search_set_fast_rows(new_mask)
            eng.search_set_fast_rows(None)                                              # NULL clears ...
            fc.targets_equal(eng, model, "lifetime: NULL has cleared the mask")
            eng.search_set_fast_rows(new_mask)                                          # ... and the mask can be set again
            model.set_fast(new_mask)
            fc.targets_equal(eng, model, "lifetime: the mask is set, before any selection")
            sm.run_steps(eng, backend, c["more"], ev)
            res = eng.search_results()
            assert model.search(c["more"], 1) == 0
            fc.compare_all(eng, res, model, ("lifetime: ply", ply), grand_every=2)
            assert any(model.decided[g] for g in range(n_new) if not new_mask[g]) or ply == 2, model.decided
        # a begin clears it too
        roots = roots_of(boards, R)
        eng.set_root_noise(gamma, fc.EPS)
        eng.search_begin(roots, C_PUCT)
        sm.run_steps(eng, backend, sims, ev)
        res = eng.search_results(roots=roots)
        ref = fc._model(pm.Model, boards, rules, fpu, solver, gamma, forced=FACTOR)
        assert ref.search(sims, 1) == 0
        fc.compare_all(eng, res, ref, "lifetime: begin has cleared the mask", grand_every=0)
    finally:
        fc._close(eng)


def errors(backend):
    """fpc_search_set_budget's table for fpc_search_set_fast_rows; a refused call changes nothing"""
    G = 3
    boards = fc.boards_for("start", SELFPLAY, G)
    gamma = fc.gamma_for(G, 11)
    ev = evaluators.make("hash", R)
    eng = make_engine(backend, R, INV, max_games=G + 1, max_sims=16)
    try:
        L, h = eng.L, eng.h
        m = (C.c_uint8 * 4)(1, 0, 0, 0)
        p = C.cast(m, C.c_void_p)
        assert L.fpc_search_set_fast_rows(None, p, G) == EINVAL
        assert L.fpc_search_set_fast_rows(h, p, G) == ESTATE and L.fpc_search_set_fast_rows(h, None, G) == ESTATE     # no search
        fc._setup(eng, SELFPLAY, True, False, FACTOR, gamma)
        eng.set_leaves(1, 1.0)
        eng.search_begin(roots_of(boards, R), C_PUCT)
        assert L.fpc_search_set_fast_rows(h, p, G + 1) == EINVAL and L.fpc_search_set_fast_rows(h, p, G - 1) == EINVAL
        assert L.fpc_search_set_fast_rows(h, None, G + 1) == EINVAL
        assert L.fpc_search_set_fast_rows(h, p, G) == 0
        bad = (C.c_uint8 * 4)(0, 0, 2, 0)
        assert L.fpc_search_set_fast_rows(h, C.cast(bad, C.c_void_p), G) == EINVAL       # nothing uploaded: the mask is still m
        bad[2] = 255
        assert L.fpc_search_set_fast_rows(h, C.cast(bad, C.c_void_p), G) == EINVAL
        eng.search_results()                                                            # before any selection: closes nothing
        assert L.fpc_search_set_fast_rows(h, p, G) == 0
        eng.search_select()
        assert L.fpc_search_set_fast_rows(h, p, G) == ESTATE and L.fpc_search_set_fast_rows(h, None, G) == ESTATE
        eng.search_results()
        assert L.fpc_search_set_fast_rows(h, p, G) == ESTATE                             # finished and read: advance or begin
        roots = roots_of(boards, R)
        eng.search_begin(roots, C_PUCT)
        assert L.fpc_search_set_fast_rows(h, p, G) == 0
        assert L.fpc_search_set_fast_rows(h, C.cast(bad, C.c_void_p), G) == EINVAL
        assert L.fpc_search_set_fast_rows(h, p, G + 1) == EINVAL
        sm.run_steps(eng, backend, 16, ev)
        res = eng.search_results(roots=roots)
        model = fc._model(pm.Model, boards, SELFPLAY, True, False, gamma, forced=FACTOR)
        model.set_fast([1, 0, 0])
        assert model.search(16, 1) == 0
        fc.compare_all(eng, res, model, "errors: the refused calls changed nothing", grand_every=0)
    finally:
        fc._close(eng)
