"""Device-side weight pack on the GPU: fpc_weights_pack against weights.export_weights byte for byte, and
fpc_load_weights_device (first load, in place, geometry change, refusals, the MCTS opt-in) against engines loaded through
the host path."""
import copy
import ctypes as C

import numpy as np
import pytest

import weights
import weights_cases as wc
from fpc_testlib import make_engine

pytestmark = pytest.mark.gpu


def _engine(R, dtype, **kw):
    kw.setdefault("max_games", 4)
    kw.setdefault("max_sims", 16)
    return make_engine("gpu", R, wc.INV_OF[R], nn_dtype=dtype, **kw)


def _kernel(eng):
    return (eng.L.fpc_nn_kernel(eng.h) or b"").decode()


def _host_loaded(R, blocks, hidden, dtype, **kw):
    eng = _engine(R, dtype, **kw)
    m = wc.model(R, blocks, hidden)
    eng.load_weights(wc.reference_blob(m, (R, blocks, hidden), dtype, weights.default_fc_layout(R)))
    return eng


# ---- 1. bytes ------------------------------------------------------------------------------------------------------------
_BYTES = [(R, hidden, dtype, layout) for R in (8, 9, 11) for hidden in (64, 128) for dtype in (0, 1)
          for layout in ((1, 2) if weights.fcw_split(R) else (1,))]
# k_pack_conv at the wider shapes: hidden 192 pads the output channels to 256 (cin_pad 192), 256 and 512 pad nothing
_BYTES += [(8, hidden, 1, weights.default_fc_layout(8)) for hidden in (192, 256, 512)]


@pytest.mark.parametrize("R,hidden,dtype,layout", _BYTES)
def test_pack_bytes(R, hidden, dtype, layout):
    """R = 9 and 11 pad both axes of the Linear and leave an RR tail of 1 and 9 positions; odd R + 1 slot strides"""
    eng = _engine(R, dtype)
    wc.case_bytes(eng, R, 1, hidden, dtype, layout)
    eng.close()


def test_pack_bytes_at_the_shape_users_run():
    """R = 14, hidden 128, fp16, layout 2: 2.2 GB in, 1.1 GB out, an RR tail of 4 positions, 18 all-zero row tiles.  Most
    of this test's time is the host reference export."""
    eng = _engine(14, 1)
    wc.case_bytes(eng, 14, 1, 128, 1, 2)
    eng.close()


@pytest.mark.parametrize("dtype", [0, 1])
def test_pack_follows_the_f32_spec_where_the_host_sqrt_does_not(dtype, monkeypatch):
    """unshifted variances, some planted where torch's CPU sqrt is one unit off: pack == numpy op-by-op fold (the
    hardware divide, square root and conversions this time)"""
    eng = _engine(9, dtype)
    wc.case_spec_bytes(eng, 9, 1, 128, dtype, 2, monkeypatch)
    eng.close()


# ---- 2. forward ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("R,hidden,kernel", [(14, 128, "k_towerc"), (8, 128, "k_towerw"), (8, 256, "k_towerw"), (8, 64, "k_conv3x3"),
                                             (8, 192, "k_conv3x3"), (8, 512, "k_conv3x3")])
def test_forward_equals_the_host_loaded_engine(R, hidden, kernel):
    """engine X loaded through the host blob, engine Y through fpc_load_weights_device (a FIRST load: it allocates):
    bit-identical logits and values, once per tower path"""
    m = wc.model(R, 1, hidden)
    x = wc.encodings(R)
    ex = _host_loaded(R, 1, hidden, 1)
    assert _kernel(ex) == kernel
    want = wc.forward(ex, x)
    ex.close()
    ey = _engine(R, 1)
    ey.load_weights_device(m)
    assert _kernel(ey) == kernel
    wc.assert_same_forward(wc.forward(ey, x), want, "R=%d hidden=%d" % (R, hidden))
    ey.close()


# ---- 3. in place ---------------------------------------------------------------------------------------------------------
def test_in_place_reload_allocates_nothing_and_refreshes_every_derived_buffer():
    import torch
    R, hidden = 8, 128
    mods = {"A": wc.model(R, 1, hidden), "B": wc.model(R, 1, hidden, seed=1)}
    x = wc.encodings(R)
    want, want_legal = {}, {}
    for k, m in mods.items():
        e = _engine(R, 1)
        e.load_weights(weights.export_weights(m, 1))
        want[k] = wc.forward(e, x)
        want_legal[k] = wc.search_counts(e, R, legal=True)
        e.close()
    assert not np.array_equal(want["A"][0], want["B"][0])
    gpu = {k: copy.deepcopy(m).cuda() for k, m in mods.items()}      # the live modules: nothing is allocated by a load
    eng = _engine(R, 1)
    eng.load_weights(weights.export_weights(mods["A"], 1))
    wc.assert_same_forward(wc.forward(eng, x), want["A"], "host load A")
    free = []
    for k in ("B", "A", "B"):
        eng.load_weights_device(gpu[k])
        torch.cuda.synchronize()
        free.append(torch.cuda.mem_get_info()[0])
        wc.assert_same_forward(wc.forward(eng, x), want[k], "device load " + k)
    print("free bytes after loads 2, 3, 4:", free)
    assert free[0] == free[1] == free[2], free
    # the legal-only head keeps a row-major copy of the policy weights (made on first use): an in-place load refreshes it
    assert wc.search_counts(eng, R, legal=True) == want_legal["B"]
    torch.cuda.synchronize()
    free_legal = torch.cuda.mem_get_info()[0]
    eng.load_weights_device(gpu["A"])
    assert wc.search_counts(eng, R, legal=True) == want_legal["A"]
    assert want_legal["A"] != want_legal["B"]
    torch.cuda.synchronize()
    assert torch.cuda.mem_get_info()[0] == free_legal
    wc.assert_same_forward(wc.forward(eng, x), want["A"], "device load A with the legal head")
    eng.close()


# ---- 4. geometry change --------------------------------------------------------------------------------------------------
def test_geometry_change_reallocates():
    R = 8
    x = wc.encodings(R)
    eng = _engine(R, 1)
    eng.load_weights_device(wc.model(R, 2, 64))
    assert _kernel(eng) == "k_conv3x3"
    fresh = _engine(R, 1)
    fresh.load_weights(weights.export_weights(wc.model(R, 2, 64), 1))
    wc.assert_same_forward(wc.forward(eng, x), wc.forward(fresh, x), "2 blocks, hidden 64")
    fresh.close()
    eng.load_weights_device(wc.model(R, 1, 128))
    assert _kernel(eng) == "k_towerw"
    fresh = _host_loaded(R, 1, 128, 1)
    wc.assert_same_forward(wc.forward(eng, x), wc.forward(fresh, x), "1 block, hidden 128")
    fresh.close()
    eng.close()


# ---- 5. errors -----------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_loaded_network_as_it_was():
    R = 8
    m = wc.model(R, 1, 64)
    x = wc.encodings(R)
    eng = _host_loaded(R, 1, 64, 1)
    want = wc.forward(eng, x)
    for load in (False, True):
        for name, rc in wc.einval_cases(eng, m, load=load):
            assert rc == wc.EINVAL, (name, load, rc)
            wc.assert_same_forward(wc.forward(eng, x), want, name)
    m96 = wc.model(R, 1, 96)
    src, keep = wc.raw_src(eng, m96)
    assert eng.L.fpc_load_weights_device(eng.h, C.byref(src), 1) == wc.EWEIGHTS
    assert b"hidden must be a multiple of 64" in eng.L.fpc_last_error(eng.h)
    wc.assert_same_forward(wc.forward(eng, x), want, "hidden 96")
    ms = C.c_float()
    assert eng.L.fpc_weights_pack_ms(eng.h, C.byref(ms)) == -9          # FPC_ESTATE: no pack was timed
    eng.set_timing(True)
    eng.load_weights_device(m)
    assert eng.weights_pack_ms() > 0.0
    wc.assert_same_forward(wc.forward(eng, x), want, "reload")
    eng.close()


# ---- 6. drop-in ----------------------------------------------------------------------------------------------------------
def test_mcts_device_weights(monkeypatch):
    """args["device_weights"]: the module on the GPU is packed there -- export_weights is never called -- and the search
    equals the host path's; after an optimizer step the next search runs on the new weights"""
    import torch
    import dropin_cases as dc
    az = dc.setup("gpu", 8)
    from fen_parser import parse_board_args_from_fen
    from four_player_chess_board import FourPlayerChess
    from mcts import MCTS
    import net
    R, G, sims = 8, 4, 16
    torch.manual_seed(11)
    cpu_model = net.ResNet(FourPlayerChess, 1, 64, "cpu").eval()
    args = {"C": 3, "num_searches": sims, "pool_size": 10, "nn_dtype": 1}

    def games():
        return [FourPlayerChess(*parse_board_args_from_fen(FourPlayerChess.start_fen, R)) for _ in range(G)]

    def counts(roots):
        return [[[c.GetMoveMade().GetFlatIndex(), c.GetVisitCount()] for c in r.GetChildren()] for r in roots]

    def fresh_counts(m):
        e = _engine(R, 1)
        e.load_weights(export(m, 1))
        out = wc.search_counts(e, R, sims, G, roots=[g._b for g in games()])
        e.close()
        return out

    export = weights.export_weights
    want = counts(MCTS(FourPlayerChess, cpu_model, args).search(games()))
    assert want == fresh_counts(cpu_model)
    gpu_model = copy.deepcopy(cpu_model).cuda()

    def refuse(*a, **k):
        raise AssertionError("the host export ran although device_weights is set and the module lies on the GPU")
    monkeypatch.setattr(weights, "export_weights", refuse)
    mcts = MCTS(FourPlayerChess, gpu_model, dict(args, device_weights=True))
    assert counts(mcts.search(games())) == want
    # one optimizer step on the live module
    opt = torch.optim.Adam(gpu_model.parameters(), lr=1e-2)      # every parameter moves by about lr, whatever the gradient's scale
    gpu_model.train()
    pol, val = gpu_model(wc.encodings(R, 8))
    (pol.square().mean() + val.square().mean()).backward()
    opt.step()
    gpu_model.eval()
    # the train-mode forward left arbitrary floats in the running variances: where the host's sqrt is not the correctly
    # rounded one (weights_cases.host_exact_var) the host-loaded reference below would differ from the spec by an ulp
    with torch.no_grad():
        for mod in gpu_model.modules():
            if isinstance(mod, torch.nn.BatchNorm2d):
                mod.running_var.copy_(wc.host_exact_var(mod.running_var.cpu(), mod.eps))
    got = counts(mcts.search(games()))
    new_cpu = copy.deepcopy(gpu_model).cpu()
    assert got == fresh_counts(new_cpu)
    assert got != want
    # a module that is not on the engine's device takes the host path as before
    monkeypatch.setattr(weights, "export_weights", export)
    assert counts(MCTS(FourPlayerChess, new_cpu, dict(args, device_weights=True)).search(games())) == got
