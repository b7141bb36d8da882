"""k_towerc's tap-specialised loop (csrc/fpc_tower.h, TU: three dy iterations of an unrolled dx triple, ring slot / DMA
destination / column masks compile-time) against the forms it must reproduce: the rolled loop it replaces
(FPC_TOWER_TAPLOOP=0), the bordered grid (FPC_TOWER_COMPACT=0) and one wave per SIMD (FPC_TOWER_WAVES=4)."""
import numpy as np
import pytest

from fpc_testlib import make_engine

pytestmark = pytest.mark.gpu

R, INV = 14, 3


class Spec:
    """the gameType attributes net.ResNet reads"""
    def __init__(self, R):
        self.R = R
        self.num_state_channels = 24
        self.num_action_channels = 8 * R + 8
        self.action_space_size = self.num_action_channels * R * R
        self.state_space_size = 24 * R * R

    def nRows(self):
        return self.R

    def nCols(self):
        return self.R


def _model(blocks, seed):
    import torch
    import net
    torch.manual_seed(seed)
    m = net.ResNet(Spec(R), blocks, 128, "cpu")
    g = torch.Generator().manual_seed(seed + 1)
    for mod in m.modules():                      # non-trivial BN statistics so that the fold is exercised
        if isinstance(mod, torch.nn.BatchNorm2d):
            mod.running_mean.copy_(torch.randn(mod.num_features, generator=g) * 0.1)
            mod.running_var.copy_(torch.rand(mod.num_features, generator=g) * 0.5 + 0.75)
            mod.weight.data.copy_(torch.rand(mod.num_features, generator=g) * 0.5 + 0.75)
            mod.bias.data.copy_(torch.randn(mod.num_features, generator=g) * 0.1)
    return m.eval()


# (developer knobs, what must match the product form): the product form is run first, with no knob but the opt-in
FORMS = [
    ({"FPC_TOWER_TAPLOOP": "0"}, "bits"),        # the rolled loop: logits AND values bit for bit
    ({"FPC_TOWER_COMPACT": "0"}, "logits"),      # bordered grid: the value head sums the same terms over other lanes
    ({"FPC_TOWER_WAVES": "4"}, "logits"),        # one wave per SIMD on the bordered grid: likewise
]


@pytest.mark.parametrize("dtype", [1, 0], ids=["fp16", "bf16"])
@pytest.mark.parametrize("blocks,G", [(10, 300), (2, 48)], ids=["10blocks-300rows", "2blocks-48rows"])
def test_taploop_reproduces_the_other_tower_forms(blocks, G, dtype, monkeypatch):
    """300 rows: more than one 256-row tile of the policy Linear and more games than CUs; 48: fewer games than CUs.
    Logits bit for bit against all three forms; values bit for bit against the rolled loop and within 2e-6 (the bound of
    test_tower_wave_forms_give_identical_bits: the same f32 terms in another summation order) against the other two."""
    import torch
    import weights
    m = _model(blocks, seed=21 + blocks)
    w = weights.export_weights(m, dtype)
    x = (torch.rand(G, 24, R, R, generator=torch.Generator().manual_seed(blocks * 100 + G)) < 0.1).float().cuda()
    monkeypatch.setenv("FPC_DEV_KNOBS", "1")

    def run(knobs):
        for k, v in knobs.items():
            monkeypatch.setenv(k, v)
        eng = make_engine("gpu", R, INV, max_games=G, max_sims=4, nn_dtype=dtype)
        eng.load_weights(w)
        assert (eng.L.fpc_nn_kernel(eng.h) or b"").decode() == ("k_towerc" if "FPC_TOWER_TAPLOOP" in knobs or not knobs else "k_tower")
        lg = torch.empty(G, eng.A, device="cuda")
        va = torch.empty(G, device="cuda")
        for _ in range(3):
            eng.nn_forward(x.data_ptr(), G, lg.data_ptr(), va.data_ptr())
        torch.cuda.synchronize()
        out = lg.cpu().numpy().copy(), va.cpu().numpy().copy()
        eng.close()
        for k in knobs:
            monkeypatch.delenv(k)
        return out

    new_l, new_v = run({})
    assert np.abs(new_l).mean() > 1e-3 and np.isfinite(new_l).all() and np.isfinite(new_v).all()
    for knobs, what in FORMS:
        ref_l, ref_v = run(knobs)
        assert np.array_equal(new_l.view(np.uint32), ref_l.view(np.uint32)), (knobs, blocks, G, dtype)
        if what == "bits":
            assert np.array_equal(new_v.view(np.uint32), ref_v.view(np.uint32)), (knobs, blocks, G, dtype)
        else:
            dv = float(np.abs(new_v - ref_v).max())
            print("values vs %s: max |diff| %.3g" % (knobs, dv))
            assert dv < 2e-6, (knobs, blocks, G, dtype)
