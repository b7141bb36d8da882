"""tests/tower_probe.py proven able to fail, without a GPU: the comparators of test_tower_probe_gpu.py are fed the
reference's own output with one layer mutated the way a tap-loop rewrite goes wrong, and must flag every mutation in
both weight families; the fp32-order reference must pass; family A's input conditions hold for every GPU case; the
spliced weight blob is the exported one."""
import copy

import numpy as np
import pytest
import torch

import tower_probe as tp
import weights

# (family, R, hidden, blocks, dtype): the shapes the mutations are tried on (14x14 has the 4-square tail tile)
SHAPES = [("A", 14, 128, 3, 1), ("A", 14, 128, 2, 0), ("B", 14, 128, 2, 1), ("B", 14, 128, 3, 0), ("B", 8, 128, 2, 1)]


def _case(family, R, hidden, blocks, dtype):
    return ("cpu", R, hidden, blocks, dtype, family, {}, 37)


@pytest.mark.parametrize("dtype", [1, 0], ids=["fp16", "bf16"])
def test_round16_is_the_operand_types_rounding(dtype):
    """round16 / quantum against torch's own conversion, on fp32 inputs (one rounding for both)"""
    g = torch.Generator().manual_seed(dtype)
    x = torch.cat([torch.randn(200000, generator=g) * s for s in (1e-6, 1e-2, 1.0, 300.0)] + [torch.tensor([0.0, 1.0, 0.5, 2047.0, 255.0])])
    want = x.to(tp.FMT[dtype]["torch"]).to(torch.float64).numpy()
    assert np.array_equal(tp.round16(x.to(torch.float64).numpy(), dtype), want)
    up = torch.nextafter(torch.from_numpy(want).to(tp.FMT[dtype]["torch"]).abs(), torch.tensor(float("inf"), dtype=tp.FMT[dtype]["torch"]))
    assert np.array_equal(tp.quantum(want, dtype), up.to(torch.float64).numpy() - np.abs(want))


@pytest.mark.parametrize("case", [c for c in tp.CASES if c[5] == "A"], ids=tp.case_id)
def test_family_a_conditions_hold_for_every_gpu_case(case):
    """from the reference alone: every layer <= 2047 (fp16) / 255 (bf16), >= 40 % of the tower nonzero, >= 32 distinct
    values -- asserted inside prepare()"""
    maxima, live, distinct = tp.prepare(case)["conditions"]
    print(tp.case_id(case), "layer maxima", maxima, "nonzero %.2f" % live, "distinct", distinct)


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%s-%dx%d-h%d-b%d-%s" % (s[0], s[1], s[1], s[2], s[3], tp.FMT[s[4]]["name"]))
def test_every_mutation_is_flagged_and_the_fp32_order_passes(shape):
    family, R, hidden, blocks, dtype = shape
    p = tp.prepare(_case(*shape))
    layers, ref = tp.conv_layers(p["net"], dtype), p["ref"]
    other = tp.forward(layers, p["x"], dtype, "f32seq4")         # an fp32 order (one of those the CPU figure is drawn from)
    if family == "A":
        for k in ("tower", "policy"):
            tp.check_exact(other[k].astype(np.float32), ref[k], k)
    else:
        for k in ("tower", "policy"):
            tp.check_bounded(other[k], ref[k], p["cpu"][k], dtype, "fp32 order, " + k)
    for name in tp.MUTATIONS:
        for layer in (2, 2 * blocks):                            # conv2 of the first and of the last block
            bad = tp.forward(layers, p["x"], dtype, "f64", (name, layer))
            with pytest.raises(AssertionError):
                if family == "A":
                    tp.check_exact(bad["tower"].astype(np.float32), ref["tower"], name)
                else:
                    tp.check_bounded(bad["tower"], ref["tower"], p["cpu"]["tower"], dtype, "%s in layer %d" % (name, layer))
    # A mutation confined to a SMALL element.  Family A sees any: the smallest live activation (1) of the last layer
    # zeroed breaks the bit identity.  Family B measures distances in roundings at max(|element|, rms of the layer), so
    # what it resolves is bound x (one rounding at the rms) in absolute terms: the smallest activation above that,
    # zeroed, must be flagged -- and the resolution must stay below 1 % of the rms (below it family A is what holds a
    # kernel: the same tiles, masks and tail elements, bit for bit).
    if family == "A":
        bad = tp.forward(layers, p["x"], dtype, "f64", ("zero_small", 2 * blocks, 1.0))
        assert np.abs(bad["tower"] - ref["tower"]).max() == 1.0
        with pytest.raises(AssertionError):
            tp.check_exact(bad["tower"].astype(np.float32), ref["tower"], "smallest live element zeroed")
    else:
        rms = float(np.sqrt((ref["tower"] ** 2).mean()))
        q = float(tp.quantum(rms, dtype))
        resolution = tp.bound_of(p["cpu"]["tower"])[0] * q
        print("family B resolves %.2e absolute = %.2f %% of the tower's rms %.3f" % (resolution, 100 * resolution / rms, rms))
        assert resolution <= (0.01 if dtype == 1 else 0.08) * rms      # 4 roundings of 2^-11 / 2^-8 relative, with margin
        bad = tp.forward(layers, p["x"], dtype, "f64", ("zero_small", 2 * blocks, resolution + q))
        moved = float(np.abs(bad["tower"] - ref["tower"]).max())
        assert resolution < moved <= resolution + 3 * q, (moved, resolution, q)
        with pytest.raises(AssertionError):
            tp.check_bounded(bad["tower"], ref["tower"], p["cpu"]["tower"], dtype, "small element zeroed")
    # the policy conv is a layer like the others: its probe must see a mutation of it
    bad = tp.forward(layers, p["x"], dtype, "f64", ("wrap_row", len(layers) - 2))
    with pytest.raises(AssertionError):
        if family == "A":
            tp.check_exact(bad["policy"].astype(np.float32), ref["policy"], "policy conv")
        else:
            tp.check_bounded(bad["policy"], ref["policy"], p["cpu"]["policy"], dtype, "wrap_row in the policy conv")


def test_what_the_logit_level_bound_sees_of_each_mutation():
    """The record of the gap: ResNet(3,128) at 14x14 without any 16-bit rounding, 12 random inputs, each
    mutation in conv2 of block 1; the largest change of a logit behind a Linear with nn.Linear's own init
    (U(-1/sqrt(A), 1/sqrt(A)), A = 23 520; 256 of its rows stand for all), next to the suite's 1e-3 -- and the largest
    change of a tower element, which is what the probe heads see."""
    R, hidden, blocks = 14, 128, 3
    m = tp.dense_net(R, blocks, hidden, seed=0)
    layers = tp.conv_layers(m, None)
    x = tp.probe_inputs(R, 12, seed=5, density=0.5)
    A = (8 * R + 8) * R * R
    fc = (torch.rand(256, A, generator=torch.Generator().manual_seed(1), dtype=torch.float64) * 2 - 1).numpy() / A ** 0.5
    base = tp.forward(layers, x, None)
    seen, q = {}, float(tp.quantum(np.sqrt((base["tower"] ** 2).mean()), 1))     # an fp16 rounding at the tower's rms
    typical = float(np.sqrt((base["acts"][2] ** 2).mean()))       # "zero_typical": the activation nearest above the layer's rms
    for name in ("zero_typical",) + tp.MUTATIONS:
        bad = tp.forward(layers, x, None, "f64", ("zero_small", 2, typical) if name == "zero_typical" else (name, 2))
        dl = float(np.abs((bad["policy"] - base["policy"]).reshape(12, -1) @ fc.T).max())
        dt = float(np.abs(bad["tower"] - base["tower"]).max())
        seen[name] = (dt, dl)
        print("%-18s largest change of a tower element %.2e, of a logit %.2e: the 1e-3 logit bound %s" % (
            name, dt, dl, "sees it" if dl > 1e-3 else "is blind to it"))
    # every mutation moves a tower element by hundreds of roundings; the single-row, single-tap one moves no logit by
    # more than about twice the logit bound (and a quarter of the bound is already used by the fp16 path itself)
    assert all(dt > 100 * q for dt, _ in seen.values())
    assert seen["zero_typical"][1] < 1e-3                        # blind to an activation of typical size zeroed
    assert seen["zero_element"][1] > 1e-3                        # sees the largest activation of a channel zeroed
    assert 1e-3 < seen["wrap_row"][1] < 3e-3                     # marginal: within 3 x the bound
    for name in ("swap_slices", "drop_bias16", "no_residual_tail"):
        assert seen[name][1] > 5e-3, name                        # seen


@pytest.mark.parametrize("dtype,layout", [(1, 2), (0, 1)])
def test_spliced_blob_is_the_exported_blob(dtype, layout):
    """splice(): conv sections of the stub-geometry network in front of the cached Linear sections == export_weights of
    the whole 8x8 network, byte for byte"""
    R, hidden, blocks = 8, 128, 2
    stub = tp.dense_net(R, blocks, hidden, seed=4)
    t = tp.tail(R, dtype, layout, "perm")
    torch.manual_seed(0)
    full = tp.net.ResNet(tp.Spec(R), blocks, hidden, "cpu").eval()
    for (c, bn), (c2, bn2) in zip(tp._convs(stub), tp._convs(full)):
        c2.load_state_dict(c.state_dict())
        bn2.load_state_dict(bn.state_dict())
    perm, scale = tp.permutation(R)
    vw, vb = tp.value_vector(R)
    with torch.no_grad():
        fc, vfc = full.policyHead[4], full.valueHead[4]
        fc.weight.zero_()
        fc.bias.zero_()
        fc.weight[torch.arange(len(perm)), torch.from_numpy(perm)] = torch.from_numpy(scale)
        vfc.weight.copy_(torch.from_numpy(vw).view(1, -1))
        vfc.bias.fill_(float(vb))
    assert tp.splice(stub, t) == weights.export_weights(full, dtype, fc_layout=layout)
    # and the probe conv is what it says: channel j of the policy conv copies tower channel c0 + j
    pm = copy.deepcopy(stub)
    width = tp.set_tower_probe(pm, 56)
    out = tp.forward(tp.conv_layers(pm, dtype), tp.probe_inputs(R, 9), dtype)
    assert width == 72 and np.array_equal(out["policy"], out["tower"][:, 56:128])
