"""tests/tower_probe.py proven able to fail, without a GPU: the comparators of test_tower_probe_gpu.py are fed the
reference's own output with one layer mutated the way a tap-loop rewrite goes wrong, and must flag every mutation in
both weight families; the fp32-order reference must pass; family A's input conditions hold for every GPU case, and its
value bound flags a misindexed value Linear on every board and width of the per-layer cases; the spliced weight blob is
the exported one.  The dense integer Linear of tests/test_linear_probe_gpu.py likewise: its blob
read back with numpy alone, its exactness condition for every GPU case, NO fragment product of its inputs dead, and five
faults of the Linear's own decomposition flagged."""
import copy

import numpy as np
import pytest
import torch

import tower_probe as tp
import weights

# (family, R, hidden, blocks, dtype): the shapes the mutations are tried on (14x14 has the 4-square tail tile)
SHAPES = [("A", 14, 128, 3, 1), ("A", 14, 128, 2, 0), ("B", 14, 128, 2, 1), ("B", 14, 128, 3, 0), ("B", 8, 128, 2, 1),
          # the per-layer path's own shapes: a width between the tower kernels' (three slabs of 64) on an odd pitch, where
          # family A draws its 7 nonzeros per output channel from 9 * 192 products, and the same width dense
          ("A", 9, 192, 3, 1), ("B", 8, 192, 2, 1)]


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


@pytest.mark.parametrize("case", [c for c in tp.CASES if c[5] == "A" and c[0] == "k_conv3x3" and not c[6]], ids=tp.case_id)
def test_family_a_value_bound_sees_a_misindexed_value_linear(case):
    """The value check of family A (bound: max(value floor, 2 x the CPU fp32 figure), as family B's) proven able to fail
    on every board and width of the per-layer cases: the value Linear read with rows and columns exchanged (q / R and
    q % R swapped), and read one square late (an off-by-one pitch), must both leave the bound."""
    kernel, R, hidden, blocks, dtype, family, knobs, rows = case
    p = tp.prepare(case)
    vw, vb = tp.value_vector(R)
    lim = max(p["value_floor"], 2.0 * p["cpu"]["value"])
    v = p["ref"]["vconv"]
    for name, bad in (("transposed", np.swapaxes(v, 2, 3)), ("one square late", np.roll(v.reshape(rows, 24, -1), 1, axis=2))):
        dv = float(np.abs(tp.value_of(bad, vw, vb) - p["ref_value"]["value"]).max())
        print("%s, value Linear %s: moves the value by %.3e, bound %.3e" % (tp.case_id(case), name, dv, lim))
        assert dv > lim, (name, dv, lim)                       # measured: 22 x the bound or more in every case


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


# ---------------------------------------------------------------------------------------------------------------------
# the dense integer Linear (tests/test_linear_probe_gpu.py)
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("R", [8, 9])
@pytest.mark.parametrize("layout", [2, 1])
def test_dense_linear_blob_round_trip(R, layout):
    """the exported "dense_int" Linear with the fragment order [k32][n-tile][lane = 16 q + c][8] and the NCHW -> NHWC input
    permutation undone by numpy: W itself, zeros in ALL padding (9x9 pads Np and Kp under both layouts), the bias --
    byte for byte"""
    W, bias = tp.dense_weights(R)
    A = W.shape[0]
    for dtype in (1, 0):
        t = tp.tail(R, dtype, layout, "dense_int")
        gw = 384 if layout == 2 else 256
        assert (t.Np, t.Kp) == ((A + gw - 1) // gw * gw, (A + 511) // 512 * 512)
        if R == 9:
            assert t.Np > A and t.Kp > A
        w, b = tp.decode_linear(t)
        assert np.array_equal(w[:A, :A], tp.engine_order(W, R).astype(np.float32))
        raw = np.frombuffer(t.bytes, np.uint16, t.Np * t.Kp).reshape(t.Kp // 32, t.Np // 16, 4, 16, 8).transpose(1, 3, 0, 2, 4).reshape(t.Np, t.Kp)
        assert not raw[A:].any() and not raw[:, A:].any()                      # padding: zero BITS, not just zero values
        assert b.tobytes() == np.concatenate([bias.astype(np.float32), np.zeros(t.Np - A, np.float32)]).tobytes()
        assert np.abs(bias).max() == 5 and np.abs(W).max() == 3


def test_dense_linear_scaled_tail_is_exact():
    """ "dense_scaled": W and bias times 2^-s survive the rounding to either operand type; the value Linear is zero"""
    R, s = 8, 9
    W, bias = tp.dense_weights(R)
    A = W.shape[0]
    for dtype in (1, 0):
        t = tp.tail(R, dtype, 2, "dense_scaled", s=s)
        w, b = tp.decode_linear(t)
        assert np.array_equal(w[:A, :A].astype(np.float64) * 2.0 ** s, tp.engine_order(W, R).astype(np.float64))
        assert np.array_equal(b[:A].astype(np.float64) * 2.0 ** s, bias.astype(np.float64))
        assert not np.frombuffer(t.bytes, np.uint8, offset=2 * t.Np * t.Kp + 4 * t.Np).any()     # value Linear and bias: 0


@pytest.mark.parametrize("key", sorted(set((c[0], c[1], max(c[3])) for c in tp.LINEAR_CASES)),
                         ids=lambda k: "%dx%d-%s-%d" % (k[0], k[0], tp.FMT[k[1]]["name"], k[2]))
def test_dense_linear_exactness_holds_for_every_gpu_case(key):
    """max_row sum|x| * max|w| + max|bias| < 2^24 (and family A's conditions, inside prepare) for every case of the GPU
    table: fp32 accumulation of these logits is exact in any order"""
    R, dtype, rows = key
    p = tp.prepare(tp.linear_case(R, dtype, rows))
    W, bias = tp.dense_weights(R)
    lhs = tp.linear_conditions(p["ref"]["policy"].reshape(rows, -1), W, bias)
    print("%dx%d %s %d rows: sum|x| max|w| + max|b| = %.0f = 2^%.2f" % (R, R, tp.FMT[dtype]["name"], rows, lhs, np.log2(lhs)))


@pytest.mark.parametrize("R,dtype", [(8, 1), (8, 0), (14, 1)], ids=["8x8-fp16", "8x8-bf16", "14x14-fp16"])
def test_no_fragment_product_of_the_dense_linear_is_dead(R, dtype):
    """What keeps the bit-for-bit test from hiding a failure: for the 256-row inputs EVERY (16-row tile, 16-column tile,
    32-deep k-step) contribution block X[16, 32] . W[16, 32]^T is nonzero somewhere -- the allowed share of dead triples
    is 0 -- so a fragment product dropped, doubled or put in the wrong place changes a logit.  The same for the row
    the 1-row forward runs, per (column tile, k-step)."""
    p = tp.prepare(tp.linear_case(R, dtype, 256))
    policy = p["ref"]["policy"]
    dead, total = tp.dead_fragment_products(policy, R)
    A = policy[0].size
    assert total == 16 * (A // 16) * ((A + 31) // 32)
    assert dead == 0, (dead, total)
    dead1, total1 = tp.dead_fragment_products(policy[tp.linear_rows(256, 1)], R, row_tiles=False)
    assert total1 == total // 16 and dead1 == 0, (dead1, total1)


@pytest.mark.parametrize("layout", [2, 1])
@pytest.mark.parametrize("dtype", [1, 0], ids=["fp16", "bf16"])
def test_every_linear_mutation_is_flagged(dtype, layout):
    """the reference Linear with one fault of the kernels' own decomposition, at 8x8 with 256 rows: check_exact must raise"""
    R = 8
    p = tp.prepare(tp.linear_case(R, dtype, 256))
    want = tp.dense_reference(p, R)
    tp.check_exact(want.astype(np.float32), want, "the reference itself")
    for name in tp.LINEAR_MUTATIONS:
        bad = tp.mutated_logits(p["ref"]["policy"], R, layout, name)
        with pytest.raises(AssertionError):
            tp.check_exact(bad.astype(np.float32), want, name)
