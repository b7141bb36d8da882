"""Probe heads: networks whose policy head turns the dense logits fpc_nn_forward returns into a window on the
residual tower, and the float64 reference those logits are held against.

* tower probe: the policy conv copies `width` tower channels from offset c0 (centre tap 1, everything else 0, BN an exact
  identity) and the policy Linear is the identity, so logits[n, ch*R*R + pos] IS the 16-bit tower activation
  [n, c0+ch, pos]: every other product of the Linear is an exact zero and no summation order can matter.
* permutation Linear: the identity replaced by a permutation matrix with entries +-2^k, still exact.
* policy-conv probe: identity Linear behind a policy conv that carries real weights (family A or B).
* family A (integer_net): 0/1 inputs, sparse conv weights in {-1, 0, +1}, integer biases, identity BNs -- every
  activation an integer below 2^11 (fp16) / 2^8 (bf16): f32 accumulation is exact in any order, the kernel must equal
  the reference BIT FOR BIT.
* family B (dense_net): Kaiming weights and randomised BN statistics; the bound is measured per case from the noise one
  more f32 summation order makes on the CPU (noise_figures / check_bounded).

A ResNet at 14x14 owns a 23 520 x 23 520 Linear (2.2 GB in fp32).  The networks here are therefore built on a stub
geometry (convolutions of the real shape, Linears of a 1 x 1 board), exported with weights.export_weights, and their
conv sections spliced in front of the Linear sections of ONE exported identity / permutation Linear per (board, operand
type, layout): splice() -- held bit for bit against a plain export_weights of the whole network by the CPU self-test."""
import struct

import numpy as np
import torch
import torch.nn.functional as TF

import net
import weights

# operand types by the engine's nn_dtype: significand bits (implicit one included) and the exponent of the smallest quantum
FMT = {1: {"name": "fp16", "p": 11, "qmin": -24, "torch": torch.float16, "int_max": 2047},
       0: {"name": "bf16", "p": 8, "qmin": -133, "torch": torch.bfloat16, "int_max": 255}}


class Spec:
    """the gameType attributes net.ResNet reads"""
    def __init__(self, R, linear_side=None):
        s = R if linear_side is None else linear_side
        self.R, self._s = R, s
        self.num_state_channels = 24
        self.num_action_channels = 8 * R + 8
        self.action_space_size = self.num_action_channels * s * s
        self.state_space_size = 24 * s * s

    def nRows(self):
        return self._s

    def nCols(self):
        return self._s


def stub_spec(R):
    """convolutions of an R x R board's network, Linears of a 1 x 1 board"""
    return Spec(R, 1)


# ---------------------------------------------------------------------------------------------------------------------
# the number formats
# ---------------------------------------------------------------------------------------------------------------------
def quantum(x, dtype):
    """spacing of the operand type's values at |x| (float64 in, float64 out): one rounding of the type at that magnitude"""
    f = FMT[dtype]
    x = np.abs(np.asarray(x, np.float64))
    _, e = np.frexp(x)
    e = np.where(x == 0, -100000, e)              # frexp(0) has exponent 0: zero sits on the finest grid
    return np.ldexp(1.0, np.maximum(e - f["p"], f["qmin"]))


def round16(x, dtype):
    """float64 -> the nearest value of the operand type (ties to even), ONE rounding; returned as float64"""
    x = np.asarray(x, np.float64)
    q = quantum(x, dtype)
    return np.rint(x / q) * q


# ---------------------------------------------------------------------------------------------------------------------
# networks
# ---------------------------------------------------------------------------------------------------------------------
def _convs(m):
    """(conv, bn) in the blob's order: stem, c1/c2 per block, policy conv, value conv"""
    out = [(m.startBlock[0], m.startBlock[1])]
    for b in m.backBone:
        out += [(b.conv1, b.bn1), (b.conv2, b.bn2)]
    return out + [(m.policyHead[0], m.policyHead[1]), (m.valueHead[0], m.valueHead[1])]


def identity_bn(bn):
    """an EXACT identity: eps = 0, unit variance, zero mean, weight 1, bias 0 (the fold multiplies by 1/sqrt(1) = 1)"""
    bn.eps = 0.0
    with torch.no_grad():
        bn.running_var.fill_(1.0)
        bn.running_mean.zero_()
        bn.weight.fill_(1.0)
        bn.bias.zero_()


def assert_fold_is_identity(conv, bn):
    w, b = weights._fold(conv, bn)
    assert torch.equal(w.view(torch.int32), conv.weight.detach().view(torch.int32))
    assert torch.equal(b.view(torch.int32), conv.bias.detach().view(torch.int32))


def dense_net(R, blocks, hidden, seed=0):
    """family B: Kaiming conv init and randomised BN statistics, like _model() of test_nn_gpu.py"""
    torch.manual_seed(seed)
    m = net.ResNet(stub_spec(R), blocks, hidden, "cpu")
    g = torch.Generator().manual_seed(seed + 1)
    with torch.no_grad():
        for mod in m.modules():
            if isinstance(mod, torch.nn.BatchNorm2d):
                mod.running_mean.copy_(torch.randn(mod.num_features, generator=g) * 0.1)
                mod.running_var.copy_(torch.rand(mod.num_features, generator=g) * 0.5 + 0.75)
                mod.weight.copy_(torch.rand(mod.num_features, generator=g) * 0.5 + 0.75)
                mod.bias.copy_(torch.randn(mod.num_features, generator=g) * 0.1)
    return m.eval()


def _sparse_int_conv(conv, bn, pos, neg, cin_live, bias_lo, bias_hi, rng):
    cout, cin = conv.weight.shape[:2]
    w = np.zeros((cout, cin * 9), np.float32)
    for co in range(cout):
        idx = rng.choice(cin_live * 9, size=pos + neg, replace=False)
        w[co, idx[:pos]] = 1.0
        w[co, idx[pos:]] = -1.0
    with torch.no_grad():
        # (cin, tap) drawn jointly: index = ci * 9 + tap
        conv.weight.copy_(torch.from_numpy(w).view(cout, cin, 3, 3))
        conv.bias.copy_(torch.from_numpy(rng.integers(bias_lo, bias_hi + 1, size=cout).astype(np.float32)))
    identity_bn(bn)
    assert_fold_is_identity(conv, bn)


def integer_net(R, blocks, hidden, seed=0, stem=(6, 2), res=(3, 4), head=(3, 4), bias=(-1, 1)):
    """family A: every conv weight in {-1, 0, +1} with (positive, negative) nonzeros per output channel at random
    (tap, cin), integer biases in [bias[0], bias[1]], every BN an exact identity"""
    torch.manual_seed(seed)
    m = net.ResNet(stub_spec(R), blocks, hidden, "cpu")
    rng = np.random.default_rng(seed + 1000)
    cb = _convs(m)
    _sparse_int_conv(cb[0][0], cb[0][1], stem[0], stem[1], 24, bias[0], bias[1], rng)
    for conv, bn in cb[1:-2]:
        _sparse_int_conv(conv, bn, res[0], res[1], hidden, bias[0], bias[1], rng)
    for conv, bn in cb[-2:]:
        _sparse_int_conv(conv, bn, head[0], head[1], hidden, bias[0], bias[1], rng)
    return m.eval()


def probe_offsets(R, hidden):
    """channel offsets c0 of the tower probes that together see every tower channel: 0, hidden - width, and the middle
    ones a tower wider than two windows needs"""
    width = min(8 * R + 8, hidden)
    offs = list(range(0, hidden - width, width)) + [hidden - width]
    return offs, width


def set_tower_probe(m, c0):
    """overwrite the policy conv + BN of m: output channel j copies tower channel c0 + j (centre tap); returns the width"""
    conv, bn = m.policyHead[0], m.policyHead[1]
    a_ch, hidden = conv.weight.shape[:2]
    width = min(a_ch, hidden - c0)
    with torch.no_grad():
        conv.weight.zero_()
        conv.bias.zero_()
        for j in range(width):
            conv.weight[j, c0 + j, 1, 1] = 1.0
    identity_bn(bn)
    assert_fold_is_identity(conv, bn)
    return width


def probe_inputs(R, n, seed=0, density=0.25):
    """0/1 planes [n, 24, R, R]: row 0 all ones (every border tap live at once), rows 1..8 single-square impulses in the
    four corners and on the four edges, the rest random with the given density"""
    rng = np.random.default_rng(seed)
    x = (rng.random((n, 24, R, R)) < density).astype(np.float32)
    h = R // 2
    squares = [(0, 0), (0, R - 1), (R - 1, 0), (R - 1, R - 1), (0, h), (R - 1, h), (h, 0), (h, R - 1)]
    k = min(n, 1 + len(squares))
    x[:k] = 0.0
    x[0] = 1.0
    for i, (r, c) in enumerate(squares[: k - 1]):
        x[1 + i, :, r, c] = 1.0
    return x


# ---------------------------------------------------------------------------------------------------------------------
# the reference: DESIGN.md 5.2 -- 16-bit operands, bias + sum (+ residual), ReLU, ONE rounding to 16 bits per layer
# ---------------------------------------------------------------------------------------------------------------------
def conv_layers(m, dtype):
    """[(w, b)] in blob order: w = the folded weights rounded to the operand type as weights.export_weights rounds them
    (float64 tensors holding 16-bit values), b = the folded f32 bias as float64.  The fold itself is weights._fold, the
    export's own: that it equals the torch model's conv + BN is held by the tests against the torch model
    (test_nn_gpu.py, test_net_gpu.py), not here -- these tests hold what the kernels do with the exported operands."""
    out = []
    for conv, bn in _convs(m):
        w, b = weights._fold(conv, bn)
        w = w if dtype is None else w.to(FMT[dtype]["torch"])     # None: unrounded (the fp32 network's stand-in)
        out.append((w.to(torch.float64), b.to(torch.float32).to(torch.float64)))
    return out


MUTATIONS = ("zero_element", "wrap_row", "swap_slices", "drop_bias16", "no_residual_tail")

# The fp32 summation orders of the CPU figure besides torch's fused conv ("f32"): (tap order, input channels per addition,
# accumulator pre-loaded with bias + residual | both added in the epilogue).  "f32seq" is the tower kernels' order (one
# MFMA k-step of 16 channels per addition), "f32seq4" k_conv3x3's with 4 channels per addition (how an MFMA adds the 16
# products of a k-step to the accumulator is not specified; 4 values are the smallest per-lane operand of its 16-bit
# forms).  "f32p0".."f32p4" permute the taps (numpy default_rng(i)) and use 8 / 1 / 2 / 4 / 8 channels per addition.
ORDERS = {"f32seq": (tuple(range(9)), 16, True), "f32seq4": (tuple(range(9)), 4, False)}
for _i, (_step, _bf) in enumerate(((8, True), (1, False), (2, True), (4, True), (8, False))):
    ORDERS["f32p%d" % _i] = (tuple(int(t) for t in np.random.default_rng(_i).permutation(9)), _step, _bf)
BASE_ORDERS = ("f32", "f32seq", "f32seq4")
SHALLOW_ORDERS = BASE_ORDERS + tuple("f32p%d" % i for i in range(5))     # networks of at most 3 blocks


def _layer(x, w, b, res, dtype, acc, mut):
    """one conv layer on float64 tensors holding 16-bit values; acc: "f64" | "f32" (torch's fused fp32 conv) | a key of
    ORDERS | "f32taps" (fp32, nine fused 1x1 convs added tap after tap; carries the mutations in fp32).
    mut: None or a mutation name, applied to this layer."""
    R = x.shape[-1]
    if mut == "swap_slices":                      # two 8-channel input slices of one tap swapped
        w = w.clone()
        w[:, 0:8, 1, 2], w[:, 8:16, 1, 2] = w[:, 8:16, 1, 2].clone(), w[:, 0:8, 1, 2].clone()
    if mut == "drop_bias16":                      # the bias of 16 output channels dropped
        b = b.clone()
        b[16:32] = 0.0
    if acc == "f64":
        y = TF.conv2d(x, w, padding=1)
    elif acc == "f32":
        y = TF.conv2d(x.float(), w.float(), padding=1)
    elif acc in ORDERS:
        # ONE fp32 accumulator per output, fed tap after tap and group of input channels after group in sequence
        taps, step, bias_first = ORDERS[acc]
        n, cin = x.shape[:2]
        xp = TF.pad(x.float(), (1, 1, 1, 1))
        if bias_first:
            y = b.float().view(1, 1, 1, -1).expand(n, R, R, -1).reshape(n * R * R, -1).clone()
            if res is not None:
                y = y + res.float().permute(0, 2, 3, 1).reshape(n * R * R, -1)
        else:
            y = torch.zeros(n * R * R, w.shape[0])
        for t in taps:
            ky, kx = divmod(t, 3)
            if step == 16:                        # does not divide the stem's 24 planes: 16, then 8
                groups = [(c, min(c + 16, cin)) for c in range(0, cin, 16)]
                xs = xp[:, :, ky:ky + R, kx:kx + R].permute(0, 2, 3, 1).reshape(n * R * R, cin)
                for c0, c1 in groups:
                    y = y + xs[:, c0:c1] @ w[:, c0:c1, ky, kx].float().t()
            else:                                 # the partial sums of all groups of one tap in one bmm, added one by one
                xg = xp[:, :, ky:ky + R, kx:kx + R].reshape(n, cin // step, step, R * R).permute(1, 0, 3, 2).reshape(cin // step, n * R * R, step)
                part = torch.bmm(xg, w[:, :, ky, kx].float().view(-1, cin // step, step).permute(1, 2, 0).contiguous())
                for g in range(cin // step):
                    y += part[g]
        y = y.view(n, R, R, -1).permute(0, 3, 1, 2)
        if not bias_first:
            y = y + b.float().view(1, -1, 1, 1)
            if res is not None:
                y = y + res.float()
        assert mut is None
        y = torch.relu(y).double()
        return y if dtype is None else torch.from_numpy(round16(y.numpy(), dtype))
    else:
        xp = TF.pad(x.float(), (1, 1, 1, 1))
        y = None
        for ky in range(3):
            for kx in range(3):
                t = TF.conv2d(xp[:, :, ky:ky + R, kx:kx + R], w[:, :, ky:ky + 1, kx:kx + 1].float())
                y = t if y is None else y + t
    if mut == "wrap_row":                         # row R // 2: the right-edge tap reads the next row's first column
        r = R // 2
        for ky in range(3):
            if 0 <= r + ky < R:
                y[:, :, r, R - 1] += (x[:, :, r + ky, 0].to(y.dtype) @ w[:, :, ky, 2].to(y.dtype).t())
    y = y + b.to(y.dtype).view(1, -1, 1, 1)
    if res is not None:
        rr = res.to(y.dtype)
        if mut == "no_residual_tail":             # the residual omitted on the last 4 squares
            rr = rr.clone().flatten(2)
            rr[:, :, -4:] = 0.0
            rr = rr.view(res.shape)
        y = y + rr
    y = torch.relu(y).double()
    if dtype is not None:                         # None: no rounding at all (the fp32 network's stand-in)
        y = torch.from_numpy(round16(y.numpy(), dtype))
    if isinstance(mut, tuple):                    # ("zero_small", t): the smallest activation >= t forced to 0
        flat = y.flatten()
        flat[int(torch.argmin(torch.where(flat >= mut[1], flat, torch.full_like(flat, float("inf")))))] = 0.0
        y = flat.view(y.shape)
    if mut == "zero_element":                     # one live activation forced to 0
        c = 77 % y.shape[1]                       # channel 77, at the input and square where it is largest
        n, r, col = np.unravel_index(int(torch.argmax(y[:, c])), (y.shape[0], R, R))
        assert y[n, c, r, col] > 0
        y[n, c, r, col] = 0.0
    return y


def forward(layers, x, dtype, acc="f64", mutation=None):
    """layers: conv_layers(m, dtype); x: 0/1 planes [n, 24, R, R].  mutation: (name, layer index into layers), or
    ("zero_small", layer index, threshold), or None.
    Returns {"acts": every tower layer's output, "tower", "policy", "vconv"} as float64 numpy arrays of 16-bit values,
    and "vconv_unrounded": the value conv's output before its rounding."""
    x = torch.from_numpy(np.asarray(x, np.float64))
    nb = (len(layers) - 3) // 2

    def mut(i):
        if mutation is None or mutation[1] != i:
            return None
        return mutation[0] if len(mutation) == 2 else (mutation[0], mutation[2])

    with torch.no_grad():
        acts = [_layer(x, layers[0][0], layers[0][1], None, dtype, acc, mut(0))]
        for i in range(nb):
            t = _layer(acts[-1], layers[1 + 2 * i][0], layers[1 + 2 * i][1], None, dtype, acc, mut(1 + 2 * i))
            acts.append(t)
            acts.append(_layer(t, layers[2 + 2 * i][0], layers[2 + 2 * i][1], acts[-2], dtype, acc, mut(2 + 2 * i)))
        tower = acts[-1]
        policy = _layer(tower, layers[-2][0], layers[-2][1], None, dtype, acc, mut(len(layers) - 2))
        vconv = _layer(tower, layers[-1][0], layers[-1][1], None, dtype, acc, mut(len(layers) - 1))
        # the switch of DESIGN.md 5.2: the tower kernels feed the value Linear from the fp32 accumulators, the value
        # conv's output is never rounded to 16 bits there; the per-layer path (k_conv3x3 -> k_value_tail) rounds it
        vraw = _layer(tower, layers[-1][0], layers[-1][1], None, None, acc, mut(len(layers) - 1))
    return {"acts": [a.numpy() for a in acts], "tower": tower.numpy(), "policy": policy.numpy(), "vconv": vconv.numpy(),
            "vconv_unrounded": vraw.numpy()}


def value_of(vconv, vw, vb, acc="f64"):
    """tanh(Linear(Flatten(vconv))): vconv [n, 24, R, R] float64, vw the value Linear's f32 weights [24 * R * R]"""
    flat = vconv.reshape(vconv.shape[0], -1)
    if acc == "f64":
        return np.tanh(flat @ vw.astype(np.float64) + float(vb))
    return np.tanh((flat.astype(np.float32) @ vw.astype(np.float32) + np.float32(vb)).astype(np.float32)).astype(np.float64)


def integer_conditions(ref, dtype):
    """family A's input conditions, from the reference alone: every layer's largest activation (the head convs included)
    within the operand type's exact integers, >= 40 % of the final tower activations nonzero, >= 32 distinct values"""
    lim = FMT[dtype]["int_max"]
    maxima = [float(a.max()) for a in ref["acts"]] + [float(ref["policy"].max()), float(ref["vconv"].max())]
    for a in ref["acts"] + [ref["policy"], ref["vconv"]]:
        assert np.array_equal(a, np.rint(a))
    t = ref["tower"]
    live, distinct = float((t != 0).mean()), len(np.unique(t))
    assert max(maxima) <= lim, ("activation beyond the exact integers of %s" % FMT[dtype]["name"], maxima)
    assert live >= 0.40, live
    assert distinct >= 32, distinct
    return maxima, live, distinct


# ---------------------------------------------------------------------------------------------------------------------
# comparators
# ---------------------------------------------------------------------------------------------------------------------
def check_exact(got, ref, what=""):
    """got: float32 from the engine; ref: float64 holding 16-bit values.  Bit for bit."""
    got = np.ascontiguousarray(got, np.float32)
    want = np.ascontiguousarray(ref + 0.0, np.float32)           # -0.0 + 0.0 = +0.0: the kernels' ReLU gives +0
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = got.view(np.uint32) != want.view(np.uint32)
    if bad.any():
        idx = np.argwhere(bad)
        raise AssertionError("%s: %d of %d elements differ; first at %s: got %r, want %r" % (
            what, int(bad.sum()), bad.size, idx[0].tolist(), float(got[tuple(idx[0])]), float(want[tuple(idx[0])])))


def noise_figures(a, ref, dtype):
    """(largest distance, share of elements more than one rounding away) of a from the float64-accumulated reference,
    in roundings of the operand type at the reference's magnitude: the quantum at max(|ref element|, rms of ref).
    The floor is the scale of the terms an element is summed from: an output that cancels to 1e-5 still carries the
    error of operands of magnitude rms, and measured in ITS quanta (6e-8 in fp16) one flipped rounding upstream is
    hundreds of "roundings" -- a maximum over 10^6 such elements is a lottery between any two summation orders (measured:
    46 960 against 22 430 for two fp32 orders of one bf16 network) and would hide a zeroed activation."""
    ref = np.asarray(ref, np.float64)
    d = np.abs(np.asarray(a, np.float64) - ref) / quantum(np.maximum(np.abs(ref), np.sqrt((ref * ref).mean())), dtype)
    return float(d.max()), float((d > 1.0).mean())


def bound_of(cpu_fig):
    """largest distance <= max(2 roundings, 2 x the CPU figure of the same case); share of elements more
    than one rounding away <= 2 x the CPU share"""
    return max(2.0, 2.0 * cpu_fig[0]), 2.0 * cpu_fig[1]


def check_bounded(got, ref, cpu_fig, dtype, what=""):
    fig = noise_figures(got, ref, dtype)
    lim = bound_of(cpu_fig)
    print("%s: CPU f32 order %.2f roundings / share>1 %.3e; kernel %.2f roundings / share>1 %.3e; bounds %.2f / %.3e" % (
        what, cpu_fig[0], cpu_fig[1], fig[0], fig[1], lim[0], lim[1]))
    assert np.isfinite(np.asarray(got)).all(), what
    assert fig[0] <= lim[0], (what, "largest distance", fig[0], "bound", lim[0])
    assert fig[1] <= lim[1], (what, "share more than one rounding away", fig[1], "bound", lim[1])
    return fig


# ---------------------------------------------------------------------------------------------------------------------
# the Linears and the blob
# ---------------------------------------------------------------------------------------------------------------------
def head_len(F, nblocks):
    """bytes of header + conv sections of a weight blob (csrc/fpc_nn.h "weight blob"; every section a multiple of 64)"""
    Fp = (F + 127) // 128 * 128
    return 64 + 9 * Fp * 32 * 2 + Fp * 4 + 2 * nblocks * (9 * Fp * F * 2 + Fp * 4) + 2 * (9 * 128 * F * 2 + 128 * 4)


def value_vector(R, seed=99):
    """the value Linear's fixed random weights [24 * R * R] (NCHW flatten) and bias"""
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(24 * R * R, generator=g) / (24 * R * R) ** 0.5).numpy().astype(np.float32), np.float32(0.05)


def permutation(R, seed=7):
    """(perm, scale): row i of the permutation Linear holds scale[i] = +-2^k, k in -2..2, at column perm[i]"""
    A = (8 * R + 8) * R * R
    rng = np.random.default_rng(seed)
    return rng.permutation(A), (rng.choice([-1.0, 1.0], size=A) * np.exp2(rng.integers(-2, 3, size=A))).astype(np.float32)


def dense_weights(R):
    """the dense integer Linear: (W int8 [A, A] in {-3..3}, indexed [out, in] in the reference's NCHW input order, bias
    int64 [A] in {-5..5}), both from ONE generator.  Plain random draws, no structure: any two columns differ, so a
    swap of two of them shows.  Kept as int8 (553 MB at 14x14); of the large ones only the last stays cached."""
    if R not in _dense:
        if R >= 12:
            for k in [k for k in _dense if k >= 12]:
                _dense.pop(k)
        A = (8 * R + 8) * R * R
        rng = np.random.default_rng(1000 + R)
        W = rng.integers(-3, 4, size=(A, A), dtype=np.int8)
        _dense[R] = (W, rng.integers(-5, 6, size=A))
    return _dense[R]


_dense = {}
DENSE = ("dense_int", "dense_scaled")


class Tail:
    """the Linear sections of an exported blob and the header words that describe them.  kind: "identity" | "perm" |
    "dense_int" (dense_weights, value Linear = value_vector) | "dense_scaled" (dense_weights times 2^-s, exact in both
    operand types; the value Linear all zero, so the value is tanh(0)) | "bias_row" (policy weights all zero, the policy
    bias a chosen f32 row -- zero as exported, with_bias() puts a row in --, the value Linear all zero: behind ANY tower
    with finite activations every leaf's logits are the row, bit for bit, and the value is tanh(0))"""
    def __init__(self, R, dtype, layout, kind, s=0, bias_row=None):
        A_ch, RR = 8 * R + 8, R * R
        A = A_ch * RR
        assert kind in ("identity", "perm", "bias_row") + DENSE and (s == 0 or kind == "dense_scaled")
        assert bias_row is None or kind == "bias_row"
        m = net.ResNet(stub_spec(R), 0, 64, "cpu")
        fc = torch.nn.utils.skip_init(torch.nn.Linear, A, A)
        with torch.no_grad():
            vfc = torch.nn.Linear(24 * RR, 1)
            vw, vb = value_vector(R)
            vfc.weight.copy_(torch.from_numpy(vw).view(1, -1))
            vfc.bias.fill_(float(vb))
            if kind in DENSE:
                W, bias = dense_weights(R)
                fc.weight.copy_(torch.from_numpy(W))
                fc.bias.copy_(torch.from_numpy(bias))
                if kind == "dense_scaled":
                    assert 0 <= s <= 12                           # 3 * 2^-s: a normal number of both operand types
                    fc.weight.mul_(2.0 ** -s)
                    fc.bias.mul_(2.0 ** -s)
                    vfc.weight.zero_()
                    vfc.bias.zero_()
                del W
            else:
                fc.weight.zero_()
                fc.bias.zero_()
                if kind == "bias_row":
                    vfc.weight.zero_()
                    vfc.bias.zero_()
                    if bias_row is not None:
                        fc.bias.copy_(torch.from_numpy(np.asarray(bias_row, np.float32)))
                elif kind == "identity":
                    fc.weight.diagonal().fill_(1.0)
                else:
                    perm, scale = permutation(R)
                    fc.weight[torch.arange(A), torch.from_numpy(perm)] = torch.from_numpy(scale)
        m.policyHead[4], m.valueHead[4] = fc, vfc
        blob = weights.export_weights(m.eval(), dtype, fc_layout=layout)
        del m, fc
        magic, version, r, F, nb, dt, a_ch, self.Np, self.Kp, lay = struct.unpack_from("<4s9i", blob, 0)
        assert (magic, version, r, F, nb, dt, a_ch, lay) == (b"FPCW", 3, R, 64, 0, dtype, A_ch, layout)
        self.R, self.dtype, self.layout, self.kind, self.s = R, dtype, layout, kind, s
        self.bytes = blob[head_len(64, 0):]

    def with_bias(self, row):
        """a copy of a "bias_row" Tail whose policy bias is the f32 row [A], any bit patterns (the blob carries the bias
        as f32 [Np] right behind the [Np][Kp] 16-bit weights; held against a plain export by tests/test_prior_range_cpu.py)"""
        import copy
        assert self.kind == "bias_row"
        row = np.ascontiguousarray(row, np.float32)
        fb = np.zeros(self.Np, np.float32)
        fb[:row.size] = row
        off = self.Np * self.Kp * 2
        t = copy.copy(self)
        t.bytes = self.bytes[:off] + fb.tobytes() + self.bytes[off + 4 * self.Np:]
        return t


_tails = {}


def tail(R, dtype, layout, kind, keep=2, s=0):
    """one exported Linear per (board, operand type, layout, kind, scale exponent); of the large ones (1.1 GB each at
    14x14) only the last `keep` stay cached"""
    key = (R, dtype, layout, kind) + ((s,) if s else ())
    if key not in _tails:
        big = [k for k in _tails if k[0] >= 12]
        while R >= 12 and len(big) >= keep:
            _tails.pop(big.pop(0))
        _tails[key] = Tail(R, dtype, layout, kind, s)
    return _tails[key]


def splice(m, t):
    """the blob of the network with m's convolutions (m on the stub geometry) and t's Linears"""
    cb = weights.export_weights(m, t.dtype, fc_layout=1)
    magic, version, r1, F, nb, dt, a_ch, _np, _kp, _lay = struct.unpack_from("<4s9i", cb, 0)
    assert r1 == 1 and a_ch == 8 * t.R + 8 and dt == t.dtype
    hl = head_len(F, nb)
    return struct.pack("<4s9i24x", b"FPCW", 3, t.R, F, nb, t.dtype, a_ch, t.Np, t.Kp, t.layout) + cb[64:hl] + t.bytes


def dense_apply(flat, W, bias, block=1024):
    """flat @ W.T + bias in float64, W (int8) converted one block of output columns at a time: no A x A matrix wider
    than int8 ever exists"""
    x = torch.from_numpy(np.ascontiguousarray(flat, np.float64))
    A = W.shape[0]
    out = torch.empty(flat.shape[0], A, dtype=torch.float64)
    Wt = torch.from_numpy(W)
    # ONE conversion buffer, refilled block after block: at 14x14 the int8 -> float64 conversion of 553 M elements is most
    # of a call (one call per search step), and into fresh memory it costs three times as much
    buf = torch.empty(min(block, A), A, dtype=torch.float64)
    for c in range(0, A, block):
        n = min(block, A - c)
        buf[:n].copy_(Wt[c:c + n])
        out[:, c:c + n] = x @ buf[:n].t()
    out = out.numpy()
    return out + np.asarray(bias, np.float64)[None, :]


def linear_conditions(flat, W, bias):
    """the dense integer Linear's exactness condition, from the reference alone: integer activations, and
    max_row sum|x| * max|w| + max|bias| < 2^24 -- then EVERY partial sum of a logit, in any order and any grouping,
    is an integer below 2^24 and fp32 accumulation is exact (a power-of-two scale of W and bias changes nothing).
    Returns the left-hand side."""
    flat = np.asarray(flat, np.float64)
    assert np.array_equal(flat, np.rint(flat))
    lhs = float(np.abs(flat).sum(axis=1).max()) * float(np.abs(W).max()) + float(np.abs(bias).max())
    assert lhs < 2.0 ** 24, ("a partial sum of the dense integer Linear may leave fp32's exact integers", lhs)
    return lhs


def expected_logits(policy, kind, R, s=0):
    """what the probe's logits must be, from the reference's policy-conv output [n, A_ch, R, R] (NCHW flatten)"""
    flat = policy.reshape(policy.shape[0], -1)
    if kind == "identity":
        return flat
    if kind in DENSE:
        W, bias = dense_weights(R)
        return dense_apply(flat, W, bias) * (2.0 ** -s if kind == "dense_scaled" else 1.0)
    perm, scale = permutation(R)
    return flat[:, perm] * scale.astype(np.float64)[None, :] + 0.0


# ---------------------------------------------------------------------------------------------------------------------
# the dense integer Linear taken apart the way k_fcw / k_fc16 + k_fc_reduce take it apart (csrc/fpc_fc.h): the engine's
# K order, the blob's fragment order, 16-row x 16-column x 32-deep fragment products, K-split slabs
# ---------------------------------------------------------------------------------------------------------------------
def engine_order(a, R):
    """last axis from the reference's NCHW flatten (ch * R * R + pos) to the engine's NHWC flatten (pos * A_ch + ch)"""
    A_ch, RR = 8 * R + 8, R * R
    return np.ascontiguousarray(a.reshape(a.shape[:-1] + (A_ch, RR)).swapaxes(-1, -2)).reshape(a.shape)


def decode_linear(t):
    """the policy Linear of a Tail read back with numpy alone: (W' float32 [Np, Kp] in the engine's K order, bias
    float32 [Np]) -- the inverse of the blob's fragment order [k-step of 32][column tile of 16][lane = 16 q + c][8],
    element (ks, nt, q, c, e) = W'[16 nt + c][32 ks + 8 q + e]"""
    n = t.Np * t.Kp
    raw = np.frombuffer(t.bytes, np.uint16, n)
    if t.dtype == 1:
        v = raw.view(np.float16).astype(np.float32)
    else:
        v = (raw.astype(np.uint32) << 16).view(np.float32)
    w = v.reshape(t.Kp // 32, t.Np // 16, 4, 16, 8).transpose(1, 3, 0, 2, 4).reshape(t.Np, t.Kp)
    return w, np.frombuffer(t.bytes, np.float32, t.Np, 2 * n)      # Np * Kp * 2 bytes: a multiple of 64, no gap


def linear_splits(R, layout):
    """(columns of a column group, K-splits of column group 0) of a forward of at most 256 rows on a 256-CU part:
    plan_fcw for layout 2; layout 1 cuts its long blocks -- group 0 is one wherever there is any -- into FC_SPLITK = 4"""
    return (384, weights.fcw_split(R)) if layout == 2 else (256, 4)


LINEAR_MUTATIONS = ("drop_kstep", "seam_twice", "drop_bias4", "drop_last_slab", "rowtile15_next_kstep")


def mutated_logits(policy, R, layout, name):
    """expected_logits(policy, "dense_int", R) with ONE fault of the kind a rewrite of the Linear kernels makes, in the
    engine's own decomposition (k-steps of 32 in NHWC order, column tiles of 16, K-split slabs per column group)"""
    W, bias = dense_weights(R)
    A = W.shape[0]
    flat = policy.reshape(policy.shape[0], -1)
    out = dense_apply(flat, W, bias)
    X, Wp = engine_order(flat, R), engine_order(W, R).astype(np.float64)
    Kp = (A + 511) // 512 * 512
    gw, sk = linear_splits(R, layout)
    klen = Kp // sk                                            # K elements per slab
    g0, ct, ks = 1, gw // 16 + 5, klen // 32 + 3               # column group 1; a column tile and a k-step inside it

    def part(rows, cols, k0, k1):
        k1 = min(k1, A)
        return X[rows, k0:k1] @ Wp[cols, k0:k1].T

    every = slice(0, X.shape[0])
    if name == "drop_kstep":                                    # one k-step of one column tile never multiplied
        cols = slice(16 * ct, 16 * ct + 16)
        out[:, cols] -= part(every, cols, 32 * ks, 32 * ks + 32)
    elif name == "seam_twice":                                  # the first k-step behind a K-split seam added twice
        cols = slice(g0 * gw, min((g0 + 1) * gw, A))
        out[:, cols] += part(every, cols, 2 * klen, 2 * klen + 32)
    elif name == "drop_bias4":                                  # k_fc_reduce: the bias of one float4 of columns
        assert np.abs(bias[4 * 301:4 * 301 + 4]).max() > 0
        out[:, 4 * 301:4 * 301 + 4] -= bias[4 * 301:4 * 301 + 4]
    elif name == "drop_last_slab":                              # k_fc_reduce / logit_at: one slab short
        cols = slice(g0 * gw, min((g0 + 1) * gw, A))
        out[:, cols] -= part(every, cols, (sk - 1) * klen, sk * klen)
    elif name == "rowtile15_next_kstep":                        # row tile 15 reads the next k-step's activations
        assert X.shape[0] == 256
        rows, cols = slice(240, 256), slice(0, A)
        out[rows] += X[rows, 32 * ks + 32:32 * ks + 64] @ Wp[:, 32 * ks:32 * ks + 32].T - part(rows, cols, 32 * ks, 32 * ks + 32)
    else:
        raise ValueError(name)
    return out


def dead_fragment_products(policy, R, row_tiles=True):
    """(dead, total) over every (16-row tile, 16-column tile, 32-deep k-step) of real indices: a triple is dead when
    its contribution X[16, 32] . W[16, 32]^T is zero in all 256 elements -- dropping, duplicating or misplacing that
    fragment product would then change no logit.  row_tiles False: the rows are taken one by one (the 1-row forward),
    a (row, column tile, k-step) is dead when all 16 elements are zero.  fp32 products of integers: exact."""
    W, _ = dense_weights(R)
    A = W.shape[0]
    X = torch.from_numpy(engine_order(policy.reshape(policy.shape[0], -1), R).astype(np.float32))
    Wk = torch.from_numpy(np.ascontiguousarray(engine_order(W, R).T))       # [K, N] int8: a k-step is 32 contiguous rows
    n, nct = X.shape[0], (A + 15) // 16
    assert not row_tiles or n % 16 == 0
    assert A % 16 == 0                                          # A = 8 (R + 1) R^2: the column tiles have no ragged end
    dead = total = 0
    for k0 in range(0, A, 32):
        c = X[:, k0:k0 + 32] @ Wk[k0:k0 + 32].to(torch.float32)
        live = (c != 0).view(n // 16 if row_tiles else n, 16 if row_tiles else 1, nct, 16).any(dim=3).any(dim=1)
        dead += int((~live).sum())
        total += live.numel()
    return dead, total


def linear_rows(rows_max, n):
    """which rows of a case's prepared inputs a forward of n rows takes: the whole set, or a window that does NOT start
    at row 0 -- whatever an earlier, larger call left in the engine's buffers then belongs to other inputs"""
    if n == rows_max:
        return slice(0, n)
    lo = {37: 64, 1: 128}[n]
    return slice(lo, lo + n)


def linear_case(R, dtype, rows):
    """the prepare() case of a dense-Linear test: family A, hidden 128, 3 blocks with fp16 / 2 with bf16"""
    return ("linear", R, 128, 3 if dtype == 1 else 2, dtype, "A", {}, rows)


def dense_reference(p, R):
    """expected dense_int logits of a prepared case, computed once; the exactness condition asserted"""
    if "dense_int" not in p:
        W, bias = dense_weights(R)
        p["linear_lhs"] = linear_conditions(p["ref"]["policy"].reshape(p["x"].shape[0], -1), W, bias)
        p["dense_int"] = expected_logits(p["ref"]["policy"], "dense_int", R)
    return p["dense_int"]


def _linear_cases():
    """(R, operand type, layout, row counts run one after the other on ONE engine), ordered so that cases sharing a
    (board, type) preparation and a (board, type, layout) tail are neighbours"""
    out = []
    for R in (8, 9, 10, 11, 12, 13, 14):
        full = R in (8, 10, 14)
        seq = (256, 37, 1) if full else (256, 37)
        for dtype in (1, 0):
            for layout in (2, 1):
                if full or dtype == 1 or layout == weights.default_fc_layout(R):
                    out.append((R, dtype, layout, seq))
                # two row tiles (blockIdx.y = 1, Mtot = 512): 10x10 layout 1 keeps a long / short mix above 256 rows (the
                # only shape whose mix CHANGES there), 14x14 layout 1 becomes all-long
                if dtype == 1 and ((R in (8, 14)) or (R == 10 and layout == 1)):
                    out.append((R, dtype, layout, (300,)))
    return out


LINEAR_CASES = _linear_cases()


def linear_case_id(c):
    return "%dx%d-%s-layout%d-%s" % (c[0], c[0], FMT[c[1]]["name"], c[2], "-".join(str(n) for n in c[3]))


# ---------------------------------------------------------------------------------------------------------------------
# the cases of tests/test_tower_probe_gpu.py: (kernel, R, hidden, blocks, dtype, family, developer knobs, rows)
# Family A depths: 3 blocks with fp16 operands, 2 with bf16 (integers stay below 2^11 / 2^8; test_tower_probe_cpu.py
# asserts the conditions for every case of this table).  Family B depths: 2, 3, 10 at hidden 128 and 2, 20 at hidden 256;
# 2 at the per-layer path's widths 64, 192 and 512.
# ---------------------------------------------------------------------------------------------------------------------
def _cases():
    out = []

    def add(kernel, R, hidden, blocks, dtype, family, knobs=None, rows=37):
        out.append((kernel, R, hidden, blocks, dtype, family, dict(knobs or {}), rows))

    def both_a(kernel, R, hidden, knobs=None):
        add(kernel, R, hidden, 3, 1, "A", knobs)
        add(kernel, R, hidden, 2, 0, "A", knobs)

    # k_towerc: 14x14, hidden 128
    both_a("k_towerc", 14, 128)
    add("k_towerc", 14, 128, 3, 1, "A", None, 300)
    both_a("k_towerc", 14, 128, {"FPC_TOWER_TAPLOOP": "0"})      # the rolled tap loop
    add("k_towerc", 14, 128, 2, 1, "B", {"FPC_TOWER_TAPLOOP": "0"})
    for blocks in (2, 3, 10):
        for dtype in (1, 0):
            add("k_towerc", 14, 128, blocks, dtype, "B")
    # k_towerw<128>: one wave row at 8x8, two wave rows at 9..13 (3 / 4 / 5 / 6 row tiles)
    for R in (8, 9, 10, 11, 12, 13):
        both_a("k_towerw", R, 128)
    add("k_towerw", 8, 128, 3, 1, "A", None, 300)
    for R, blocks in ((8, 10), (10, 3), (13, 2)):
        for dtype in (1, 0):
            add("k_towerw", R, 128, blocks, dtype, "B")
    # k_towerw<256>: R = 8..14 (4 / 6 / 7 / 8 / 9 / 11 / 13 row tiles), and two wave rows
    for R in (8, 9, 10, 11, 12, 13, 14):
        both_a("k_towerw", R, 256)
    for R in (8, 14):
        both_a("k_towerw", R, 256, {"FPC_TOWERW_ROWS": "2"})
    add("k_towerw", 8, 256, 3, 1, "A", None, 300)
    for R, blocks in ((8, 2), (14, 2), (14, 20)):
        for dtype in (1, 0):
            add("k_towerw", R, 256, blocks, dtype, "B")
    add("k_towerw", 14, 256, 2, 1, "B", {"FPC_TOWERW_ROWS": "2"})
    # k_conv3x3, one launch per layer: hidden 64 always, hidden 128 / 256 under FPC_NO_TOWER=1
    for hidden, knobs in ((64, None), (128, {"FPC_NO_TOWER": "1"}), (256, {"FPC_NO_TOWER": "1"})):
        for R in (8, 14):
            both_a("k_conv3x3", R, hidden, knobs)
        for dtype in (1, 0):
            add("k_conv3x3", 14, hidden, 2, dtype, "B", knobs)
    add("k_conv3x3", 8, 64, 3, 1, "A", None, 300)
    # k_conv3x3 WITHOUT a knob (the product dispatch must choose it), on every board and at every width it serves:
    # boards 9..13: the bordered grid has 121 / 144 / 169 / 196 / 225 rows per game, so the 256-row blocks straddle games at
    # another offset in every block, the halo is 12..16 rows and every m / PP, pos / P, pos % P runs on an odd pitch;
    # 300 rows at 13x13: nearly every block straddles two games
    for R in (9, 10, 11, 12, 13):
        both_a("k_conv3x3", R, 64)
    add("k_conv3x3", 13, 64, 3, 1, "A", None, 300)
    # widths: 192 / 320 / 448 as 3 / 5 / 7 slabs of 64 channels, 384 / 512 as 3 / 4 slabs of 128 (grid.y 2..4, pitches up to
    # 1024 bytes); 37 games of PP = 100 are 15 blocks, every block boundary inside a game
    for hidden in (192, 320, 384, 448, 512):
        both_a("k_conv3x3", 8, hidden)
    # an odd pitch and more than one slab at once
    add("k_conv3x3", 9, 192, 3, 1, "A")
    add("k_conv3x3", 13, 512, 3, 1, "A")
    # family A draws 7 of 9 * cin products per output channel; family B touches every one
    for hidden in (192, 512):
        for dtype in (1, 0):
            add("k_conv3x3", 8, hidden, 2, dtype, "B")
    # k_tower on the bordered grid: 14x14 on 8 and on 4 waves, and the sizes k_towerw took over
    for R, knobs in ((14, {"FPC_TOWER_COMPACT": "0"}), (14, {"FPC_TOWER_COMPACT": "0", "FPC_TOWER_WAVES": "4"}),
                     (8, {"FPC_TOWERW": "0"}), (10, {"FPC_TOWERW": "0"}), (13, {"FPC_TOWERW": "0"})):
        both_a("k_tower", R, 128, knobs)
    for R, knobs in ((14, {"FPC_TOWER_COMPACT": "0"}), (8, {"FPC_TOWERW": "0"})):
        for dtype in (1, 0):
            add("k_tower", R, 128, 2, dtype, "B", knobs)
    add("k_tower", 8, 128, 3, 1, "A", {"FPC_TOWERW": "0"}, 300)
    return out


CASES = _cases()


def case_id(c):
    kernel, R, hidden, blocks, dtype, family, knobs, rows = c
    return "%s-%dx%d-h%d-b%d-%s-%s-%s%d" % (kernel, R, R, hidden, blocks, FMT[dtype]["name"], family,
                                           "".join("%s=%s-" % (k[4:].lower(), v) for k, v in sorted(knobs.items())), rows)


_prepared = {}


def prepare(case):
    """everything a case needs that the GPU does not: the network, its inputs, the float64 reference and -- family B --
    the figures of the fp32 order on the CPU; family A's conditions are asserted here.  Cases that differ only in the
    kernel share one preparation."""
    kernel, R, hidden, blocks, dtype, family, knobs, rows = case
    key = (R, hidden, blocks, dtype, family, rows)
    if key in _prepared:
        return _prepared[key]
    seed = 100 * R + blocks
    x = probe_inputs(R, rows, seed=seed, density=0.25 if family == "A" else 0.1)
    m = integer_net(R, blocks, hidden, seed) if family == "A" else dense_net(R, blocks, hidden, seed)
    layers = conv_layers(m, dtype)
    ref = forward(layers, x, dtype)
    p = {"net": m, "x": x, "ref": ref}
    if family == "A":
        p["conditions"] = integer_conditions(ref, dtype)
        # the value: tanh of the float64 pre-activation, bounded as family B's is.  Every fp32 order of the convolutions
        # gives the reference's own integers here (rounded and unrounded value conv alike), so the CPU fp32 figure is that
        # of the value Linear alone
        vw, vb = value_vector(R)
        assert np.array_equal(ref["vconv"], ref["vconv_unrounded"])
        rv = value_of(ref["vconv"], vw, vb)
        fig = float(np.abs(value_of(ref["vconv"], vw, vb, "f32") - rv).max())
        p["ref_value"] = {"value": rv, "value_unrounded": rv}
        p["cpu"] = {"value": fig, "value_unrounded": fig}
        p["value_floor"] = 2.0 * float(quantum(ref["vconv"].max(), dtype)) * float(np.abs(vw).max())
    else:
        # the CPU figure: the noisiest of a fixed set of fp32 orders.  One order is one draw: on a shallow
        # network the elements more than one rounding away are 0..8 of 10^6 and differ from order to order by more than the
        # factor 2 of the bound, so networks of at most 3 blocks draw eight orders; on deeper ones the orders agree within
        # a few per cent and three are drawn
        vw, vb = value_vector(R)
        # "value": the value conv's output rounded to 16 bits (k_conv3x3 + k_value_tail); "value_unrounded": not (towers)
        vk = {"value": "vconv", "value_unrounded": "vconv_unrounded"}
        p["ref_value"] = {k: value_of(ref[v], vw, vb) for k, v in vk.items()}
        figs = []
        for order in (SHALLOW_ORDERS if blocks <= 3 else BASE_ORDERS):
            cpu = forward(layers, x, dtype, order)
            f = {"tower": noise_figures(cpu["tower"], ref["tower"], dtype),
                 "policy": noise_figures(cpu["policy"], ref["policy"], dtype)}
            for k, v in vk.items():
                f[k] = float(np.abs(value_of(cpu[v], vw, vb, "f32") - p["ref_value"][k]).max())
            figs.append(f)
        p["cpu_orders"] = figs
        p["cpu"] = {"tower": tuple(max(f["tower"][i] for f in figs) for i in (0, 1)),
                    "policy": tuple(max(f["policy"][i] for f in figs) for i in (0, 1)),
                    "value": max(f["value"] for f in figs), "value_unrounded": max(f["value_unrounded"] for f in figs)}
        # two roundings of the largest value-conv activation through the largest weight: the floor of the value bound
        p["value_floor"] = 2.0 * float(quantum(ref["vconv"].max(), dtype)) * float(np.abs(vw).max())
    if len(_prepared) >= 4:
        _prepared.pop(next(iter(_prepared)))
    _prepared[key] = p
    return p
