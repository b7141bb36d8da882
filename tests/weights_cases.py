"""Shared cases of the device-side weight pack (fpc_weights_pack / fpc_load_weights_device): fixture modules with
randomised BatchNorm statistics, the host export as the reference, and the byte comparison.  Used by
test_weights_device_emul.py (wavefront emulator, CPU) and test_weights_device_gpu.py (HIP engine)."""
import copy
import ctypes as C
import struct

import numpy as np
import torch

import fpc_ffi
import weights
from net_cases import Spec

INV_OF = {8: 2, 9: 2, 11: 3, 14: 3}
EINVAL, EWEIGHTS = -1, -10

_models, _blobs = {}, {}


def host_exact_var(var, eps):
    """The byte comparison rests on the host export following the f32 spec op for op (s = g / sqrt(var + eps) with a
    correctly rounded square root, which is what the kernel computes).  torch's CPU sqrt is a vector-library routine that
    on some builds is not correctly rounded: about 0.7 % of the f32 values in [0.01, 3] come out one unit off (seen: var +
    eps = 0x1.175148p+1 gives 0x1.7a2ad8p+0, the correctly rounded root is 0x1.7a2adap+0).  Such a draw is moved to the next
    float, so that the reference blob IS the spec; numpy's f32 sqrt is the correctly rounded one.  What the pack does on
    the draws this function moves away is held by case_spec_bytes against the numpy fold."""
    var = var.clone()
    for _ in range(8):
        x = var + eps
        bad = torch.sqrt(x) != torch.from_numpy(np.sqrt(x.numpy()))
        if not bool(bad.any()):
            return var
        var[bad] = torch.nextafter(var[bad], torch.full_like(var[bad], 4.0))
    raise AssertionError("the host square root disagrees with the correctly rounded one on consecutive floats")


def inexact_vars(eps, n, seed=0):
    """up to n variances in [0.01, 3] on which torch's CPU sqrt(var + eps) is NOT the correctly rounded root (none on a
    build whose sqrt is exact)"""
    g = torch.Generator().manual_seed(seed + 99)
    v = torch.rand(200000, generator=g) * 2.99 + 0.01
    x = v + eps
    bad = torch.sqrt(x) != torch.from_numpy(np.sqrt(x.numpy()))
    return v[bad][:n].clone()


def numpy_fold(conv, bn):
    """weights._fold written op by op in numpy f32 (correctly rounded divide and square root, no contraction): the
    numeric spec of k_pack_conv"""
    def f(t):
        return t.detach().to("cpu", torch.float32).numpy()
    w = f(conv.weight)
    b = f(conv.bias) if conv.bias is not None else np.zeros(w.shape[0], np.float32)
    s = f(bn.weight) / np.sqrt(f(bn.running_var) + np.float32(bn.eps))
    return torch.from_numpy(w * s[:, None, None, None]), torch.from_numpy((b - f(bn.running_mean)) * s + f(bn.bias))


def case_spec_bytes(eng, R, blocks, hidden, dtype, layout, monkeypatch):
    """The property a user can rely on whatever the host's sqrt does: on UNSHIFTED random variances, with values planted
    on which torch's CPU sqrt is one unit off, the packed blob equals export_weights run over the op-by-op numpy f32 fold
    byte for byte.  Returns (planted values, bytes in which the plain host export differs from the pack)."""
    m = copy.deepcopy(model(R, blocks, hidden))
    g = torch.Generator().manual_seed(5)
    planted = 0
    with torch.no_grad():
        for i, mod in enumerate(b for b in m.modules() if isinstance(b, torch.nn.BatchNorm2d)):
            mod.running_var.copy_(torch.rand(mod.num_features, generator=g) * 2.99 + 0.01)      # not passed through host_exact_var
            bad = inexact_vars(mod.eps, 4, seed=i)
            mod.running_var[:bad.numel()] = bad
            planted += int(bad.numel())
    host = weights.export_weights(m, dtype, layout)
    monkeypatch.setattr(weights, "_fold", numpy_fold)
    spec = weights.export_weights(m, dtype, layout)
    monkeypatch.undo()
    got = eng.weights_pack(m, layout)
    assert_same_blob(got, spec, "numpy fold, R=%d hidden=%d dtype=%d layout=%d" % (R, hidden, dtype, layout))
    differ = int(np.count_nonzero(np.frombuffer(got, np.uint8) != np.frombuffer(host, np.uint8)))
    print("planted %d variances with an inexact host sqrt; the plain host export differs from the pack in %d bytes" % (planted, differ))
    return planted, differ


def model(R, blocks, hidden, seed=0):
    """net.ResNet on the CPU in eval mode.  BatchNorm statistics, weights and biases are RANDOM (var in [0.01, 3], normal
    weight, bias and mean): a default-initialised BN folds to the identity.  A slice of the policy Linear is scaled into
    the f32 / bf16 subnormal range, so that a flushing conversion cannot pass in either 16-bit type (fp16 subnormals come
    from the default initialisation by themselves).  Cached: the tests share one module and one reference blob per shape."""
    key = (R, blocks, hidden, seed)
    if key not in _models:
        import net
        torch.manual_seed(1000 * R + 10 * blocks + hidden + seed)
        m = net.ResNet(Spec(R), blocks, hidden, "cpu")
        g = torch.Generator().manual_seed(seed + 7)
        with torch.no_grad():
            for mod in m.modules():
                if isinstance(mod, torch.nn.BatchNorm2d):
                    n = mod.num_features
                    mod.running_var.copy_(host_exact_var(torch.rand(n, generator=g) * 2.99 + 0.01, mod.eps))
                    mod.running_mean.copy_(torch.randn(n, generator=g))
                    mod.weight.copy_(torch.randn(n, generator=g))
                    mod.bias.copy_(torch.randn(n, generator=g))
            m.policyHead[4].weight[5:37] *= 1e-36
        m.eval()
        _models[key] = m
    return _models[key]


def reference_blob(m, key, dtype, layout):
    """weights.export_weights, computed once per (module, dtype, layout) and left unchanged"""
    k = (key, dtype, layout)
    if k not in _blobs:
        _blobs[k] = weights.export_weights(m, dtype, layout)
    return _blobs[k]


def geometry(R, hidden, blocks, layout):
    A_ch = 8 * R + 8
    A = A_ch * R * R
    gw = 384 if layout == 2 else 256
    Np, Kp = (A + gw - 1) // gw * gw, (A + 511) // 512 * 512
    Fp = (hidden + 127) // 128 * 128
    off = 64 + 9 * Fp * 32 * 2 + Fp * 4 + 2 * blocks * (9 * Fp * hidden * 2 + Fp * 4) + 2 * (9 * 128 * hidden * 2 + 128 * 4)
    return {"A": A, "A_ch": A_ch, "Np": Np, "Kp": Kp, "fc_off": off, "fc_bytes": Np * Kp * 2}


def subnormal_count(blob, geo, dtype):
    """16-bit subnormals (exponent field 0, mantissa not 0) in the blob's policy-Linear section"""
    w = np.frombuffer(blob, np.uint16, geo["fc_bytes"] // 2, geo["fc_off"])
    emask = 0x7f80 if dtype == 0 else 0x7c00
    return int(np.count_nonzero(((w & emask) == 0) & ((w & 0x7fff) != 0)))


def assert_same_blob(got, ref, what):
    assert len(got) == len(ref), (what, len(got), len(ref))
    assert got[:64] == ref[:64], (what, struct.unpack("<4s9i24x", got[:64]), struct.unpack("<4s9i24x", ref[:64]))
    if got != ref:
        a, b = np.frombuffer(got, np.uint8), np.frombuffer(ref, np.uint8)
        bad = np.nonzero(a != b)[0]
        raise AssertionError("%s: %d bytes differ, first at offset %d (got %d, want %d)" % (what, bad.size, bad[0], a[bad[0]], b[bad[0]]))


def case_bytes(eng, R, blocks, hidden, dtype, layout):
    """weights_pack == export_weights byte for byte; header, nbytes == fpc_weights_blob_size == len(blob)"""
    m = model(R, blocks, hidden)
    ref = reference_blob(m, (R, blocks, hidden), dtype, layout)
    geo = geometry(R, hidden, blocks, layout)
    hdr = struct.unpack("<4s9i24x", ref[:64])
    assert hdr[7] == geo["Np"] and hdr[8] == geo["Kp"]
    nsub = subnormal_count(ref, geo, dtype)
    assert nsub > 0, "the reference blob holds no 16-bit subnormal: the comparison would let a flushing conversion pass"
    assert eng.weights_blob_size(hidden, blocks, layout) == len(ref)
    got = eng.weights_pack(m, layout)
    assert_same_blob(got, ref, "R=%d blocks=%d hidden=%d dtype=%d layout=%d" % (R, blocks, hidden, dtype, layout))
    return nsub


def raw_src(eng, m):
    """(descriptor, keep-alive) for direct calls of the C entry points"""
    src, keep, _ = eng._net_src(m, None)
    return src, keep


def einval_cases(eng, m, layout=1, load=False):
    """every FPC_EINVAL refusal of the header comment as (name, return code) pairs, through fpc_weights_pack or (load)
    through fpc_load_weights_device"""
    L = eng.L
    out = []
    cap = eng.weights_blob_size(m.num_hidden, m.num_resBlocks, layout)
    n = C.c_uint64()
    if not load:
        buf = torch.zeros(cap + 64, dtype=torch.uint8, device="cpu" if eng.host_memory else "cuda")
        ptr = (buf.data_ptr() + 63) & ~63

    def call(src, lay=layout, p=None, c=cap, h=eng.h):
        sp = None if src is None else C.byref(src)
        return L.fpc_load_weights_device(h, sp, lay) if load else L.fpc_weights_pack(h, sp, lay, ptr if p is None else p, c, C.byref(n))

    src, keep = raw_src(eng, m)
    if not load:
        assert call(src) == 0 and n.value == cap                       # the descriptor itself is good
        out.append(("null blob", L.fpc_weights_pack(eng.h, C.byref(src), layout, None, cap, C.byref(n))))
        out.append(("cap too small", call(src, c=cap - 1)))
    out.append(("null engine", call(src, h=None)))
    out.append(("null descriptor", call(None)))
    out.append(("fc_layout 3", call(src, lay=3)))
    out.append(("fc_layout -1", call(src, lay=-1)))
    for name, edit in (("null fc_w", lambda s: setattr(s, "fc_w", None)),
                       ("null vfc_b", lambda s: setattr(s, "vfc_b", None)),
                       ("null stem.w", lambda s: setattr(s.stem, "w", None)),
                       ("null pconv.bn_var", lambda s: setattr(s.pconv, "bn_var", None)),
                       ("null c1", lambda s: setattr(s, "c1", None)),
                       ("stem cin", lambda s: setattr(s.stem, "cin", 23)),
                       ("stem cout", lambda s: setattr(s.stem, "cout", s.hidden + 64)),
                       ("block cin", lambda s: setattr(s.c1[0], "cin", s.hidden - 1)),
                       ("policy conv cout", lambda s: setattr(s.pconv, "cout", s.pconv.cout + 8)),
                       ("value conv cout", lambda s: setattr(s.vconv, "cout", 32))):
        s2, keep2 = raw_src(eng, m)
        edit(s2)
        out.append((name, call(s2)))
        del keep2
    del keep
    return out


# ---- GPU side: forwards and searches of engines loaded one way or the other ---------------------------------------------
def encodings(R, n=4, seed=3):
    """n random sparse [24, R, R] inputs on the GPU"""
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(n, 24, R, R, generator=g) < 0.06).float().cuda()


def forward(eng, x):
    """(logits, values) of fpc_nn_forward as numpy arrays"""
    n = x.shape[0]
    lg = torch.empty(n, eng.A, device="cuda")
    va = torch.empty(n, device="cuda")
    torch.cuda.synchronize()
    eng.nn_forward(x.data_ptr(), n, lg.data_ptr(), va.data_ptr())
    torch.cuda.synchronize()
    return lg.cpu().numpy(), va.cpu().numpy()


def assert_same_forward(a, b, what):
    assert np.array_equal(a[0].view(np.uint32), b[0].view(np.uint32)), "%s: logits differ" % what
    assert np.array_equal(a[1].view(np.uint32), b[1].view(np.uint32)), "%s: values differ" % what


def start_roots(R, n):
    import positions
    turn, entries = positions.start_entries(R)
    return [fpc_ffi.board_from_dict(R, turn, entries) for _ in range(n)]


def search_counts(eng, R, sims=16, games=4, legal=False, roots=None):
    """root children (flat, visits) of a fused search from the start position (or from `roots`, a list of fpc_ffi.Board)"""
    eng.set_policy_mode(legal)
    eng.search_begin(start_roots(R, games) if roots is None else [fpc_ffi.clone_board(b) for b in roots], 3.0)
    eng.search_run(sims)
    res = eng.search_results()
    return [[[int(res["flat"][g, k]), int(res["visits"][g, k])] for k in range(int(res["n_children"][g]))] for g in range(games)]
