"""Export of a ResNet (net.py here, or the reference's net.py -- same parameter names) into the
flat weight blob the engine's MFMA kernels consume (format: csrc/fpc_nn.h "weight blob").

eval()-mode BatchNorm is folded into the preceding conv (the search runs under model.eval() +
torch.no_grad(), alphazero.py:262 / mcts.py:15):   w' = w * g/sqrt(var+eps),  b' = (b-mean)*g/sqrt(var+eps)+beta.
Conv weights go to [tap][Cout_pad][Cin_pad] (K contiguous); the policy Linear's input axis is
permuted from the reference's NCHW flatten (ch*R*R + pos) to the engine's NHWC flatten
(pos*A_ch + ch) and both axes are zero-padded to tile multiples."""
import os
import struct

import numpy as np
import torch


def _cpu(t):
    """a detached fp32 host copy; the caller's module stays on its device"""
    return t.detach().to("cpu", torch.float32)


def _fold(conv, bn):
    w = _cpu(conv.weight)
    b = _cpu(conv.bias) if conv.bias is not None else torch.zeros(w.shape[0])
    s = _cpu(bn.weight) / torch.sqrt(_cpu(bn.running_var) + bn.eps)
    return w * s.view(-1, 1, 1, 1), (b - _cpu(bn.running_mean)) * s + _cpu(bn.bias)


def _to16(t, dtype):
    t = t.contiguous()
    if dtype == 0:
        return t.to(torch.bfloat16).view(torch.int16).numpy().tobytes()
    return t.to(torch.float16).view(torch.int16).numpy().tobytes()


def _conv_section(w, b, cin_pad, cout_pad, dtype):
    cout, cin = w.shape[0], w.shape[1]
    wt = torch.zeros(9, cout_pad, cin_pad)
    wt[:, :cout, :cin] = w.permute(2, 3, 0, 1).reshape(9, cout, cin)     # tap = ky*3+kx
    bb = torch.zeros(cout_pad)
    bb[:cout] = b
    return [_to16(wt, dtype), bb.numpy().astype(np.float32).tobytes()]


# Fragment order / block tile of the policy Linear: 2 = 16x16x32 fragments over 384-column groups (k_fcw: 256 x 384 block
# tiles, ONE round of blocks; the default wherever its one-round K-split exists on a 256-CU part: every board of 8..14
# a side), 1 = the same fragment order over 256-column groups (k_fc16: long and short blocks in two rounds; the fallback).
# FPC_FC_LAYOUT forces one.  (0, the 32x32x16 order of k_fc, was retired in round 5 together with blob version 2.)
FC_LAYOUT = int(os.environ["FPC_FC_LAYOUT"]) if "FPC_FC_LAYOUT" in os.environ else None


def fcw_split(R, cus=256):
    """K-splits k_fcw would use for an R x R board on a part with `cus` CUs (csrc/fpc_nn.h: plan_fcw), 0 if none"""
    A = (8 * R + 8) * R * R
    groups, stages = (A + 383) // 384, ((A + 511) // 512 * 512) // 64
    best = 0
    for sk in range(1, 9):
        if groups * sk <= cus and stages % sk == 0 and stages // sk >= 4:
            best = sk
    return best


def default_fc_layout(R):
    if FC_LAYOUT is not None:
        return FC_LAYOUT
    return 2 if fcw_split(R) else 1


FC_WEIGHTS = {"w16": 0, "int8": 1}     # the blob header's fc_wtype / include/fpc_engine.h FPC_FC_W16, FPC_FC_W8


def quantize_fc(weight_f32, block=1024):
    """The policy Linear's opt-in 8-bit weights: weight f32 [N, K], one scale per output row n.
    m_n = max_k |w[n][k]|;  s_n = m_n / 127 (f32, correctly rounded);  m_n < 127 * 2^-100 (zero included): s_n = 1 and the
    row quantises to zeros;  q[n][k] = clamp(rint(w[n][k] / s_n), -127, 127), ties to even.  -128 is never written.
    A non-finite weight refuses the export (ValueError).  Returns (q int8 [N, K], scale f32 [N]).  Every op is an f32
    torch CPU op, so k_pack_fc8 (csrc/fpc_pack.h) reproduces it byte for byte."""
    w = _cpu(weight_f32)
    if not bool(torch.isfinite(w).all()):
        raise ValueError("policy Linear: non-finite weight, int8 export refused")
    m = w.abs().amax(dim=1)
    s = m / torch.tensor(127.0, dtype=torch.float32)
    s = torch.where(m < 127.0 * 2.0 ** -100, torch.ones_like(s), s)
    q = torch.empty(w.shape, dtype=torch.int8)
    for r in range(0, w.shape[0], block):      # row blocks: no second f32 copy of a 2.2 GB matrix
        q[r:r + block] = torch.round(w[r:r + block] / s[r:r + block, None]).clamp_(-127.0, 127.0).to(torch.int8)
    return q, s


def export_weights(model, dtype=0, fc_layout=None, fc_weights="w16"):
    """model: ResNet in eval semantics.  dtype 0 = bf16, 1 = fp16.  fc_weights "w16" (the default: 16-bit policy-Linear
    weights, blob version 3) or "int8" (opt-in, fp16 and fc_layout 2 only: quantize_fc, blob version 4).  Returns bytes."""
    if fc_weights not in FC_WEIGHTS:
        raise ValueError("fc_weights must be \"w16\" or \"int8\"")
    wtype = FC_WEIGHTS[fc_weights]
    F = model.startBlock[0].weight.shape[0]
    nblocks = len(model.backBone)
    A_ch = model.policyHead[0].weight.shape[0]
    fc = model.policyHead[4]
    A = fc.weight.shape[0]
    RR = A // A_ch
    R = int(round(RR ** 0.5))
    assert R * R == RR and fc.weight.shape[1] == A
    fc_layout = default_fc_layout(R) if fc_layout is None else int(fc_layout)
    gw = 384 if fc_layout == 2 else 256
    Np = (A + gw - 1) // gw * gw         # a block owns gw columns
    Kp = (A + 511) // 512 * 512      # k_fc: K/16 k-steps, split-K 4 (8 for the short blocks), 4 k-steps per stage, stages in pairs
    if wtype and (fc_layout != 2 or dtype != 1):
        raise ValueError("int8 policy-Linear weights need fp16 operands (dtype 1) and fc_layout 2 (k_fcw8)")
    secs = []
    w, b = _fold(model.startBlock[0], model.startBlock[1])
    Fp = (F + 127) // 128 * 128
    secs += _conv_section(w, b, 32, Fp, dtype)
    for blk in model.backBone:
        w, b = _fold(blk.conv1, blk.bn1)
        secs += _conv_section(w, b, F, Fp, dtype)
        w, b = _fold(blk.conv2, blk.bn2)
        secs += _conv_section(w, b, F, Fp, dtype)
    w, b = _fold(model.policyHead[0], model.policyHead[1])
    secs += _conv_section(w, b, F, 128, dtype)
    w, b = _fold(model.valueHead[0], model.valueHead[1])
    secs += _conv_section(w, b, F, 128, dtype)
    # policy Linear: in index ch*RR+pos -> pos*A_ch+ch ; pad to [Np][Kp]
    fw = _cpu(fc.weight).view(A, A_ch, RR).permute(0, 2, 1).reshape(A, A)
    if fc_layout not in (1, 2):
        raise ValueError("fc_layout must be 1 (k_fc16) or 2 (k_fcw); 0 (k_fc) was retired")
    if wtype:
        # int8 in FRAGMENT-PAIR order [kstep32][n_pair32][lane = 16*q + c][2 tiles][8]: element (ks, np, q, c, t, e) =
        # q8[np*32 + t*16 + c][ks*32 + q*8 + e] -- a lane's 16 bytes are the fragments of two column tiles (k_fcw8);
        # then the scales f32[Np] (1.0 in the padding)
        q8, sc = quantize_fc(fw)
        del fw
        qp = torch.zeros(Np, Kp, dtype=torch.int8)
        qp[:A, :A] = q8
        del q8
        qf = qp.view(Np // 32, 2, 16, Kp // 32, 4, 8).permute(3, 0, 4, 2, 1, 5).contiguous()
        del qp
        secs.append(qf.numpy().tobytes())
        del qf
        fs = np.ones(Np, np.float32)
        fs[:A] = sc.numpy()
        secs.append(fs.tobytes())
    else:
        t16 = torch.bfloat16 if dtype == 0 else torch.float16
        fwp = torch.zeros(Np, Kp, dtype=t16)
        fwp[:A, :A] = fw.to(t16)
        del fw
        # MFMA fragment order of k_fc16 / k_fcw (16x16x32): [kstep32][n_tile16][lane = 16*q + c][8],
        # element (ks, nt, q, c, e) = W'[nt*16 + c][ks*32 + q*8 + e]
        wf = fwp.view(Np // 16, 16, Kp // 32, 4, 8).permute(2, 0, 3, 1, 4).contiguous()
        del fwp
        secs.append(wf.view(torch.int16).numpy().tobytes())
        del wf
    fb = np.zeros(Np, np.float32)
    fb[:A] = _cpu(fc.bias).numpy()
    secs.append(fb.tobytes())
    vfc = model.valueHead[4]
    vw = torch.zeros(RR, 32)
    vw[:, :24] = _cpu(vfc.weight).view(24, RR).t()
    secs.append(vw.numpy().astype(np.float32).tobytes())
    secs.append(struct.pack("<f", float(_cpu(vfc.bias).item())))
    # version 3: the header word fc_layout names the policy Linear's layout (version 2, rounds 1-2: k_fc's 32x32x16
    # order without that word; an engine of that time refuses version 3, this engine refuses version 2)
    # version 4: the header word fc_wtype (byte 40, the first of version 3's pad words) = 1, the policy-fc section is int8 in
    # pair order + scales; a blob with fc_wtype 0 IS version 3, byte for byte
    version = 4 if wtype else 3
    out = bytearray(struct.pack("<4s10i20x", b"FPCW", version, R, F, nblocks, dtype, A_ch, Np, Kp, fc_layout, wtype))
    assert len(out) == 64
    for s in secs:
        out += b"\0" * ((-len(out)) % 64)
        out += s
    return bytes(out)


def net_src(model, device):
    """The module's parameters as the device-side pack reads them (include/fpc_engine.h fpc_net_src): returns
    (descriptor, keep).  Every tensor is detach().to(float32).contiguous() on `device` -- no copy for an fp32 module that
    already lies there -- and `keep` holds them (and the ctypes arrays the descriptor points into) alive: keep it until
    the call that takes the descriptor has returned.  device "cpu" serves the emulator build, whose "device" memory is
    host memory."""
    import fpc_ffi
    keep = []

    def ptr(t):
        t = t.detach().to(device=device, dtype=torch.float32).contiguous()
        keep.append(t)
        return fpc_ffi.C.cast(t.data_ptr(), fpc_ffi.P(fpc_ffi.C.c_float))

    def conv(cv, bn):
        return fpc_ffi.ConvSrc(ptr(cv.weight), ptr(cv.bias) if cv.bias is not None else None, ptr(bn.weight), ptr(bn.bias),
                               ptr(bn.running_mean), ptr(bn.running_var), float(bn.eps), int(cv.weight.shape[1]), int(cv.weight.shape[0]))

    nblocks = len(model.backBone)
    c1 = (fpc_ffi.ConvSrc * max(nblocks, 1))(*[conv(b.conv1, b.bn1) for b in model.backBone])
    c2 = (fpc_ffi.ConvSrc * max(nblocks, 1))(*[conv(b.conv2, b.bn2) for b in model.backBone])
    keep += [c1, c2]
    fc, vfc = model.policyHead[4], model.valueHead[4]
    src = fpc_ffi.NetSrc(int(model.startBlock[0].weight.shape[0]), nblocks, conv(model.startBlock[0], model.startBlock[1]),
                         conv(model.policyHead[0], model.policyHead[1]), conv(model.valueHead[0], model.valueHead[1]),
                         fpc_ffi.C.cast(c1, fpc_ffi.P(fpc_ffi.ConvSrc)), fpc_ffi.C.cast(c2, fpc_ffi.P(fpc_ffi.ConvSrc)),
                         ptr(fc.weight), ptr(fc.bias), ptr(vfc.weight), ptr(vfc.bias))
    return src, keep
