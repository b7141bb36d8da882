// fpc_pack.h -- the device-side weight pack: the torch module's fp32 parameters, read where they lie in device memory,
// become the sections of the version-3 (int8 policy Linear: version-4) weight blob (fpc_nn.h "weight blob"), byte for byte what
// alphazero-4-player-chess_amd/weights.py export_weights produces on the host wherever the host's f32 arithmetic is
// correctly rounded (torch's CPU sqrt is not always: DESIGN 7.3).  The sections go into a blob
// (fpc_weights_pack) or straight into the engine's live weight allocations (fpc_load_weights_device).
//
// Plain HIP without MFMA or 16-bit types in the interface, so the same source runs on the wavefront emulator of the
// CPU test-suite (-DFPC_EMUL), where "device" memory is host memory.
//
//   k_pack_conv  BN fold (weights._fold op for op in f32: s = g / sqrtf(var + eps), w' = w * s, b' = (b - mean) * s + beta;
//                the build has -ffp-contract=off, divide and square root are correctly rounded) + [tap][cout_pad][cin_pad]
//                16-bit reorder of ALL convolutions in one launch over a device table of descriptors.  ~7 MB.
//   k_pack_fc    the policy Linear, the hot path: 4 A^2 bytes in, 2 Np Kp out (2.2 GB / 1.1 GB at 14x14).  Per 16-row
//                tile an [A_ch][RR] -> [RR][A_ch] transpose through LDS into MFMA fragment order.
//   k_fc_rowmax, k_pack_fc8   the same Linear as int8 + per-row scales (opt-in, fpc_set_fc_weight_type): see below.
//   k_pack_misc  policy bias padded to Np, value Linear as [pos][32], value bias.
#pragma once
#include "fpc_platform.h"
#include "../../include/fpc_engine.h"

#include <string>
#include <vector>

namespace fpc {

// 16 bytes moved as one piece: a vector type in the product (one dwordx4 / b128 access, held in registers), a plain
// aligned struct on the emulator
#ifdef FPC_EMUL
struct alignas(16) PkChunk {
  uint32_t x, y, z, w;
};
#else
typedef uint32_t PkChunk __attribute__((ext_vector_type(4)));
#endif

// f32 -> bf16 (dt 0) / fp16 (dt 1), round to nearest even, subnormals kept: torch's .to(bfloat16) / .to(float16).
// The product uses the hardware conversion, the emulator build (g++ has neither __bf16 nor _Float16 arithmetic) integer
// arithmetic; both are held to torch by the byte comparisons of tests/test_weights_device_*.py.
#ifdef FPC_EMUL
inline uint16_t pk_cvt16(float f, int dt) {
  uint32_t x;
  memcpy(&x, &f, 4);
  if (dt == 0) {
    if ((x & 0x7fffffffu) > 0x7f800000u) return (uint16_t)((x >> 16) | 0x0040u);   // NaN stays a (quiet) NaN
    return (uint16_t)((x + 0x7fffu + ((x >> 16) & 1u)) >> 16);
  }
  const uint32_t sign = (x >> 16) & 0x8000u;
  x &= 0x7fffffffu;
  if (x > 0x7f800000u) return (uint16_t)(sign | 0x7e00u);
  if (x >= 0x477ff000u) return (uint16_t)(sign | 0x7c00u);           // 65520 and above (infinity included) round to infinity
  if (x >= 0x38800000u) {                                            // normal in fp16 (2^-14 and above)
    const uint32_t y = x - 0x38000000u;
    return (uint16_t)(sign | ((y + 0xfffu + ((y >> 13) & 1u)) >> 13));
  }
  const int e = (int)(x >> 23);
  if (e < 102) return (uint16_t)sign;                                // below 2^-25: zero
  const uint32_t m = (x & 0x7fffffu) | 0x800000u;
  const int s = 126 - e;                                             // 14..24: the result counts units of 2^-24
  uint32_t q = m >> s;
  const uint32_t rem = m & ((1u << s) - 1u), half = 1u << (s - 1);
  if (rem > half || (rem == half && (q & 1u))) ++q;                  // may carry into the smallest normal: the right encoding
  return (uint16_t)(sign | q);
}
#else
__device__ __forceinline__ uint16_t pk_cvt16(float f, int dt) {
  if (dt == 0) { const __bf16 h = (__bf16)f; return __builtin_bit_cast(uint16_t, h); }
  const _Float16 h = (_Float16)f;
  return __builtin_bit_cast(uint16_t, h);
}
#endif

__device__ __forceinline__ PkChunk pk_pack8(const float *v, int dt) {
  return PkChunk{(uint32_t)pk_cvt16(v[0], dt) | ((uint32_t)pk_cvt16(v[1], dt) << 16), (uint32_t)pk_cvt16(v[2], dt) | ((uint32_t)pk_cvt16(v[3], dt) << 16),
                 (uint32_t)pk_cvt16(v[4], dt) | ((uint32_t)pk_cvt16(v[5], dt) << 16), (uint32_t)pk_cvt16(v[6], dt) | ((uint32_t)pk_cvt16(v[7], dt) << 16)};
}

// ---- k_pack_conv ---------------------------------------------------------------------------------------------------
struct PackConv {      // one Conv2d(3x3) + BatchNorm2d -> one blob section pair; device pointers
  const float *w, *b, *g, *beta, *mean, *var;   // b nullable
  float eps;
  int cin, cout, cin_pad, cout_pad;
  uint16_t *w16;       // [9][cout_pad][cin_pad]
  float *b32;          // [cout_pad]
};

constexpr int PK_THREADS = 256;

// blocks [conv * bpc, (conv + 1) * bpc) share convolution `conv`; one item = 8 consecutive input channels of one
// (tap, output channel) = one 16-byte store, padding included
__global__ void __launch_bounds__(PK_THREADS) k_pack_conv(const PackConv *tab, int bpc, int dt) {
  const PackConv d = tab[blockIdx.x / bpc];
  const int j = blockIdx.x % bpc, c8n = d.cin_pad / 8;
  const int items = 9 * d.cout_pad * c8n;
  for (int it = j * PK_THREADS + (int)threadIdx.x; it < items; it += bpc * PK_THREADS) {
    const int c8 = it % c8n, co = (it / c8n) % d.cout_pad, tap = it / (c8n * d.cout_pad);
    float v[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    if (co < d.cout) {
      const float s = d.g[co] / sqrtf(d.var[co] + d.eps);
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const int ci = c8 * 8 + e;
        if (ci < d.cin) v[e] = d.w[((size_t)co * d.cin + ci) * 9 + tap] * s;
      }
      if (tap == 0 && c8 == 0) {
        const float t = ((d.b ? d.b[co] : 0.f) - d.mean[co]) * s;
        d.b32[co] = t + d.beta[co];
      }
    } else if (tap == 0 && c8 == 0) {
      d.b32[co] = 0.f;
    }
    *reinterpret_cast<PkChunk *>(d.w16 + ((size_t)tap * d.cout_pad + co) * d.cin_pad + c8 * 8) = pk_pack8(v, dt);
  }
}

// ---- k_pack_fc -----------------------------------------------------------------------------------------------------
// Destination element (ks, nt, q, c, e) of [Kp/32][Np/16][64 lanes = 16 q + c][8] is W'[nt*16 + c][ks*32 + q*8 + e] with
// W'[n][pos*A_ch + ch] = W[n][ch*RR + pos], zero for n >= A or k' >= A.  A_ch = 8 (R + 1) is a multiple of 8, so a lane's
// 16 bytes are eight consecutive channels of ONE position -- RR floats apart in the source.
// One block = one tile of 16 rows x one chunk of 16 positions (16 positions x A_ch = whole 32-deep k-steps):
//   in   item (row, channel octet, position), position fastest: 8 loads per thread, each a 64-byte segment per 16 lanes,
//        all eight in flight; converted on the way in and stored as ONE 16-byte LDS write at [row][position][channel]
//        (61 KB of LDS as 16-bit at 14x14; f32 would not fit twice on a CU).  Consecutive positions are A_ch * 2 bytes =
//        R + 1 sixteen-byte slots apart: an odd count on the even boards, so 16 lanes hit 16 different slots.
//   out  wave w writes the chunk's k-steps w, w + 4, ...: each a 1 KiB fragment, one 16-byte store per lane; lane (q, c)
//        reads [row c][k' - chunk start .. + 8].  Rows are padded by 16 bytes so the 16 rows of a quarter wave fall into
//        16 different slots.
// The last chunk of a tile (RR tail: 4 positions at 14x14, 1 at 9x9) also writes the zero k-steps up to Kp; tiles past A
// write zeros only.  Every byte of the destination is written: the in-place path overwrites a live buffer.
// Block b = tile * chunks + chunk: the chunks of one tile run together, so both halves of a 128-byte line are used while
// it is in the cache.
constexpr int PK_PC = 16, PK_ROWS = 16, PK_MAXCH = 120;
constexpr int PK_TILE = PK_ROWS * (PK_PC * PK_MAXCH + 8);

__global__ void __launch_bounds__(PK_THREADS) k_pack_fc(const float *W, int A, int A_ch, int RR, int Np, int Kp, int dt, uint16_t *dst) {
  __shared__ __attribute__((aligned(16))) uint16_t tile[PK_TILE];
  const int tid = (int)threadIdx.x;
  const int nchunks = (RR + PK_PC - 1) / PK_PC;
  const int nt = (int)blockIdx.x / nchunks, chunk = (int)blockIdx.x % nchunks;
  const int p0 = chunk * PK_PC, pcv = RR - p0 < PK_PC ? RR - p0 : PK_PC;
  const int n0 = nt * PK_ROWS, rs = PK_PC * A_ch + 8, c8n = A_ch / 8;
  if (n0 < A) {
    const int nitems = PK_ROWS * c8n * PK_PC;
    for (int it = tid; it < nitems; it += PK_THREADS) {
      const int p = it & (PK_PC - 1), c8 = (it / PK_PC) % c8n, row = (it / PK_PC) / c8n;
      float v[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
      if (p < pcv && n0 + row < A) {
        const float *s = W + (size_t)(n0 + row) * A + (size_t)(c8 * 8) * RR + p0 + p;
#pragma unroll
        for (int e = 0; e < 8; ++e) v[e] = s[(size_t)e * RR];
      }
      *reinterpret_cast<PkChunk *>(tile + row * rs + p * A_ch + c8 * 8) = pk_pack8(v, dt);
    }
  }
  __syncthreads();
  const int ks0 = p0 * A_ch / 32, ks1 = chunk == nchunks - 1 ? Kp / 32 : (p0 + PK_PC) * A_ch / 32;
  const int wave = tid >> 6, lane = tid & 63, q = lane >> 4, c = lane & 15;
  for (int ks = ks0 + wave; ks < ks1; ks += PK_THREADS / 64) {
    const int k = ks * 32 + q * 8;
    PkChunk o{0u, 0u, 0u, 0u};
    if (k < A && n0 + c < A) o = *reinterpret_cast<const PkChunk *>(tile + c * rs + (k - p0 * A_ch));
    *reinterpret_cast<PkChunk *>(dst + (((size_t)ks * (Np / 16) + nt) * 64 + lane) * 8) = o;
  }
}

// ---- k_fc_rowmax + k_pack_fc8: the policy Linear as int8 with one f32 scale per output row --------------
// weights.quantize_fc op for op in f32 (the build has -ffp-contract=off and a correctly rounded divide; unlike the BN fold
// there is no square root, so the host export has no caveat):
//   m_n = max_k |w[n][k]|;  s_n = m_n / 127;  m_n < 127 * 2^-100 (zero included): s_n = 1;  q = clamp(rintf(w / s_n), -127, 127).
// k_fc_rowmax  one block per row of the padded matrix: s_n into a SCRATCH row of Np floats (1.0 for n >= A), and *bad = 1
//              if the row holds a non-finite weight -- the host looks at the flag before anything is written anywhere.
// k_pack_fc8   k_pack_fc's transpose on tiles of 32 rows, one byte per element, into the fragment-pair order
//              [Kp/32][Np/32][64 lanes = 16 q + c][2 tiles][8]: element (ks, np, q, c, t, e) = q8[32 np + 16 t + c][32 ks + 8 q + e];
//              a lane's 16-byte store holds the fragments of two column tiles.  The blocks of chunk 0 also write their 32
//              scales.  Every byte of both sections is written.
constexpr float PK_Q8_FLOOR = 127.f * 0x1p-100f;

__global__ void __launch_bounds__(PK_THREADS) k_fc_rowmax(const float *W, int A, float *scale, int *bad) {
  __shared__ float red[PK_THREADS / 64];
  __shared__ int redbad[PK_THREADS / 64];
  const int n = (int)blockIdx.x, tid = (int)threadIdx.x;
  float m = 0.f;
  int nf = 0;
  if (n < A)
    for (int k = tid; k < A; k += PK_THREADS) {
      const float a = fabsf(W[(size_t)n * A + k]);
      if (!(a < INFINITY)) nf = 1;      // infinity or NaN
      else if (a > m) m = a;
    }
  for (int off = 32; off >= 1; off >>= 1) {
    const float o = __shfl_xor(m, off);
    const int ob = __shfl_xor(nf, off);
    if (o > m) m = o;
    nf |= ob;
  }
  if ((tid & 63) == 0) { red[tid >> 6] = m; redbad[tid >> 6] = nf; }
  __syncthreads();
  if (tid == 0) {
    for (int w = 1; w < PK_THREADS / 64; ++w) { if (red[w] > m) m = red[w]; nf |= redbad[w]; }
    const float s = m / 127.f;
    scale[n] = (n >= A || m < PK_Q8_FLOOR) ? 1.f : s;
    if (nf) *bad = 1;
  }
}

__device__ __forceinline__ uint32_t pk_quant8(float w, float s) {
  float r = rintf(w / s);
  r = r < -127.f ? -127.f : r > 127.f ? 127.f : r;
  return (uint32_t)(int)r & 0xffu;
}

constexpr int PK_ROWS8 = 32;
constexpr int PK_TILE8 = PK_ROWS8 * (PK_PC * PK_MAXCH + 16);

__global__ void __launch_bounds__(PK_THREADS) k_pack_fc8(const float *W, const float *scale, int A, int A_ch, int RR, int Np, int Kp,
                                                         unsigned char *dst, float *dscale) {
  __shared__ __attribute__((aligned(16))) unsigned char tile[PK_TILE8];
  const int tid = (int)threadIdx.x;
  const int nchunks = (RR + PK_PC - 1) / PK_PC;
  const int np = (int)blockIdx.x / nchunks, chunk = (int)blockIdx.x % nchunks;
  const int p0 = chunk * PK_PC, pcv = RR - p0 < PK_PC ? RR - p0 : PK_PC;
  const int n0 = np * PK_ROWS8, rs = PK_PC * A_ch + 16, c8n = A_ch / 8;
  if (chunk == 0 && tid < PK_ROWS8) dscale[n0 + tid] = scale[n0 + tid];
  if (n0 < A) {
    const int nitems = PK_ROWS8 * c8n * PK_PC;
    for (int it = tid; it < nitems; it += PK_THREADS) {
      const int p = it & (PK_PC - 1), c8 = (it / PK_PC) % c8n, row = (it / PK_PC) / c8n;
      uint32_t lo = 0u, hi = 0u;
      if (p < pcv && n0 + row < A) {
        const float *s = W + (size_t)(n0 + row) * A + (size_t)(c8 * 8) * RR + p0 + p;
        const float sc = scale[n0 + row];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          lo |= pk_quant8(s[(size_t)e * RR], sc) << (8 * e);
          hi |= pk_quant8(s[(size_t)(e + 4) * RR], sc) << (8 * e);
        }
      }
      uint32_t *t = reinterpret_cast<uint32_t *>(tile + row * rs + p * A_ch + c8 * 8);
      t[0] = lo;
      t[1] = hi;
    }
  }
  __syncthreads();
  const int ks0 = p0 * A_ch / 32, ks1 = chunk == nchunks - 1 ? Kp / 32 : (p0 + PK_PC) * A_ch / 32;
  const int wave = tid >> 6, lane = tid & 63, q = lane >> 4, c = lane & 15;
  for (int ks = ks0 + wave; ks < ks1; ks += PK_THREADS / 64) {
    const int k = ks * 32 + q * 8;
    PkChunk o{0u, 0u, 0u, 0u};
    if (k < A) {
      if (n0 + c < A) {
        const uint32_t *t = reinterpret_cast<const uint32_t *>(tile + c * rs + (k - p0 * A_ch));
        o.x = t[0]; o.y = t[1];
      }
      if (n0 + 16 + c < A) {
        const uint32_t *t = reinterpret_cast<const uint32_t *>(tile + (16 + c) * rs + (k - p0 * A_ch));
        o.z = t[0]; o.w = t[1];
      }
    }
    *reinterpret_cast<PkChunk *>(dst + (((size_t)ks * (Np / 32) + np) * 64 + lane) * 16) = o;
  }
}

// ---- k_pack_misc: fcb f32[Np] (zero past A), vw f32[RR][32] (channels 24..31 zero), the value bias -------------------
__global__ void __launch_bounds__(PK_THREADS) k_pack_misc(const float *fc_b, const float *vfc_w, const float *vfc_b, int A, int RR, int Np,
                                                          int nblk, float *fcb, float *vw, float *vb) {
  const int total = Np + RR * 32 + 1;
  for (int i = (int)blockIdx.x * PK_THREADS + (int)threadIdx.x; i < total; i += nblk * PK_THREADS) {
    if (i < Np) fcb[i] = i < A ? fc_b[i] : 0.f;
    else if (i < Np + RR * 32) {
      const int j = i - Np, pos = j >> 5, ch = j & 31;
      vw[j] = ch < 24 ? vfc_w[ch * RR + pos] : 0.f;
    } else *vb = vfc_b[0];
  }
}

// ---- host side -------------------------------------------------------------------------------------------------------
constexpr int PK_FCW_COLS = 384, PK_FCW_MAXSPLIT = 8;   // k_fcw's column group and its largest K-split (fpc_fc.h / fpc_nn.h)

// K-splits k_fcw uses for [Np][Kp] on a part with `cus` CUs, 0 if it has no one-round split (weights.py: fcw_split)
inline int pk_plan_fcw(int Np, int Kp, int cus) {
  const int groups = Np / PK_FCW_COLS, stages = Kp / 64;
  int best = 0;
  for (int sk = 1; sk <= PK_FCW_MAXSPLIT && groups * sk <= cus; ++sk)
    if (stages % sk == 0 && stages / sk >= 4) best = sk;
  return best;
}

// the shapes the engine runs: the host blob's header (NN::load) and the device pack's descriptor are both held to this
// (wtype: the policy Linear's weight type, 0 = 16 bit, 1 = int8 -- the latter only on fp16 operands and layout 2)
inline int pk_check_geom(int F, int nblocks, int Np, int Kp, int layout, int wtype, int dtype, int A, int cus, int *split, std::string *err) {
  if (wtype < 0 || wtype > 1) { *err = "unknown policy-Linear weight type (fc_wtype: 0 = 16 bit, 1 = int8)"; return FPC_EWEIGHTS; }
  if (wtype == 1 && (layout != 2 || dtype != 1)) {
    *err = "int8 policy-Linear weights (fc_wtype 1) exist only for fp16 operands and fc_layout 2 (k_fcw8), not for bf16 or fc_layout 1";
    return FPC_EWEIGHTS;
  }
  if (layout < 1 || layout > 2) { *err = "unknown policy-Linear weight layout in weight blob (1 = k_fc16, 2 = k_fcw)"; return FPC_EWEIGHTS; }
  if (F % 64 || F < 64 || F > 512 || nblocks < 0 || Np % (layout == 2 ? PK_FCW_COLS : 256) || Kp % 512 || Kp < 1024 || Np < A || Kp < A) {
    // every hidden width accepted here forwards (NN::launch_conv: 128 / 256 on the tower kernels, the rest on k_conv3x3 per
    // layer); a width without a kernel is refused here, at load, never by a later forward
    *err = "unsupported network shape in weight blob (hidden must be a multiple of 64 in 64..512, Np of 256 -- 384 for fc_layout 2 --, Kp of 512)";
    return FPC_EWEIGHTS;
  }
  *split = 0;
  if (layout == 2) {
    *split = pk_plan_fcw(Np, Kp, cus);
    if (!*split) { *err = "weight blob fc_layout 2 (k_fcw): no one-round K-split for this shape on this device; export with fc_layout 1"; return FPC_EWEIGHTS; }
  }
  return 0;
}

struct PackGeom {
  int R = 0, RR = 0, A = 0, A_ch = 0, F = 0, Fp = 0, nblocks = 0, Np = 0, Kp = 0, fc_layout = 0, dtype = 0, fcw_split = 0;
  int fc_wtype = 0;    // 0: 16-bit policy-Linear weights, 1: int8 + scales (FPC_FC_W8)
  int nconv() const { return 2 * nblocks + 3; }
  void conv_dims(int i, int *cin, int *cout, int *cin_pad, int *cout_pad) const {   // blob order: stem, c1[0], c2[0], ..., policy, value
    if (i == 0) { *cin = 24; *cout = F; *cin_pad = 32; *cout_pad = Fp; }
    else if (i <= 2 * nblocks) { *cin = F; *cout = F; *cin_pad = F; *cout_pad = Fp; }
    else { *cin = F; *cout = i == 2 * nblocks + 1 ? A_ch : 24; *cin_pad = F; *cout_pad = 128; }
  }
};

// where the sections go: a blob's section offsets, or the engine's live allocations
struct PackDst {
  std::vector<uint16_t *> cw;
  std::vector<float *> cb;
  uint16_t *fcw = nullptr;     // int8 bytes in pair order where the geometry's fc_wtype is 1
  float *fcb = nullptr, *vw = nullptr, *vb = nullptr;
  float *fcs = nullptr;        // fc_wtype 1: the scales f32[Np]
};

// byte offsets of the sections in a blob (64-byte aligned, blob order); returns the blob's size
inline uint64_t pk_blob_layout(const PackGeom &g, std::vector<uint64_t> *cw, std::vector<uint64_t> *cb, uint64_t *fcw, uint64_t *fcb,
                               uint64_t *vw, uint64_t *vb, uint64_t *fcs = nullptr) {
  uint64_t off = 64;
  auto take = [&](uint64_t bytes) { off = (off + 63) & ~63ull; const uint64_t at = off; off += bytes; return at; };
  for (int i = 0; i < g.nconv(); ++i) {
    int cin, cout, cin_pad, cout_pad;
    g.conv_dims(i, &cin, &cout, &cin_pad, &cout_pad);
    const uint64_t a = take((uint64_t)9 * cout_pad * cin_pad * 2), b = take((uint64_t)cout_pad * 4);
    if (cw) cw->push_back(a);
    if (cb) cb->push_back(b);
  }
  const uint64_t a = take((uint64_t)g.Np * g.Kp * (g.fc_wtype ? 1 : 2));
  const uint64_t s = g.fc_wtype ? take((uint64_t)g.Np * 4) : 0;      // version 4: the scales between the weights and the bias
  const uint64_t b = take((uint64_t)g.Np * 4), c = take((uint64_t)g.RR * 32 * 4), d = take(4);
  if (fcw) *fcw = a;
  if (fcs) *fcs = s;
  if (fcb) *fcb = b;
  if (vw) *vw = c;
  if (vb) *vb = d;
  return off;
}

}  // namespace fpc
