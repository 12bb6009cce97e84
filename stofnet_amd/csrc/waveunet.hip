// Wave-U-Net (the reference's models/wave_unet.py, `main.py model=unet`) on gfx950, inference only, exact fp32
// (v_mfma_f32_16x16x4_f32).  channels_interval = 16, n = n_layers in 1 .. 12, L a multiple of 2^n; L_i = L / 2^i.
//
//   x [N, 1, L] -> encoder i = 0 .. n-1: conv 16 i (1 for i = 0) -> 16 (i + 1), k 15, pad 7 + BN + LeakyReLU(0.1) = skip i
//                  at length L_i; the next level reads every second position of it
//               -> middle: conv 16 n -> 16 n, k 15, pad 7 + BN + LeakyReLU(0.1) at length L_n               (= bottleneck)
//               -> decoder i = 0 .. n-1: x2 linear interpolation (align_corners) of the previous output, concatenated with
//                  skip n-1-i, conv -> 16 (n - i), k 5, pad 2 + BN + LeakyReLU(0.1) at length L_(n-1-i)
//               -> out: tanh(w[0:16] . o + w[16] x + b)                                                     -> y [N, 1, L]
// BatchNorm (eval mode) is folded into the convolution by the host packer in double: s = gamma / sqrt(var + 1e-5),
// w' = w s, b' = (b - mean) s + beta, both rounded to fp32 once.
//
// Activations are dense channel-last fp32, act[n][t][C], so the K span (tap, channel) of one output is contiguous.
//
// The kernels live in waveunet_net.h (shared with the training kernels of waveunet_train.hip); this file instantiates them with
// the inference epilogue and holds the blob layout, the host packer and the forward.
//
//   wu_in_kernel     encoder 0 (Cin = 1) on the vector pipe, one thread per (position, 4 channels): folded bias, then taps
//                    0 .. 14 as one fma chain, LeakyReLU.
//   wu_conv_kernel   every other convolution as an implicit GEMM, templated on the tap count (15 | 5), the A source and
//                    the N tiles per wave.  A work-group owns TM = 64 positions of one waveform and NTW N tiles of 16
//                    output channels (blockIdx.y picks the group of N tiles); wave w owns positions 16 w .. 16 w + 15.
//                    The input window (TM + taps - 1 positions x up to 192 channels) is built once in LDS and all taps
//                    read it:
//                      encoder source  window position u holds prev[n][2 u][:]: the decimation is the stride of the load
//                      decoder source  channels [0, Cu) hold l0 low[n][i0][c] + l1 low[n][i1][c], channels [Cu, Cu + Cs)
//                                      hold skip[n][u][c]; neither the interpolated nor the concatenated map reaches HBM
//                    and positions outside [0, L_out) are zero (the padding, per waveform).  Wider inputs (decoders of
//                    n >= 7) take a second pass over channels 192 .. Cin into the same accumulators.  Epilogue: folded
//                    bias, LeakyReLU as v > 0 ? v : 0.1 v (keeps NaN).
//                    The interpolation coordinates are ATen's fp32 ones: scale = float(M - 1) / float(2 M - 1) from the
//                    host, r = scale * float(u) as a multiply of its own (no contraction), i0 = (int) r clamped to M - 1,
//                    i1 = min(i0 + 1, M - 1), l1 = r - i0 clamped to [0, 1], l0 = 1 - l1.
//   wu_head_kernel   the 17 -> 1 output convolution and tanhf on the vector pipe, one thread per sample; the logits
//                    before the tanh go to an optional second pointer.
//
// Every output element is one fixed-order chain (MFMA k order, fixed fma loops, no atomics) inside a tile that is fixed
// by (row, position), so a row's result does not depend on its batch, its chunk or its position there.
//
// ---- packed blob (floats; every section starts on a 256-byte boundary) -------------------------------------------------
//   enc0  [16][16]             rows 0 .. 14 = w'[c][0][tap] as [tap][c], row 15 = b'
//   then for each GEMM convolution in the order encoder 1 .. n-1, middle, decoder 0 .. n-1:
//     frag [NTP][G][64][4]     NTP = N tiles padded to a multiple of NTW (tiles >= Cout / 16 are zero), G = taps Cin / 16
//     bias [16 NTP]            b', zero from Cout on
//   head  [18]                 out.0.weight[0][0 .. 16][0], out.0.bias
//   NTW(T = Cout / 16) = T for T <= 4, else 4 when T % 4 == 0 or T % 3 != 0, else 3.
//   Fragment order: lane l (j = l & 15, q = l >> 4), element e of K group g of N tile t holds W'[16 t + j][k] where group
//   g covers, for the channel pass c0 (0, then 192 when Cin > 192; width cw = min(192, Cin - c0)), tap d and 16-channel
//   block b in that nesting order, the input channels c0 + 16 b .. + 15 of tap d, and k = channel c0 + 16 b + 4 q + e
//   of tap d (= weight[16 t + j][channel][d]).
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdlib.h>
#include <string.h>
#include "mfma32_frag.h"
#include "stof_common.h"
#include "waveunet_net.h"

namespace {

using namespace stof_frag;

bool wu_desc_ok(const stof_waveunet_desc* d) {
    return d && d->channels_interval == CI && d->n_layers >= 1 && d->n_layers <= MAX_LAYERS;
}

struct WuConv {
    int taps, cin, cout, cu;               // cu: interpolated channels of a decoder (the first cu of cin), 0 otherwise
    int ntw, ntp, groups;
    int64_t frag, bias;                    // float offsets into the blob
};

struct WuLayout {
    int nconv;                             // 2 n: encoder 1 .. n-1, middle, decoder 0 .. n-1
    WuConv conv[2 * MAX_LAYERS];
    int64_t enc0, head, total;
};

WuLayout wu_layout(const stof_waveunet_desc* d) {
    const int n = d->n_layers;
    WuLayout o{};
    int64_t at = 0;
    o.enc0 = at; at = align_up(at + 16 * CI);
    int k = 0;
    auto add = [&](int taps, int cin, int cout, int cu) {
        WuConv& c = o.conv[k++];
        c.taps = taps; c.cin = cin; c.cout = cout; c.cu = cu;
        const int tiles = cout / 16;
        c.ntw = wu_ntw(tiles);
        c.ntp = (tiles + c.ntw - 1) / c.ntw * c.ntw;
        c.groups = taps * cin / 16;
        c.frag = at; at += (int64_t)c.ntp * c.groups * 256;
        c.bias = at; at = align_up(at + 16 * c.ntp);
    };
    for (int i = 1; i < n; ++i) add(ENC_TAPS, CI * i, CI * (i + 1), 0);
    add(ENC_TAPS, CI * n, CI * n, 0);
    for (int i = 0; i < n; ++i) {
        const int cu = i == 0 ? CI * n : CI * (n - i + 1), cs = CI * (n - i);
        add(DEC_TAPS, cu + cs, cs, cu);
    }
    o.nconv = k;
    o.head = at; at = align_up(at + CI + 2);
    o.total = at;
    return o;
}

// Workspace (floats): skip i [N, L_i, 16 (i + 1)], middle [N, L_n, 16 n], two decoder buffers [N, L, 16] (decoder i
// writes L_(n-1-i) x 16 (n - i) <= L x 16 floats per row).
struct WuWorkspace {
    int64_t skip[MAX_LAYERS], mid, dec[2], total;
};

WuWorkspace wu_workspace(int n, int64_t N, int64_t L) {
    WuWorkspace w{};
    int64_t at = 0;
    for (int i = 0; i < n; ++i) { w.skip[i] = at; at = align_up(at + N * (L >> i) * CI * (i + 1)); }
    w.mid = at; at = align_up(at + N * (L >> n) * CI * n);
    for (int j = 0; j < 2; ++j) { w.dec[j] = at; at = align_up(at + N * L * CI); }
    w.total = at;
    return w;
}

bool wu_shape_ok(const stof_waveunet_desc* d, int64_t L) {
    return L >= 1 && L % ((int64_t)1 << d->n_layers) == 0;
}

}  // namespace

extern "C" size_t stof_waveunet_packed_bytes(const stof_waveunet_desc* desc) {
    if (!wu_desc_ok(desc)) return 0;
    return (size_t)wu_layout(desc).total * sizeof(float);
}

extern "C" int stof_waveunet_pack_weights(const stof_waveunet_desc* desc, const float* const* params, void* out,
                                          size_t out_bytes) {
    if (!wu_desc_ok(desc) || !params || !out) return STOF_ERR_BAD_ARG;
    const int n = desc->n_layers, np = 6 * (2 * n + 1) + 2;
    for (int i = 0; i < np; ++i)
        if (!params[i]) return STOF_ERR_BAD_ARG;
    const WuLayout o = wu_layout(desc);
    if (out_bytes < (size_t)o.total * sizeof(float)) return STOF_ERR_WORKSPACE;
    float* const blob = static_cast<float*>(out);
    memset(blob, 0, (size_t)o.total * sizeof(float));
    // block b of the state dict (encoder 0 .. n-1, middle, decoder 0 .. n-1): conv weight, conv bias, BN weight, BN bias,
    // running mean, running var.  Folded weight [oc][cin][taps] and bias in fp32, from double.
    auto fold = [&](int b, int cout, int per_oc, float* w, float* bias) {
        const float* const* p = params + 6 * b;
        for (int oc = 0; oc < cout; ++oc) {
            const double s = (double)p[2][oc] / sqrt((double)p[5][oc] + 1e-5);
            for (int k = 0; k < per_oc; ++k) w[(int64_t)oc * per_oc + k] = (float)((double)p[0][(int64_t)oc * per_oc + k] * s);
            bias[oc] = (float)(((double)p[1][oc] - (double)p[4][oc]) * s + (double)p[3][oc]);
        }
    };
    float* w = static_cast<float*>(malloc(sizeof(float) * (CI * MAX_LAYERS) * (2 * CI * MAX_LAYERS) * ENC_TAPS));
    if (!w) return STOF_ERR_WORKSPACE;
    float b0[CI * MAX_LAYERS];
    fold(0, CI, ENC_TAPS, w, b0);
    for (int c = 0; c < CI; ++c) {
        for (int j = 0; j < ENC_TAPS; ++j) blob[o.enc0 + j * CI + c] = w[c * ENC_TAPS + j];
        blob[o.enc0 + 15 * CI + c] = b0[c];
    }
    for (int k = 0; k < o.nconv; ++k) {
        const WuConv& c = o.conv[k];
        fold(k + 1, c.cout, c.cin * c.taps, w, blob + c.bias);
        float* frag = blob + c.frag;
        int g = 0;
        for (int c0 = 0; c0 < c.cin; c0 += CHUNK) {
            const int cw = c.cin - c0 < CHUNK ? c.cin - c0 : CHUNK;
            for (int tap = 0; tap < c.taps; ++tap)
                for (int blk = 0; blk < cw / 16; ++blk, ++g)
                    for (int nt = 0; nt < c.cout / 16; ++nt)
                        for (int lane = 0; lane < 64; ++lane)
                            for (int e = 0; e < 4; ++e) {
                                const int oc = 16 * nt + (lane & 15), ch = c0 + 16 * blk + 4 * (lane >> 4) + e;
                                frag[(((int64_t)nt * c.groups + g) * 64 + lane) * 4 + e] = w[((int64_t)oc * c.cin + ch) * c.taps + tap];
                            }
        }
    }
    free(w);
    const float* wo = params[np - 2];
    for (int c = 0; c <= CI; ++c) blob[o.head + c] = wo[c];
    blob[o.head + CI + 1] = params[np - 1][0];
    return STOF_OK;
}

extern "C" size_t stof_waveunet_workspace_bytes(const stof_waveunet_desc* desc, int64_t N, int64_t L) {
    if (!wu_desc_ok(desc) || N <= 0 || !wu_shape_ok(desc, L)) return 0;
    return (size_t)wu_workspace(desc->n_layers, N, L).total * sizeof(float);
}

extern "C" int stof_waveunet_forward(const stof_waveunet_desc* desc, const float* x, int64_t N, int64_t L, const void* packed,
                                     float* y, float* bottleneck, float* logits, void* workspace, size_t workspace_bytes,
                                     void* stream) {
    if (!wu_desc_ok(desc) || N < 0 || !wu_shape_ok(desc, L)) return STOF_ERR_BAD_ARG;
    if (N == 0) return STOF_OK;
    if (!x || !packed || !y || !workspace) return STOF_ERR_BAD_ARG;
    if (L >= (1ll << 31) || N >= (1ll << 31) || N * L >= (1ll << 31) - 64) return STOF_ERR_UNSUPPORTED;   // grid sizes
    const int n = desc->n_layers;
    const WuWorkspace ws = wu_workspace(n, N, L);
    if (workspace_bytes < (size_t)ws.total * sizeof(float)) return STOF_ERR_WORKSPACE;
    const WuLayout o = wu_layout(desc);
    const float* const blob = static_cast<const float*>(packed);
    float* const base = static_cast<float*>(workspace);
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int64_t M = N * L;

    hipLaunchKernelGGL(wu_in_kernel<true>, dim3((unsigned)((M * 4 + 255) / 256)), dim3(256), 0, s, x, (long long)M, (long long)L,
                       blob + o.enc0, base + ws.skip[0]);
    if (hipGetLastError() != hipSuccess) return STOF_ERR_HIP;

    auto conv = [&](const WuConv& c, const float* src, const float* low, float* out, int64_t Lout) {
        WuConvArgs a{};
        a.src = src; a.low = low; a.out = out;
        a.frag = reinterpret_cast<const float4*>(blob + c.frag);
        a.bias = blob + c.bias;
        a.Lout = Lout;
        a.Cin = c.cin; a.Cu = c.cu; a.Cout = c.cout;
        dim3 grid;
        size_t lds;
        wu_conv_geometry(a, c.taps, N, c.ntw, c.ntp, grid, lds);
        if (c.cu) wu_launch_conv<DEC_TAPS, SRC_DECODER, true>(c.ntw, grid, lds, s, a);
        else wu_launch_conv<ENC_TAPS, SRC_DECIMATED, true>(c.ntw, grid, lds, s, a);
        return hipGetLastError() == hipSuccess;
    };

    int k = 0;
    for (int i = 1; i < n; ++i, ++k)
        if (!conv(o.conv[k], base + ws.skip[i - 1], nullptr, base + ws.skip[i], L >> i)) return STOF_ERR_HIP;
    float* const mid = bottleneck ? bottleneck : base + ws.mid;
    if (!conv(o.conv[k++], base + ws.skip[n - 1], nullptr, mid, L >> n)) return STOF_ERR_HIP;
    const float* low = mid;
    for (int i = 0; i < n; ++i, ++k) {
        float* const out = base + ws.dec[i & 1];
        if (!conv(o.conv[k], base + ws.skip[n - 1 - i], low, out, L >> (n - 1 - i))) return STOF_ERR_HIP;
        low = out;
    }
    hipLaunchKernelGGL(wu_head_kernel, dim3((unsigned)((M + 255) / 256)), dim3(256), 0, s, low, x, (long long)M, blob + o.head,
                       blob + o.head + CI + 1, y, logits);
    return hipGetLastError() == hipSuccess ? STOF_OK : STOF_ERR_HIP;
}
