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

namespace {

using namespace stof_frag;

constexpr int CI = 16;                     // channels_interval
constexpr int MAX_LAYERS = 12;
constexpr int TM = 64;                     // positions per work-group of wu_conv_kernel
constexpr int CHUNK = 192;                 // channels per LDS pass
constexpr int ENC_TAPS = 15, DEC_TAPS = 5;

bool wu_desc_ok(const stof_waveunet_desc* d) {
    return d && d->channels_interval == CI && d->n_layers >= 1 && d->n_layers <= MAX_LAYERS;
}

int wu_ntw(int tiles) {
    if (tiles <= 4) return tiles;
    return (tiles % 4 == 0 || tiles % 3 != 0) ? 4 : 3;
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

__device__ __forceinline__ float leaky(float v) { return v > 0.f ? v : 0.1f * v; }   // NaN takes the second arm and stays

// ATen's fp32 source coordinates of the x2 linear interpolation with align_corners.  Contraction is off here: r has to be
// the rounded product before i0 is subtracted (an fma would subtract from the exact one and move l1 by up to an ulp of r).
__device__ __forceinline__ void wu_coords(float scale, int u, int M, int& i0, int& i1, float& l0, float& l1) {
#pragma clang fp contract(off)
    const float r = scale * (float)u;
    i0 = (int)r;
    if (i0 > M - 1) i0 = M - 1;
    i1 = i0 + 1 < M ? i0 + 1 : M - 1;
    l1 = r - (float)i0;
    l1 = l1 < 0.f ? 0.f : (l1 > 1.f ? 1.f : l1);
    l0 = 1.f - l1;
}

typedef float f32x4 __attribute__((ext_vector_type(4)));
#define MFMA16(a, b, acc) __builtin_amdgcn_mfma_f32_16x16x4f32((a), (b), (acc), 0, 0, 0)

// --------------------------------------------------------------------------------------------------------- encoder 0
// Thread o: flattened position m = o / 4 (m = n L + t), channels 4 (o % 4) .. + 3.
__global__ __launch_bounds__(256) void wu_in_kernel(const float* __restrict__ x, long long M, long long L,
                                                    const float* __restrict__ w, float* __restrict__ out) {
    const long long o = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (o >= M * 4) return;
    const long long m = o >> 2, t = m % L;
    const int c = 4 * (int)(o & 3);
    float4 acc = *reinterpret_cast<const float4*>(w + 15 * CI + c);
#pragma unroll
    for (int j = 0; j < ENC_TAPS; ++j) {
        const long long u = t + j - 7;
        const float xv = (u >= 0 && u < L) ? x[m + j - 7] : 0.f;
        const float4 wv = *reinterpret_cast<const float4*>(w + j * CI + c);
        acc.x = fmaf(wv.x, xv, acc.x);
        acc.y = fmaf(wv.y, xv, acc.y);
        acc.z = fmaf(wv.z, xv, acc.z);
        acc.w = fmaf(wv.w, xv, acc.w);
    }
    *reinterpret_cast<float4*>(out + m * CI + c) = make_float4(leaky(acc.x), leaky(acc.y), leaky(acc.z), leaky(acc.w));
}

// ------------------------------------------------------------------------------------------------- implicit-GEMM convs
struct WuConvArgs {
    const float* src;                      // encoder source: the previous level [N, 2 Lout, Cin]; decoder: the skip [N, Lout, Cin - Cu]
    const float* low;                      // decoder: the map to interpolate [N, Lout / 2, Cu]
    const float4* frag;
    const float* bias;
    float* out;                            // [N, Lout, Cout]
    long long Lout;
    int tiles;                             // work-groups per waveform
    int Cin, Cu, Cout, groups;
    float scale;                           // decoder: float(M - 1) / float(2 M - 1), M = Lout / 2
};

// blockIdx.x = (waveform n, tile of TM positions), blockIdx.y = group of NTW N tiles.  LDS window row j holds position
// t0 - PAD + j; lane (i = l & 15, q = l >> 4) of wave w reads rows 16 w + i + tap, channels 16 b + 4 q .. + 3.
// C/D map of the MFMA: channel = lane & 15, position = 4 (lane >> 4) + r.
template <int TAPS, bool DEC, int NTW>
__global__ __launch_bounds__(256) void wu_conv_kernel(const WuConvArgs a) {
    extern __shared__ __attribute__((aligned(16))) float win[];
    constexpr int PAD = TAPS / 2, ROWS = TM + TAPS - 1;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int i = lane & 15, q = lane >> 4;
    const long long n = blockIdx.x / a.tiles, t0 = (long long)(blockIdx.x % a.tiles) * TM;
    const long long Lout = a.Lout;
    const int nt0 = blockIdx.y * NTW;
    const bool active = t0 + 16 * wave < Lout;          // a wave past the end of the waveform only takes part in the staging
    const float4* bq = a.frag + (long long)nt0 * a.groups * 64 + lane;
    f32x4 acc[NTW] = {};
    int g = 0;
    for (int c0 = 0; c0 < a.Cin; c0 += CHUNK) {
        const int cw = a.Cin - c0 < CHUNK ? a.Cin - c0 : CHUNK, S = cw + 4, q4 = cw / 4;
        if (c0) __syncthreads();
        for (int idx = tid; idx < ROWS * q4; idx += 256) {
            const int j = idx / q4, cl = 4 * (idx - j * q4), c = c0 + cl;
            const long long u = t0 - PAD + j;
            float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
            if (u >= 0 && u < Lout) {
                if constexpr (!DEC) {
                    v = *reinterpret_cast<const float4*>(a.src + (n * 2 * Lout + 2 * u) * a.Cin + c);
                } else if (c < a.Cu) {
                    const long long M = Lout >> 1;
                    int i0, i1;
                    float l0, l1;
                    wu_coords(a.scale, (int)u, (int)M, i0, i1, l0, l1);
                    const float4 p0 = *reinterpret_cast<const float4*>(a.low + (n * M + i0) * a.Cu + c);
                    const float4 p1 = *reinterpret_cast<const float4*>(a.low + (n * M + i1) * a.Cu + c);
                    v = make_float4(l0 * p0.x + l1 * p1.x, l0 * p0.y + l1 * p1.y, l0 * p0.z + l1 * p1.z, l0 * p0.w + l1 * p1.w);
                } else {
                    const int Cs = a.Cin - a.Cu;
                    v = *reinterpret_cast<const float4*>(a.src + (n * Lout + u) * Cs + (c - a.Cu));
                }
            }
            *reinterpret_cast<float4*>(win + j * S + cl) = v;
        }
        __syncthreads();
        const int blocks = cw / 16;
        if (active) {
            const float* ap = win + (16 * wave + i) * S + 4 * q;
            for (int tap = 0; tap < TAPS; ++tap) {
                for (int b = 0; b < blocks; ++b, ++g) {
                    const float4 av = *reinterpret_cast<const float4*>(ap + tap * S + 16 * b);
                    float4 bv[NTW];
#pragma unroll
                    for (int nt = 0; nt < NTW; ++nt) bv[nt] = bq[((long long)nt * a.groups + g) * 64];
#pragma unroll
                    for (int nt = 0; nt < NTW; ++nt) acc[nt] = MFMA16(av.x, bv[nt].x, acc[nt]);
#pragma unroll
                    for (int nt = 0; nt < NTW; ++nt) acc[nt] = MFMA16(av.y, bv[nt].y, acc[nt]);
#pragma unroll
                    for (int nt = 0; nt < NTW; ++nt) acc[nt] = MFMA16(av.z, bv[nt].z, acc[nt]);
#pragma unroll
                    for (int nt = 0; nt < NTW; ++nt) acc[nt] = MFMA16(av.w, bv[nt].w, acc[nt]);
                }
            }
        }
    }
    if (!active) return;
#pragma unroll
    for (int nt = 0; nt < NTW; ++nt) {
        const int ch = 16 * (nt0 + nt) + i;
        if (ch >= a.Cout) continue;
        const float b = a.bias[ch];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const long long p = t0 + 16 * wave + 4 * q + r;
            if (p < Lout) a.out[(n * Lout + p) * a.Cout + ch] = leaky(acc[nt][r] + b);
        }
    }
}

// -------------------------------------------------------------------------------------------------------------- head
// Thread m = n L + t: bias, then the 16 decoder channels and x as one fma chain.
__global__ __launch_bounds__(256) void wu_head_kernel(const float* __restrict__ o, const float* __restrict__ x, long long M,
                                                      const float* __restrict__ w, float* __restrict__ y,
                                                      float* __restrict__ logits) {
    const long long m = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (m >= M) return;
    float acc = w[CI + 1];
#pragma unroll
    for (int c = 0; c < CI; c += 4) {
        const float4 v = *reinterpret_cast<const float4*>(o + m * CI + c);
        acc = fmaf(w[c], v.x, acc);
        acc = fmaf(w[c + 1], v.y, acc);
        acc = fmaf(w[c + 2], v.z, acc);
        acc = fmaf(w[c + 3], v.w, acc);
    }
    acc = fmaf(w[CI], x[m], acc);
    if (logits) logits[m] = acc;
    y[m] = tanhf(acc);
}

template <int TAPS, bool DEC, int NTW>
void launch_conv_ntw(dim3 grid, size_t lds, hipStream_t s, const WuConvArgs& a) {
    hipLaunchKernelGGL((wu_conv_kernel<TAPS, DEC, NTW>), grid, dim3(256), lds, s, a);
}

template <int TAPS, bool DEC>
void launch_conv(int ntw, dim3 grid, size_t lds, hipStream_t s, const WuConvArgs& a) {
    switch (ntw) {
        case 1: launch_conv_ntw<TAPS, DEC, 1>(grid, lds, s, a); break;
        case 2: launch_conv_ntw<TAPS, DEC, 2>(grid, lds, s, a); break;
        case 3: launch_conv_ntw<TAPS, DEC, 3>(grid, lds, s, a); break;
        default: launch_conv_ntw<TAPS, DEC, 4>(grid, lds, s, a); break;
    }
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

    hipLaunchKernelGGL(wu_in_kernel, dim3((unsigned)((M * 4 + 255) / 256)), dim3(256), 0, s, x, (long long)M, (long long)L,
                       blob + o.enc0, base + ws.skip[0]);
    if (hipGetLastError() != hipSuccess) return STOF_ERR_HIP;

    auto conv = [&](const WuConv& c, const float* src, const float* low, float* out, int64_t Lout) {
        WuConvArgs a{};
        a.src = src; a.low = low; a.out = out;
        a.frag = reinterpret_cast<const float4*>(blob + c.frag);
        a.bias = blob + c.bias;
        a.Lout = Lout;
        a.tiles = (int)((Lout + TM - 1) / TM);
        a.Cin = c.cin; a.Cu = c.cu; a.Cout = c.cout; a.groups = c.groups;
        const int64_t Mlow = Lout / 2;
        a.scale = c.cu ? (float)(Mlow - 1) / (float)(2 * Mlow - 1) : 0.f;
        const dim3 grid((unsigned)(N * a.tiles), (unsigned)(c.ntp / c.ntw));
        const int cw = c.cin < CHUNK ? c.cin : CHUNK;
        const size_t lds = sizeof(float) * (size_t)(TM + c.taps - 1) * (cw + 4);
        if (c.cu) launch_conv<DEC_TAPS, true>(c.ntw, grid, lds, s, a);
        else launch_conv<ENC_TAPS, false>(c.ntw, grid, lds, s, a);
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
    hipLaunchKernelGGL(wu_head_kernel, dim3((unsigned)((M + 255) / 256)), dim3(256), 0, s, low, x, (long long)M, blob + o.head, y,
                       logits);
    return hipGetLastError() == hipSuccess ? STOF_OK : STOF_ERR_HIP;
}
