// What kuleshov.hip (inference) and kuleshov_train.hip (training) share: the constants and lengths of the network, the
// implicit-GEMM convolution ks_conv_kernel, final_conv and output_fc.  The kernels are documented in kuleshov.hip; the
// inference instantiations (TRAIN = false) are the code that was there, instruction for instruction.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <string.h>
#include "mfma32_frag.h"
#include "stof_common.h"

namespace {

using namespace stof_frag;

constexpr int NL = 4;
constexpr int NF[NL] = {128, 256, 512, 512};
constexpr int FS[NL] = {65, 33, 17, 9};
constexpr int FS0 = 65;                         // taps of down_conv0 (= FS[0]; a scalar for device code)
constexpr int KB = 9;                           // bottleneck and final_conv taps
constexpr int C0 = 128;                         // width of down 0 and of final_conv's input
constexpr int UP_CIN[NL] = {512, 512, 512, 256};
constexpr int UP_COUT[NL] = {1024, 1024, 512, 256};
constexpr int UP_FS[NL] = {9, 17, 33, 65};
constexpr int MIN_L = 641;                      // shortest input for which every convolution has an output
constexpr int T0 = 64;                          // outputs per work-group of ks_down0_kernel
constexpr int XS0 = 2 * T0 + 64;                // its LDS window (2 (T0 - 1) + 65 samples, rounded up)
constexpr int FIN_T = 16;                       // positions per wave of ks_final_kernel
constexpr int QU_WIDE = 1, QU_MID = 2, QU_NARROW = 4;   // K groups per step of the 64 x 128, 32 x 128 and 32 x 32 wave tile
constexpr int FC_MT = 4;                        // M tiles (of 32 rows) per work-group of ks_fc_kernel
constexpr int NUM_PARAMS = 54;                  // see stof_kuleshov_pack_weights in include/stofnet_amd.h
enum { EP_DOWN = 0, EP_BOTT = 1, EP_UP = 2 };

struct Dims {
    int64_t L, O, D[NL], B, U[NL], Lc[NL], F, Kp, G, OT;
};

bool dims(const stof_kuleshov_desc* d, Dims* o) {
    if (!d || d->input_length < MIN_L || d->output_length < 1 || !std::isfinite(d->bn_eps) || d->bn_eps < 0.0) return false;
    if (d->tile_variant < 0 || d->tile_variant > 3) return false;
    if (d->input_length >= (1ll << 24) || d->output_length >= (1ll << 24)) return false;
    o->L = d->input_length;
    o->O = d->output_length;
    int64_t w = o->L;
    for (int i = 0; i < NL; ++i) {
        w = (w - FS[i]) / 2 + 1;
        o->D[i] = w;
    }
    o->B = (w - KB) / 2 + 1;
    w = o->B;
    for (int i = 0; i < NL; ++i) {
        o->U[i] = w - UP_FS[i] + 1;
        if (o->U[i] < 1) return false;
        w = 2 * o->U[i] + o->D[NL - 1 - i];
        o->Lc[i] = w;
    }
    o->F = w - KB + 1;
    o->Kp = (2 * o->F + 7) / 8 * 8;
    o->G = o->Kp / 8;
    o->OT = (o->O + 31) / 32;
    return true;
}

__device__ __forceinline__ float leaky(float v, float slope) { return v > 0.f ? v : slope * v; }   // NaN stays NaN

// ----------------------------------------------------------------------------------------------- the implicit GEMM
struct ConvArgs {
    const float* in;             // row 0 of waveform 0 of the input range
    long long in_n_stride;       // floats between waveforms
    float* out;                  // row 0 of waveform 0 of the output range (for EP_UP: of the concatenation buffer)
    long long out_n_stride;
    float* out2;                 // optional second copy of the output (the bottleneck tap), dense [N][Lout][Cout]
    const float4* frag;
    const float* ep;             // [3][Cout]
    unsigned M, Lout;            // M = N Lout
    int Cin, Cout, stride, G, mode;
    // training epilogue only (TRAIN = true; behind the inference fields, whose offsets stay)
    long long out_t_stride;      // floats between output positions
    const float* bias;           // [Cout] or NULL
    int slope01;                 // 1: store leaky0.01(acc + bias) (the down blocks' u), 0: acc + bias
};

// Wave (blockIdx.x, w) owns flattened outputs m0 .. m0 + 32 MT - 1 (m = n Lout + t) and N tiles blockIdx.y NTW .. + NTW - 1.
// Lane (i = l & 31, h = l >> 5) of M tile mt reads its own output's K span at k = 8 q + 4 h .. + 3; a step takes QU K
// groups, and the next step's operands are loaded before this step's MFMAs (the small tiles have few MFMAs per group
// and few waves per SIMD, so they keep more loads in flight).  Tail lanes compute a duplicate of output M - 1 and store
// nothing.  TRAIN, what training runs (the forward's z or u, and the data gradients on their own weight images): the same K loop
// with the training epilogue out[n][t] = sum (+ bias), optionally through leaky0.01, at out + n out_n_stride + t out_t_stride + c,
// and the K span summed in partial chains of CHAIN_GROUPS K groups, each added to a running total when it ends
// (a fixed order).  One fp32 chain over the 4352 .. 17408 products of a data gradient misses the backward kernels' 2e-6 bound
// (measured 2.3e-6 at 4352), and in the forward it flips several times as many near-zero leaky-ReLU decisions as the
// reference's blocked sums do.
constexpr int CHAIN_GROUPS = 8;                  // K groups (of 8 products) per partial chain of the training convolutions
template <int MT, int NTW, int QU, bool TRAIN = false>
__global__ __launch_bounds__(256) void ks_conv_kernel(const ConvArgs p) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const unsigned m0 = ((unsigned)blockIdx.x * 4 + wave) * (32 * MT);
    if (m0 >= p.M) return;
    const int i = lane & 31, h = lane >> 5;
    const int G = p.G;                                  // a multiple of 16 (Cin >= 128), so of QU
    const float* a[MT];
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) {
        unsigned m = m0 + 32 * mt + i;
        if (m >= p.M) m = p.M - 1;
        const unsigned n = m / p.Lout, t = m - n * p.Lout;
        a[mt] = p.in + (long long)n * p.in_n_stride + (long long)t * p.stride * p.Cin + 4 * h;
    }
    const int nt0 = blockIdx.y * NTW;
    const float4* bq = p.frag + (long long)nt0 * G * 64 + lane;
    f32x16 acc[MT][NTW] = {};
    f32x16 total[TRAIN ? MT : 1][TRAIN ? NTW : 1] = {};
    float4 av[QU][MT], bv[QU][NTW];
#pragma unroll
    for (int u = 0; u < QU; ++u) {
#pragma unroll
        for (int mt = 0; mt < MT; ++mt) av[u][mt] = *reinterpret_cast<const float4*>(a[mt] + 8 * u);
#pragma unroll
        for (int nt = 0; nt < NTW; ++nt) bv[u][nt] = bq[((long long)nt * G + u) * 64];
    }
    for (int q = 0; q < G; q += QU) {
        float4 ca[QU][MT], cb[QU][NTW];
#pragma unroll
        for (int u = 0; u < QU; ++u) {
#pragma unroll
            for (int mt = 0; mt < MT; ++mt) ca[u][mt] = av[u][mt];
#pragma unroll
            for (int nt = 0; nt < NTW; ++nt) cb[u][nt] = bv[u][nt];
        }
        if (q + QU < G) {
#pragma unroll
            for (int u = 0; u < QU; ++u) {
#pragma unroll
                for (int mt = 0; mt < MT; ++mt) av[u][mt] = *reinterpret_cast<const float4*>(a[mt] + 8 * (q + QU + u));
#pragma unroll
                for (int nt = 0; nt < NTW; ++nt) bv[u][nt] = bq[((long long)nt * G + q + QU + u) * 64];
            }
        }
#pragma unroll
        for (int u = 0; u < QU; ++u) {
#pragma unroll
            for (int mt = 0; mt < MT; ++mt)
#pragma unroll
                for (int nt = 0; nt < NTW; ++nt) acc[mt][nt] = MFMA32(ca[u][mt].x, cb[u][nt].x, acc[mt][nt]);
#pragma unroll
            for (int mt = 0; mt < MT; ++mt)
#pragma unroll
                for (int nt = 0; nt < NTW; ++nt) acc[mt][nt] = MFMA32(ca[u][mt].y, cb[u][nt].y, acc[mt][nt]);
#pragma unroll
            for (int mt = 0; mt < MT; ++mt)
#pragma unroll
                for (int nt = 0; nt < NTW; ++nt) acc[mt][nt] = MFMA32(ca[u][mt].z, cb[u][nt].z, acc[mt][nt]);
#pragma unroll
            for (int mt = 0; mt < MT; ++mt)
#pragma unroll
                for (int nt = 0; nt < NTW; ++nt) acc[mt][nt] = MFMA32(ca[u][mt].w, cb[u][nt].w, acc[mt][nt]);
        }
        if constexpr (TRAIN) {
            if ((q + QU) % CHAIN_GROUPS == 0 || q + QU >= G) {
#pragma unroll
                for (int mt = 0; mt < MT; ++mt)
#pragma unroll
                    for (int nt = 0; nt < NTW; ++nt) {
                        total[mt][nt] += acc[mt][nt];
                        acc[mt][nt] = f32x16{};
                    }
            }
        }
    }
    // C/D map: column (channel) = lane & 31, row (output) = (r & 3) + 8 (r >> 2) + 4 h
    const int Cout = p.Cout;
    if constexpr (TRAIN) {
#pragma unroll
        for (int nt = 0; nt < NTW; ++nt) {
            const int c = 32 * (nt0 + nt) + i;
            const float b = p.bias ? p.bias[c] : 0.f;
#pragma unroll
            for (int mt = 0; mt < MT; ++mt) {
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const unsigned row = m0 + 32 * mt + (r & 3) + 8 * (r >> 2) + 4 * h;
                    if (row >= p.M) continue;
                    const unsigned rn = row / p.Lout, rt = row - rn * p.Lout;
                    const float v = total[mt][nt][r] + b;
                    p.out[(long long)rn * p.out_n_stride + (long long)rt * p.out_t_stride + c] = p.slope01 ? leaky(v, 0.01f) : v;
                }
            }
        }
        return;
    }
#pragma unroll
    for (int nt = 0; nt < NTW; ++nt) {
        const int c = 32 * (nt0 + nt) + i;
        const float b = p.ep[c], s = p.ep[Cout + c], t = p.ep[2 * Cout + c];
#pragma unroll
        for (int mt = 0; mt < MT; ++mt) {
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const unsigned row = m0 + 32 * mt + (r & 3) + 8 * (r >> 2) + 4 * h;
                if (row >= p.M) continue;
                const unsigned rn = row / p.Lout, rt = row - rn * p.Lout;
                float* const o = p.out + (long long)rn * p.out_n_stride;
                const float v = acc[mt][nt][r];
                if (p.mode == EP_UP) {
                    o[(long long)(2 * rt + (c & 1)) * (Cout >> 1) + (c >> 1)] = fmaf(v, s, t);
                } else {
                    const float u = p.mode == EP_DOWN ? leaky(fmaf(leaky(v + b, 0.01f), s, t), 0.2f) : leaky(v + b, 0.2f);
                    o[(long long)rt * Cout + c] = u;
                    if (p.out2) p.out2[(long long)row * Cout + c] = u;
                }
            }
        }
    }
}

// ------------------------------------------------------------------------------------------------------ final_conv
// Wave: row n, positions t0 .. t0 + 15 of flat's Kp / 2 position pairs.  Lane l keeps channels 2 l, 2 l + 1 of rows
// t0 .. t0 + 23 (rows past Lc3 feed no stored output and are not read), then per position the fma chain over (tap,
// channel pair) for both output channels and the xor-butterfly over the lanes.  Positions >= F are flat's zero tail.
__global__ __launch_bounds__(256) void ks_final_kernel(const float* __restrict__ in, long long N, int Lc, int F, int Kp,
                                                       int tblocks, const float* __restrict__ wf,
                                                       const float* __restrict__ bf, float* __restrict__ flat,
                                                       float* __restrict__ tap) {
    const int lane = threadIdx.x & 63;
    const long long wid = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (wid >= N * tblocks) return;
    const long long n = wid / tblocks;
    const int t0 = (int)(wid % tblocks) * FIN_T;
    constexpr int R = FIN_T + KB - 1;
    const float* base = in + n * (long long)Lc * C0 + 2 * lane;
    float2 v[R];
#pragma unroll
    for (int j = 0; j < R; ++j) {
        const int t = t0 + j;
        v[j] = t < Lc ? *reinterpret_cast<const float2*>(base + (long long)t * C0) : make_float2(0.f, 0.f);
    }
    float2 w[2][KB];
#pragma unroll
    for (int oc = 0; oc < 2; ++oc)
#pragma unroll
        for (int j = 0; j < KB; ++j) w[oc][j] = *reinterpret_cast<const float2*>(wf + (oc * KB + j) * C0 + 2 * lane);
    const float b0 = bf[0], b1 = bf[1];
#pragma unroll
    for (int u = 0; u < FIN_T; ++u) {
        float a0 = 0.f, a1 = 0.f;
#pragma unroll
        for (int j = 0; j < KB; ++j) {
            a0 = fmaf(w[0][j].x, v[u + j].x, a0);
            a0 = fmaf(w[0][j].y, v[u + j].y, a0);
            a1 = fmaf(w[1][j].x, v[u + j].x, a1);
            a1 = fmaf(w[1][j].y, v[u + j].y, a1);
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            a0 += __shfl_xor(a0, o);
            a1 += __shfl_xor(a1, o);
        }
        const int pos = t0 + u;
        if (lane == u && 2 * pos < Kp) {
            const bool live = pos < F;
            const float2 r = live ? make_float2(a0 + b0, a1 + b1) : make_float2(0.f, 0.f);
            *reinterpret_cast<float2*>(flat + n * (long long)Kp + 2 * pos) = r;
            if (tap && live) *reinterpret_cast<float2*>(tap + n * 2ll * F + 2 * pos) = r;
        }
    }
}

// ------------------------------------------------------------------------------------------------------- output_fc
// Work-group bid: M group mg = bid % mgroups (rows 32 MTW mg ..), output tile ot = bid / mgroups (outputs 32 ot ..), so
// that the groups sharing a weight tile run together.  Wave w accumulates K groups q = w, w + 4, .., QU of them per
// step (a small batch is bound by streaming the weight, so 8 KiB per wave are in flight); waves 1..3 park their
// accumulators in LDS and wave 0 adds them in order and stores y = sum + bias.
template <int MTW, int QU>
__global__ __launch_bounds__(256) void ks_fc_kernel(const float* __restrict__ flat, int Kp, unsigned rows, int mgroups,
                                                    const float4* __restrict__ frag, int G, const float* __restrict__ bias,
                                                    int O, float* __restrict__ y) {
    __shared__ float part[3][MTW][16][64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int i = lane & 31, h = lane >> 5;
    const unsigned mg = blockIdx.x % mgroups, ot = blockIdx.x / mgroups;
    const unsigned m0 = mg * (32 * MTW);
    const float* a[MTW];
#pragma unroll
    for (int mt = 0; mt < MTW; ++mt) {
        unsigned m = m0 + 32 * mt + i;
        if (m >= rows) m = rows - 1;
        a[mt] = flat + (long long)m * Kp + 4 * h;
    }
    const float4* bq = frag + (long long)ot * G * 64 + lane;
    f32x16 acc[MTW] = {};
    // QU groups (q, q + 4, ..) per step; the loads of the next step are issued before this step's MFMAs
    float4 av[QU][MTW], bv[QU];
#pragma unroll
    for (int u = 0; u < QU; ++u) {
        const int qq = wave + 4 * u;
        if (qq < G) {
#pragma unroll
            for (int mt = 0; mt < MTW; ++mt) av[u][mt] = *reinterpret_cast<const float4*>(a[mt] + 8 * qq);
            bv[u] = bq[(long long)qq * 64];
        }
    }
    for (int q = wave; q < G; q += 4 * QU) {
        float4 ca[QU][MTW], cb[QU];
#pragma unroll
        for (int u = 0; u < QU; ++u) {
#pragma unroll
            for (int mt = 0; mt < MTW; ++mt) ca[u][mt] = av[u][mt];
            cb[u] = bv[u];
        }
#pragma unroll
        for (int u = 0; u < QU; ++u) {
            const int qq = q + 4 * (QU + u);
            if (qq < G) {
#pragma unroll
                for (int mt = 0; mt < MTW; ++mt) av[u][mt] = *reinterpret_cast<const float4*>(a[mt] + 8 * qq);
                bv[u] = bq[(long long)qq * 64];
            }
        }
#pragma unroll
        for (int u = 0; u < QU; ++u) {
            if (q + 4 * u < G) {
#pragma unroll
                for (int mt = 0; mt < MTW; ++mt) acc[mt] = MFMA32(ca[u][mt].x, cb[u].x, acc[mt]);
#pragma unroll
                for (int mt = 0; mt < MTW; ++mt) acc[mt] = MFMA32(ca[u][mt].y, cb[u].y, acc[mt]);
#pragma unroll
                for (int mt = 0; mt < MTW; ++mt) acc[mt] = MFMA32(ca[u][mt].z, cb[u].z, acc[mt]);
#pragma unroll
                for (int mt = 0; mt < MTW; ++mt) acc[mt] = MFMA32(ca[u][mt].w, cb[u].w, acc[mt]);
            }
        }
    }
    if (wave > 0) {
#pragma unroll
        for (int mt = 0; mt < MTW; ++mt)
#pragma unroll
            for (int r = 0; r < 16; ++r) part[wave - 1][mt][r][lane] = acc[mt][r];
    }
    __syncthreads();
    if (wave > 0) return;
    const int o = 32 * (int)ot + i;
    if (o >= O) return;
    const float b = bias[o];
#pragma unroll
    for (int mt = 0; mt < MTW; ++mt) {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const unsigned row = m0 + 32 * mt + (r & 3) + 8 * (r >> 2) + 4 * h;
            if (row >= rows) continue;
            const float sum = ((acc[mt][r] + part[0][mt][r][lane]) + part[1][mt][r][lane]) + part[2][mt][r][lane];
            y[(long long)row * O + o] = sum + b;
        }
    }
}

template <typename K, typename... A>
bool launch(K kernel, dim3 grid, hipStream_t s, A... args) {
    hipLaunchKernelGGL(kernel, grid, dim3(256), 0, s, args...);
    return hipGetLastError() == hipSuccess;
}

template <bool TRAIN = false>
bool launch_conv(const ConvArgs& p, int variant, hipStream_t s) {
    const int64_t M = p.M, nb = p.Cout / 128;
    if (variant == 0) variant = (M + 63) / 64 * nb >= 1536 ? 3 : (M + 31) / 32 * nb >= 1024 ? 2 : 1;
    if constexpr (TRAIN) {
        if (variant == 3) variant = 2;                        // two sets of accumulators: the 64 x 128 wave tile has no room for them
    } else {
        if (variant == 3) return launch(ks_conv_kernel<2, 4, QU_WIDE>, dim3((unsigned)((M + 255) / 256), (unsigned)nb), s, p);
    }
    if (variant == 2) return launch((ks_conv_kernel<1, 4, QU_MID, TRAIN>), dim3((unsigned)((M + 127) / 128), (unsigned)nb), s, p);
    return launch((ks_conv_kernel<1, 1, QU_NARROW, TRAIN>), dim3((unsigned)((M + 127) / 128), (unsigned)(p.Cout / 32)), s, p);
}

}  // namespace
