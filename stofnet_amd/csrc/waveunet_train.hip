// Wave-U-Net training on gfx950 (models/wave_unet.py in train mode): the stages of one step, one kernel each, staged through
// device memory, exact fp32 (v_mfma_f32_16x16x4_f32 where the work is a GEMM), no float atomic and no library call: every
// output element is one fixed-order sum, so two runs are bitwise equal.  Activations are dense channel-last fp32 [N, L_i, C]
// as in waveunet.hip; the convolution, window and coordinate code is waveunet_net.h.  The host side
// (stofnet_amd/waveunet_training.py) chains the stages; every entry here works on one convolution / one block.
//
// Forward, per Conv + BN + LeakyReLU block:
//   wt_pack_frag_kernel     the raw weight [cout][cin][taps] -> the B fragment image of wu_conv_kernel (flip = 0), or the
//                           image of the data gradient W'[ci][co][d] = W[co][ci][taps - 1 - d] (flip = 1)
//   wu_in_kernel<false>     encoder 0: z = conv(x) + bias            wu_conv_kernel<.., false>   every other conv: z
//   bn_train.h              the train-mode BatchNorm with WaveAct below: the batch statistics and a = leaky_0.1(z s + t) in
//                           double, rounded once.  The LeakyReLU decision of the backward is a > 0.
//   wu_head_kernel          y = tanh(w[0:16] . o + w[16] x + b)
// Backward:
//   wt_head_bwd_kernel      dl = dy (1 - y^2); do = w[0:16] dl; the w[16] dl term of dx (only if dx is wanted)
//   wt_head_wgrad_kernel    sum dl o, sum dl x, sum dl as row-chunk partials -> partial_reduce
//   bn_train.h              g = da (a > 0 ? 1 : 0.1) in double -> dbeta, dgamma, dz
//   wt_wgrad_kernel         dW[co][ci][d] = sum_rows dz[row][co] in[row + d - pad][ci], fp32 MFMA with K over rows: a work-group
//                           owns 16 output x 16 input channels and all taps (wave w: taps w, w + 4, ..) of one chunk of
//                           (waveform, 64-position tile) units; `in` is the forward's virtual input, built in LDS by the
//                           forward's wu_source; zero padding per waveform.  The work-groups of input block 0 also sum the
//                           columns of dz (d bias).  One partial per chunk -> partial_reduce (ConvTapsThenBias).
//   wt_in_wgrad_kernel      encoder 0 (Cin = 1) on the vector pipe, thread (co, tap | bias) over a row chunk
//   wu_conv_kernel<.., SRC_PLAIN, .., false> on the flipped image: the gradient of the virtual input [N, Lout, Cin]
//   wt_interp_t_kernel      the transpose of the interpolation, gather: low position m sums l0(u) g[u] (where i0(u) = m) then
//                           l1(u) g[u] (where i1(u) = m) over u ascending in wu_interp_window(m)
//   wt_skip_sum_kernel      d skip = the decoder's part at every position, then + the next encoder's (or the middle's) part
//                           at even positions, written once
//   wt_in_dgrad_kernel      encoder 0's data gradient (16 -> 1, 15 taps) + the head's term -> dx
//
// Bounded chunks, cut by fill_chunks of wgrad_reduce.h (rows per partial at the least / partials at the most; beyond that the rows per partial grow):
//   statistics, BN backward  ST_ROWS = 256 rows / ST_MAX = 256        head weights   HB_ROWS = 256 rows / HB_MAX = 256
//   encoder-0 weights        IW_ROWS = 256 rows / IW_MAX = 256
//   conv weights             whole 64-position tiles of one waveform (a tile past the end of a waveform is partly empty),
//                            WG_TILES = 1 tile / WG_MAX = 128
#include <hip/hip_runtime.h>
#include <math.h>
#include "stof_common.h"
#include "waveunet_net.h"
#include "bn_train.h"
#include "wgrad_reduce.h"

namespace {

constexpr int ST_ROWS = 256, ST_MAX = 256;
constexpr int HB_ROWS = 256, HB_MAX = 256;
constexpr int IW_ROWS = 256, IW_MAX = 256;
constexpr int WG_TILES = 1, WG_MAX = 128;
constexpr int MAX_C = 2 * CI * MAX_LAYERS;          // 384: the widest virtual input (decoder 0 of n = 12)

bool rows_ok(int64_t N, int64_t L) { return N >= 1 && L >= 1 && L < (1ll << 31) && N < (1ll << 31) && N * L < (1ll << 31) - 64; }
bool nrows_ok(int64_t rows) { return rows >= 1 && rows < (1ll << 31) - 64; }
bool chan_ok(int c) { return c >= 16 && c <= MAX_C && c % 16 == 0; }

// ------------------------------------------------------------------------------------------------------------ packing
// image element (nt, g, lane, e) <- W[16 nt + (lane & 15)][channel][tap] of the image's own (Cin, Cout), see waveunet.hip
__global__ __launch_bounds__(256) void wt_pack_frag_kernel(const float* __restrict__ w, int cin, int cout, int taps, int flip,
                                                           int ntp, float* __restrict__ out) {
    const int icin = flip ? cout : cin, icout = flip ? cin : cout;
    const int groups = taps * icin / 16;
    const long long total = (long long)ntp * groups * 256;
    const long long at = (long long)blockIdx.x * 256 + threadIdx.x;
    if (at >= total) return;
    const int e = (int)(at & 3), lane = (int)((at >> 2) & 63);
    const long long ng = at >> 8;
    const int nt = (int)(ng / groups);
    int g = (int)(ng - (long long)nt * groups);
    int c0 = 0, cw = icin < CHUNK ? icin : CHUNK;
    if (g >= taps * cw / 16) { g -= taps * cw / 16; c0 = CHUNK; cw = icin - CHUNK; }
    const int blocks = cw / 16, tap = g / blocks, blk = g - tap * blocks;
    const int oc = 16 * nt + (lane & 15), ch = c0 + 16 * blk + 4 * (lane >> 4) + e;
    float v = 0.f;
    if (oc < icout) v = flip ? w[((long long)ch * cin + oc) * taps + (taps - 1 - tap)] : w[((long long)oc * cin + ch) * taps + tap];
    out[at] = v;
}

// encoder 0: weight [16][1][15], bias [16] -> rows 0 .. 14 = [tap][c], row 15 = bias
__global__ __launch_bounds__(256) void wt_pack_in_kernel(const float* __restrict__ w, const float* __restrict__ b, float* __restrict__ out) {
    const int j = threadIdx.x >> 4, c = threadIdx.x & 15;
    out[threadIdx.x] = j < ENC_TAPS ? w[c * ENC_TAPS + j] : b[c];
}

// ----------------------------------------------------------------------------------------------------------- BatchNorm
// What Wave-U-Net brings to bn_train.h: dense [rows][C] tensors (Rows), 64 channels per work-group with four row parts folded
// in pairs, the rows cut by the fill-to-minimum rule, and the slope, xhat and the LeakyReLU all in double.
struct WaveAct {
    static constexpr bool reads_a = true;
    __device__ static double g(float da, float a) { return (double)da * (a > 0.f ? 1.0 : 0.1); }
    __device__ static double seen(double xh) { return xh; }
    __device__ static double scale(const float*, const double* stat, int C, int c) { return stat[2 * C + c]; }
    __device__ static float out(double u) { return (float)(u > 0.0 ? u : 0.1 * u); }
};

// ---------------------------------------------------------------------------------------------------------------- head
__global__ __launch_bounds__(256) void wt_head_bwd_kernel(const float* __restrict__ dy, const float* __restrict__ y, const float* __restrict__ w,
                                                          long long M, float* __restrict__ dout, float* __restrict__ dxh) {
    const long long m = (long long)blockIdx.x * 256 + threadIdx.x;
    if (m >= M) return;
    const float yv = y[m], dl = dy[m] * (1.f - yv * yv);
#pragma unroll
    for (int c = 0; c < CI; c += 4)
        *reinterpret_cast<float4*>(dout + m * CI + c) = make_float4(w[c] * dl, w[c + 1] * dl, w[c + 2] * dl, w[c + 3] * dl);
    if (dxh) dxh[m] = w[CI] * dl;
}

// thread (k = tid & 31, rl = tid >> 5): element k (0 .. 15: sum dl o[.][k], 16: sum dl x, 17: sum dl) over rows r0 + rl, + 8, ..;
// the eight row lanes fold as ((0 + 1) + (2 + 3)) + ((4 + 5) + (6 + 7)).  part [chunk][18].
__global__ __launch_bounds__(256) void wt_head_wgrad_kernel(const float* __restrict__ dy, const float* __restrict__ y, const float* __restrict__ o,
                                                            const float* __restrict__ x, long long M, long long rows_per,
                                                            float* __restrict__ part) {
    __shared__ float red[8][32];
    const int k = threadIdx.x & 31, rl = threadIdx.x >> 5;
    const long long r0 = blockIdx.x * rows_per, r1 = r0 + rows_per < M ? r0 + rows_per : M;
    float acc = 0.f;
    if (k < CI + 2)
        for (long long r = r0 + rl; r < r1; r += 8) {
            const float yv = y[r], dl = dy[r] * (1.f - yv * yv);
            const float v = k < CI ? o[r * CI + k] : (k == CI ? x[r] : 1.f);
            acc = fmaf(dl, v, acc);
        }
    red[rl][k] = acc;
    __syncthreads();
    if (rl != 0 || k >= CI + 2) return;
    part[(long long)blockIdx.x * (CI + 2) + k] = ((red[0][k] + red[1][k]) + (red[2][k] + red[3][k])) + ((red[4][k] + red[5][k]) + (red[6][k] + red[7][k]));
}

// ------------------------------------------------------------------------------------------------------ weight gradients
struct WuWgradArgs {
    WuConvArgs c;                          // src, low, Lout, tiles, Cin, Cu, Cout, scale of the forward convolution
    const float* dz;                       // [N, Lout, Cout]
    float* part;                           // [chunks][E], E = Cout K + Cout, K = TAPS Cin: element co K + tap Cin + ci, then the bias
    long long units, units_per, E;         // units = N tiles
};

// grid (chunk, Cout / 16, Cin / 16).  MFMA: A[i = co][k = row] = dz, B[k = row][j = ci] = in[row + tap - PAD], four rows per MFMA,
// rows ascending; D[co = 4 (lane >> 4) + r][ci = lane & 15].
template <int TAPS, int SRC>
__global__ __launch_bounds__(256) void wt_wgrad_kernel(const WuWgradArgs w) {
    constexpr int PAD = TAPS / 2, ROWS = TM + TAPS - 1, SW = 20, NT = (TAPS + 3) / 4;
    __shared__ __attribute__((aligned(16))) float win[ROWS * SW];
    __shared__ __attribute__((aligned(16))) float dzt[TM * SW];
    const WuConvArgs& a = w.c;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int j = lane & 15, q = lane >> 4;
    const int co0 = 16 * blockIdx.y, ci0 = 16 * blockIdx.z;
    const long long Lout = a.Lout;
    f32x4 acc[NT] = {};
    float bsum = 0.f;
    const long long ub = blockIdx.x * w.units_per, ue = ub + w.units_per < w.units ? ub + w.units_per : w.units;
    for (long long unit = ub; unit < ue; ++unit) {
        const long long n = unit / a.tiles, t0 = (unit % a.tiles) * TM;
        if (unit != ub) __syncthreads();
        wu_build_window<SRC>(win, SW, ci0, 16, n, t0 - PAD, ROWS, a, tid);
        {
            const int row = tid >> 2, c4 = 4 * (tid & 3);
            const long long p = t0 + row;
            float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
            if (p < Lout) v = *reinterpret_cast<const float4*>(w.dz + (n * Lout + p) * a.Cout + co0 + c4);
            *reinterpret_cast<float4*>(dzt + row * SW + c4) = v;
        }
        __syncthreads();
#pragma unroll
        for (int k = 0; k < NT; ++k) {
            const int tap = wave + 4 * k;
            if (tap < TAPS) {
#pragma unroll
                for (int s = 0; s < TM / 4; ++s)
                    acc[k] = MFMA16(dzt[(4 * s + q) * SW + j], win[(4 * s + q + tap) * SW + j], acc[k]);
            }
        }
        if (blockIdx.z == 0 && tid < 16)
            for (int r = 0; r < TM; ++r) bsum += dzt[r * SW + tid];
    }
    float* const part = w.part + (long long)blockIdx.x * w.E;
    const long long K = (long long)TAPS * a.Cin;
#pragma unroll
    for (int k = 0; k < NT; ++k) {
        const int tap = wave + 4 * k;
        if (tap < TAPS) {
#pragma unroll
            for (int r = 0; r < 4; ++r) part[(co0 + 4 * q + r) * K + (long long)tap * a.Cin + ci0 + j] = acc[k][r];
        }
    }
    if (blockIdx.z == 0 && tid < 16) part[(long long)a.Cout * K + co0 + tid] = bsum;
}

// encoder 0: thread (co = tid >> 4, d = tid & 15; d = 15: the bias) over rows r0 .. r1 ascending.  part [chunk][256]: co 15 + d, then
// 240 + co.
__global__ __launch_bounds__(256) void wt_in_wgrad_kernel(const float* __restrict__ x, const float* __restrict__ dz, long long M, long long L,
                                                          long long rows_per, float* __restrict__ part) {
    const int co = threadIdx.x >> 4, d = threadIdx.x & 15;
    const long long r0 = blockIdx.x * rows_per, r1 = r0 + rows_per < M ? r0 + rows_per : M;
    long long t = r0 % L;
    float acc = 0.f;
    for (long long r = r0; r < r1; ++r) {
        const float g = dz[r * CI + co];
        float xv = 1.f;
        if (d < ENC_TAPS) {
            const long long u = t + d - 7;
            xv = (u >= 0 && u < L) ? x[r + d - 7] : 0.f;
        }
        acc = fmaf(g, xv, acc);
        if (++t == L) t = 0;
    }
    part[(long long)blockIdx.x * 256 + (d < ENC_TAPS ? co * ENC_TAPS + d : CI * ENC_TAPS + co)] = acc;
}

// ------------------------------------------------------------------------------------------------------ gradient routing
// g [N, 2 M, Cg] (the first Cu channels are the gradient of the interpolated map) -> dlow [N, M, Cu].  Thread: four channels of (n, m).
__global__ __launch_bounds__(256) void wt_interp_t_kernel(const float* __restrict__ g, long long total4, int M, int Cg, int Cu, float scale,
                                                          float* __restrict__ dlow) {
    const long long at = (long long)blockIdx.x * 256 + threadIdx.x;
    if (at >= total4) return;
    const int q4 = Cu / 4, c = 4 * (int)(at % q4);
    const long long nm = at / q4, n = nm / M;
    const int m = (int)(nm - n * M);
    int lo, hi;
    wu_interp_window(m, M, lo, hi);
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int u = lo; u <= hi; ++u) {
        int i0, i1;
        float l0, l1;
        wu_coords(scale, u, M, i0, i1, l0, l1);
        if (i0 != m && i1 != m) continue;
        const float4 v = *reinterpret_cast<const float4*>(g + (n * 2 * M + u) * Cg + c);
        if (i0 == m) { acc.x = fmaf(l0, v.x, acc.x); acc.y = fmaf(l0, v.y, acc.y); acc.z = fmaf(l0, v.z, acc.z); acc.w = fmaf(l0, v.w, acc.w); }
        if (i1 == m) { acc.x = fmaf(l1, v.x, acc.x); acc.y = fmaf(l1, v.y, acc.y); acc.z = fmaf(l1, v.z, acc.z); acc.w = fmaf(l1, v.w, acc.w); }
    }
    *reinterpret_cast<float4*>(dlow + nm * Cu + c) = acc;
}

// out[n][u][c] = gdec[n][u][Cu + c] (+ genc[n][u / 2][c] at even u), gdec [N, L, Cu + Cs], genc [N, L / 2, Cs]
__global__ __launch_bounds__(256) void wt_skip_sum_kernel(const float* __restrict__ gdec, const float* __restrict__ genc, long long total4,
                                                          long long L, int Cu, int Cs, float* __restrict__ out) {
    const long long at = (long long)blockIdx.x * 256 + threadIdx.x;
    if (at >= total4) return;
    const int q4 = Cs / 4, c = 4 * (int)(at % q4);
    const long long nu = at / q4, n = nu / L, u = nu - n * L;
    float4 v = *reinterpret_cast<const float4*>(gdec + nu * (Cu + Cs) + Cu + c);
    if ((u & 1) == 0) {
        const float4 e = *reinterpret_cast<const float4*>(genc + (n * (L / 2) + u / 2) * Cs + c);
        v = make_float4(v.x + e.x, v.y + e.y, v.z + e.z, v.w + e.w);
    }
    *reinterpret_cast<float4*>(out + nu * Cs + c) = v;
}

// dx[n][t] = (dxh[n][t] +) sum_d sum_co dz[n][t - d + 7][co] w[co][0][d], taps then channels ascending in one fma chain
__global__ __launch_bounds__(256) void wt_in_dgrad_kernel(const float* __restrict__ dz, const float* __restrict__ w, const float* __restrict__ dxh,
                                                          long long M, long long L, float* __restrict__ dx) {
    __shared__ float wt[ENC_TAPS * CI];
    if (threadIdx.x < ENC_TAPS * CI) wt[threadIdx.x] = w[(threadIdx.x & 15) * ENC_TAPS + (threadIdx.x >> 4)];
    __syncthreads();
    const long long m = (long long)blockIdx.x * 256 + threadIdx.x;
    if (m >= M) return;
    const long long t = m % L;
    float acc = 0.f;
    for (int d = 0; d < ENC_TAPS; ++d) {
        const long long u = t - d + 7;
        if (u < 0 || u >= L) continue;
        const float* row = dz + (m - d + 7) * CI;
#pragma unroll
        for (int c = 0; c < CI; c += 4) {
            const float4 v = *reinterpret_cast<const float4*>(row + c);
            acc = fmaf(v.x, wt[d * CI + c], acc);
            acc = fmaf(v.y, wt[d * CI + c + 1], acc);
            acc = fmaf(v.z, wt[d * CI + c + 2], acc);
            acc = fmaf(v.w, wt[d * CI + c + 3], acc);
        }
    }
    dx[m] = dxh ? dxh[m] + acc : acc;
}

bool conv_ok(int64_t N, int64_t Lout, int cin, int cu, int cout, int taps, int mode) {
    if (!rows_ok(N, Lout) || !chan_ok(cin) || !chan_ok(cout) || N * Lout * (cin > cout ? cin : cout) >= (1ll << 40)) return false;
    if (mode == SRC_DECIMATED) return taps == ENC_TAPS && cu == 0 && N * Lout * 2 < (1ll << 31) - 64;
    if (mode == SRC_DECODER) return taps == DEC_TAPS && cu >= 16 && cu % 16 == 0 && cu < cin && Lout % 2 == 0;
    return mode == SRC_PLAIN && (taps == ENC_TAPS || taps == DEC_TAPS) && cu == 0;
}

}  // namespace

extern "C" int stof_waveunet_train_constants(int64_t* out) {
    if (!out) return STOF_ERR_BAD_ARG;
    const int64_t v[10] = {ST_ROWS, ST_MAX, HB_ROWS, HB_MAX, IW_ROWS, IW_MAX, (int64_t)WG_TILES * TM, WG_MAX, TM, WU_INTERP_MAX_M};
    for (int i = 0; i < 10; ++i) out[i] = v[i];
    return STOF_OK;
}

// host only: the coordinates of every high position u in [0, 2 M) and the window of every low position m in [0, M)
extern "C" int stof_waveunet_interp_table(int64_t M, int32_t* i0, int32_t* i1, float* l0, float* l1, int32_t* lo, int32_t* hi) {
    if (M < 1 || M > WU_INTERP_MAX_M || !i0 || !i1 || !l0 || !l1 || !lo || !hi) return STOF_ERR_BAD_ARG;
    const float scale = wu_scale(M);
    for (int u = 0; u < 2 * M; ++u) {
        int a, b;
        wu_coords(scale, u, (int)M, a, b, l0[u], l1[u]);
        i0[u] = a;
        i1[u] = b;
    }
    for (int m = 0; m < M; ++m) {
        int a, b;
        wu_interp_window(m, (int)M, a, b);
        lo[m] = a;
        hi[m] = b;
    }
    return STOF_OK;
}

extern "C" size_t stof_waveunet_train_frag_floats(int32_t cin, int32_t cout, int32_t taps, int32_t flip) {
    if (!chan_ok(cin) || !chan_ok(cout) || (taps != ENC_TAPS && taps != DEC_TAPS)) return 0;
    const int icin = flip ? cout : cin, icout = flip ? cin : cout;
    const int tiles = icout / 16, ntw = wu_ntw(tiles), ntp = (tiles + ntw - 1) / ntw * ntw;
    return (size_t)ntp * (taps * icin / 16) * 256;
}

extern "C" int stof_waveunet_train_pack_frag(const float* w, int32_t cin, int32_t cout, int32_t taps, int32_t flip, float* frag,
                                             void* stream) {
    const size_t total = stof_waveunet_train_frag_floats(cin, cout, taps, flip);
    if (!total || !w || !frag) return STOF_ERR_BAD_ARG;
    const int icout = flip ? cin : cout, tiles = icout / 16, ntw = wu_ntw(tiles), ntp = (tiles + ntw - 1) / ntw * ntw;
    hipLaunchKernelGGL(wt_pack_frag_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, static_cast<hipStream_t>(stream), w, cin,
                       cout, taps, flip ? 1 : 0, ntp, frag);
    return launched();
}

extern "C" int stof_waveunet_train_pack_in(const float* w, const float* b, float* image, void* stream) {
    if (!w || !b || !image) return STOF_ERR_BAD_ARG;
    hipLaunchKernelGGL(wt_pack_in_kernel, dim3(1), dim3(256), 0, static_cast<hipStream_t>(stream), w, b, image);
    return launched();
}

extern "C" int stof_waveunet_train_in_conv(const float* x, int64_t N, int64_t L, const float* image, float* z, void* stream) {
    if (!rows_ok(N, L) || !x || !image || !z) return STOF_ERR_BAD_ARG;
    const long long M = N * L;
    hipLaunchKernelGGL(wu_in_kernel<false>, dim3((unsigned)((M * 4 + 255) / 256)), dim3(256), 0, static_cast<hipStream_t>(stream), x, M,
                       (long long)L, image, z);
    return launched();
}

extern "C" int stof_waveunet_train_conv(const float* src, const float* low, int64_t N, int64_t Lout, int32_t cin, int32_t cu, int32_t cout,
                                        int32_t taps, int32_t mode, const float* frag, const float* bias, float* out, void* stream) {
    if (!conv_ok(N, Lout, cin, cu, cout, taps, mode) || !src || !frag || !out || (mode == SRC_DECODER && !low)) return STOF_ERR_BAD_ARG;
    WuConvArgs a{};
    a.src = src; a.low = low; a.out = out; a.bias = bias;
    a.frag = reinterpret_cast<const float4*>(frag);
    a.Lout = Lout; a.Cin = cin; a.Cu = cu; a.Cout = cout;
    const int tiles = cout / 16, ntw = wu_ntw(tiles), ntp = (tiles + ntw - 1) / ntw * ntw;
    dim3 grid;
    size_t lds;
    wu_conv_geometry(a, taps, N, ntw, ntp, grid, lds);
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (mode == SRC_DECIMATED) wu_launch_conv<ENC_TAPS, SRC_DECIMATED, false>(ntw, grid, lds, s, a);
    else if (mode == SRC_DECODER) wu_launch_conv<DEC_TAPS, SRC_DECODER, false>(ntw, grid, lds, s, a);
    else if (taps == ENC_TAPS) wu_launch_conv<ENC_TAPS, SRC_PLAIN, false>(ntw, grid, lds, s, a);
    else wu_launch_conv<DEC_TAPS, SRC_PLAIN, false>(ntw, grid, lds, s, a);
    return launched();
}

extern "C" size_t stof_waveunet_train_stats_workspace_bytes(void) { return ((size_t)ST_MAX * 2 * MAX_C + 2 * MAX_C) * sizeof(double); }

extern "C" int stof_waveunet_train_stats(const float* z, int64_t rows, int32_t ch, const float* gamma, const float* beta,
                                         const float* run_mean, const float* run_var, double eps, double momentum, double* stat,
                                         float* new_mean, float* new_var, void* workspace, size_t workspace_bytes, void* stream) {
    if (!nrows_ok(rows) || rows < 2 || !chan_ok(ch) || !z || !gamma || !beta || !run_mean || !run_var || !stat || !new_mean || !new_var)
        return STOF_ERR_BAD_ARG;
    if (!workspace || workspace_bytes < stof_waveunet_train_stats_workspace_bytes()) return STOF_ERR_WORKSPACE;
    const Chunks cs = fill_chunks(rows, ST_ROWS, ST_MAX);
    double* part = static_cast<double*>(workspace);
    hipStream_t s = static_cast<hipStream_t>(stream);
    return bn_stats_launch<64, FoldPairs>(s, z, rows, Rows{ch}, cs, eps, momentum, gamma, beta, run_mean, run_var, stat, new_mean, new_var, part);
}

extern "C" int stof_waveunet_train_apply(const float* z, int64_t rows, int32_t ch, const double* stat, float* a, void* stream) {
    if (!nrows_ok(rows) || !chan_ok(ch) || !z || !stat || !a) return STOF_ERR_BAD_ARG;
    return bn_apply_launch<4, WaveAct>(static_cast<hipStream_t>(stream), z, rows, Rows{ch}, stat, a);
}

extern "C" int stof_waveunet_train_head(const float* o, const float* x, int64_t N, int64_t L, const float* w, const float* b, float* y,
                                        void* stream) {
    if (!rows_ok(N, L) || !o || !x || !w || !b || !y) return STOF_ERR_BAD_ARG;
    const long long M = N * L;
    hipLaunchKernelGGL(wu_head_kernel, dim3((unsigned)((M + 255) / 256)), dim3(256), 0, static_cast<hipStream_t>(stream), o, x, M, w, b, y,
                       (float*)nullptr);
    return launched();
}

extern "C" size_t stof_waveunet_train_head_bwd_workspace_bytes(void) { return (size_t)HB_MAX * (CI + 2) * sizeof(float); }

extern "C" int stof_waveunet_train_head_bwd(const float* dy, const float* y, const float* o, const float* x, int64_t N, int64_t L,
                                            const float* w, float* dout, float* dxh, float* dw, float* db, void* workspace,
                                            size_t workspace_bytes, void* stream) {
    if (!rows_ok(N, L) || !dy || !y || !o || !x || !w || !dout || !dw || !db) return STOF_ERR_BAD_ARG;
    if (!workspace || workspace_bytes < stof_waveunet_train_head_bwd_workspace_bytes()) return STOF_ERR_WORKSPACE;
    const long long M = N * L;
    hipStream_t s = static_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(wt_head_bwd_kernel, dim3((unsigned)((M + 255) / 256)), dim3(256), 0, s, dy, y, w, M, dout, dxh);
    const Chunks cs = fill_chunks(M, HB_ROWS, HB_MAX);
    float* part = static_cast<float*>(workspace);
    hipLaunchKernelGGL(wt_head_wgrad_kernel, dim3(cs.n), dim3(256), 0, s, dy, y, o, x, M, cs.per, part);
    partial_reduce(s, part, cs.n, CI + 2, CI + 2, DwThenDb{dw, db, CI + 1}, 1.f);
    return launched();
}

extern "C" int stof_waveunet_train_bn_bwd(const float* da, const float* a, const float* z, const double* stat, int64_t rows, int32_t ch,
                                          float* dgamma, float* dbeta, float* dz, void* workspace, size_t workspace_bytes, void* stream) {
    if (!nrows_ok(rows) || rows < 2 || !chan_ok(ch) || !da || !a || !z || !stat || !dgamma || !dbeta || !dz) return STOF_ERR_BAD_ARG;
    if (!workspace || workspace_bytes < stof_waveunet_train_stats_workspace_bytes()) return STOF_ERR_WORKSPACE;
    const Chunks cs = fill_chunks(rows, ST_ROWS, ST_MAX);
    double* part = static_cast<double*>(workspace);
    double* coef = part + (size_t)ST_MAX * 2 * MAX_C;
    hipStream_t s = static_cast<hipStream_t>(stream);
    return bn_bnb_launch<4, 64, FoldPairs, WaveAct>(s, da, a, z, stat, nullptr, rows, Rows{ch}, cs, dgamma, dbeta, dz, part, coef);
}

extern "C" size_t stof_waveunet_train_wgrad_workspace_bytes(int64_t N, int64_t Lout, int32_t cin, int32_t cout, int32_t taps) {
    if (!rows_ok(N, Lout) || !chan_ok(cin) || !chan_ok(cout) || (taps != ENC_TAPS && taps != DEC_TAPS)) return 0;
    const Chunks cs = fill_chunks(N * ((Lout + TM - 1) / TM), WG_TILES, WG_MAX);
    return (size_t)cs.n * ((size_t)cout * taps * cin + cout) * sizeof(float);
}

extern "C" int stof_waveunet_train_wgrad(const float* src, const float* low, const float* dz, int64_t N, int64_t Lout, int32_t cin,
                                         int32_t cu, int32_t cout, int32_t taps, int32_t mode, float* dw, float* db, void* workspace,
                                         size_t workspace_bytes, void* stream) {
    if (!conv_ok(N, Lout, cin, cu, cout, taps, mode) || cout > CI * MAX_LAYERS || !src || !dz || !dw || !db || (mode == SRC_DECODER && !low))
        return STOF_ERR_BAD_ARG;
    if (!workspace || workspace_bytes < stof_waveunet_train_wgrad_workspace_bytes(N, Lout, cin, cout, taps)) return STOF_ERR_WORKSPACE;
    WuWgradArgs w{};
    w.c.src = src; w.c.low = low; w.c.Lout = Lout; w.c.Cin = cin; w.c.Cu = cu; w.c.Cout = cout;
    w.c.tiles = (int)((Lout + TM - 1) / TM);
    w.c.scale = cu ? wu_scale(Lout / 2) : 0.f;
    w.dz = dz;
    w.part = static_cast<float*>(workspace);
    w.units = N * w.c.tiles;
    const Chunks cs = fill_chunks(w.units, WG_TILES, WG_MAX);
    w.units_per = cs.per;
    w.E = (long long)cout * taps * cin + cout;
    if (w.E >= (1ll << 31)) return STOF_ERR_UNSUPPORTED;
    const dim3 grid(cs.n, cout / 16, cin / 16);
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (mode == SRC_DECIMATED) hipLaunchKernelGGL((wt_wgrad_kernel<ENC_TAPS, SRC_DECIMATED>), grid, dim3(256), 0, s, w);
    else if (mode == SRC_DECODER) hipLaunchKernelGGL((wt_wgrad_kernel<DEC_TAPS, SRC_DECODER>), grid, dim3(256), 0, s, w);
    else if (taps == ENC_TAPS) hipLaunchKernelGGL((wt_wgrad_kernel<ENC_TAPS, SRC_PLAIN>), grid, dim3(256), 0, s, w);
    else hipLaunchKernelGGL((wt_wgrad_kernel<DEC_TAPS, SRC_PLAIN>), grid, dim3(256), 0, s, w);
    partial_reduce(s, w.part, cs.n, (int)w.E, (int)w.E, ConvTapsThenBias{dw, db, cout, cin, cin, taps * cin, taps}, 1.f);
    return launched();
}

extern "C" size_t stof_waveunet_train_in_wgrad_workspace_bytes(void) { return (size_t)IW_MAX * 256 * sizeof(float); }

extern "C" int stof_waveunet_train_in_wgrad(const float* x, const float* dz, int64_t N, int64_t L, float* dw, float* db, void* workspace,
                                            size_t workspace_bytes, void* stream) {
    if (!rows_ok(N, L) || !x || !dz || !dw || !db) return STOF_ERR_BAD_ARG;
    if (!workspace || workspace_bytes < stof_waveunet_train_in_wgrad_workspace_bytes()) return STOF_ERR_WORKSPACE;
    const long long M = N * L;
    const Chunks cs = fill_chunks(M, IW_ROWS, IW_MAX);
    float* part = static_cast<float*>(workspace);
    hipStream_t s = static_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(wt_in_wgrad_kernel, dim3(cs.n), dim3(256), 0, s, x, dz, M, (long long)L, cs.per, part);
    partial_reduce(s, part, cs.n, 256, 256, ConvTapsThenBias{dw, db, CI, 1, 1, ENC_TAPS, ENC_TAPS}, 1.f);
    return launched();
}

extern "C" int stof_waveunet_train_interp_t(const float* g, int64_t N, int64_t M, int32_t cg, int32_t cu, float* dlow, void* stream) {
    if (!rows_ok(N, 2 * M) || M > WU_INTERP_MAX_M || !chan_ok(cg) || cu < 16 || cu % 16 || cu > cg || !g || !dlow) return STOF_ERR_BAD_ARG;
    const long long total4 = N * M * (cu / 4);
    hipLaunchKernelGGL(wt_interp_t_kernel, dim3((unsigned)((total4 + 255) / 256)), dim3(256), 0, static_cast<hipStream_t>(stream), g, total4,
                       (int)M, cg, cu, wu_scale(M), dlow);
    return launched();
}

extern "C" int stof_waveunet_train_skip_sum(const float* gdec, const float* genc, int64_t N, int64_t L, int32_t cu, int32_t cs, float* out,
                                            void* stream) {
    if (!rows_ok(N, L) || L % 2 || cu < 16 || cu % 16 || !chan_ok(cs) || !chan_ok(cu + cs) || !gdec || !genc || !out) return STOF_ERR_BAD_ARG;
    const long long total4 = N * L * (cs / 4);
    hipLaunchKernelGGL(wt_skip_sum_kernel, dim3((unsigned)((total4 + 255) / 256)), dim3(256), 0, static_cast<hipStream_t>(stream), gdec, genc,
                       total4, (long long)L, cu, cs, out);
    return launched();
}

extern "C" int stof_waveunet_train_in_dgrad(const float* dz, const float* w, const float* dxh, int64_t N, int64_t L, float* dx, void* stream) {
    if (!rows_ok(N, L) || !dz || !w || !dx) return STOF_ERR_BAD_ARG;
    const long long M = N * L;
    hipLaunchKernelGGL(wt_in_dgrad_kernel, dim3((unsigned)((M + 255) / 256)), dim3(256), 0, static_cast<hipStream_t>(stream), dz, w, dxh, M,
                       (long long)L, dx);
    return launched();
}
