// Training the SincNet baseline in exact fp32, one kernel per stage, on the GAP layout of the inference file (sincnet_net.h):
// every 128-channel tensor (z_l, a_l, dz_l, da_l of layers 0..2) is [GAP + N (L + GAP)][128] with zero gap rows, the
// one-channel tensors of layer 3 (z_3, y, dy, dz_3) are flat [N L].
//
//   forward, per layer    the kernels of sincnet_net.h with EPI_BIAS: the raw pre-BatchNorm z_l = conv + bias;
//                         the train-mode BatchNorm of bn_train.h (statistics, a_l = leaky(z_l s + t), layer 3: y = z_3 s + t)
//                         with the view and the activation below (GapRows, SincAct).
//   backward, per layer   bn_train.h again: dgamma, dbeta and dz with g = da (a > 0 ? 1 : 0.2);
//                         data gradient of layers 1, 2: sn_conv_kernel with EPI_NONE on the flipped, transposed image;
//                         sn_wgrad_kernel (v_mfma_f32_32x32x2_f32): dW[co][tap 128 + ci] = sum over rows of dz[row][co]
//                         a_prev[row + tap - P][ci], the reduction dimension is the rows; db in a bias slot of the partial;
//                         layer 3 on the vector pipe: sn_out_wgrad_kernel, sn_out_dgrad_kernel;
//                         layer 0: sn_bank_grad_kernel (MFMA): G[c][k] = sum over (n, t) of dz0[n][t][c] x[n][t - 511 + k], x
//                         staged in LDS as in sn_sinc_kernel; sn_band_grad_kernel chains G to low_hz_ / band_hz_ in double
//                         (one work-group per filter); sn_in_dgrad_kernel: dx on the vector pipe, on request only.
//   packing               (stof_sincnet_device_pack builds the INFERENCE blob from the same kernels plus sn_pack_affine_kernel)
//                         sn_pack_bank_kernel synthesises the bank in double straight into fragment order (and as bank_t
//                         [tap][filter] for dx), pack_frag32_kernel of mfma32_frag.h the conv images, sn_dgrad_image_kernel
//                         the flipped ones of the data gradient, sn_pack_w3_kernel w3 [tap][ci].
//
// No float atomics and no library call.  Rows (bank gradient: 128-sample tiles) are cut into contiguous chunks, at most
// *_MAX_COPIES of them, so above *_CHUNK x *_MAX_COPIES rows (64 tiles) a chunk grows: a work-group then walks more rows, and
// the bank gradient's several 128-sample tiles, re-staging its LDS image between them.  Every work-group owns ONE chunk and
// writes one partial (there is no grid-stride loop over chunks); partial_reduce adds the partials.  Every sum's order depends on the shape alone, so two runs are bitwise equal.
#include <stdint.h>
#include "sincnet_net.h"
#include "bn_train.h"
#include "wgrad_reduce.h"

namespace {

constexpr int SW_CHUNK = 64;             // rows per partial of sn_wgrad_kernel, at the least
constexpr int SW_MAX_COPIES = 64;
constexpr int OW_CHUNK = 256;            // rows per partial of sn_out_wgrad_kernel, at the least
constexpr int OW_MAX_COPIES = 256;
constexpr int BG_MAX_COPIES = 64;        // partials of sn_bank_grad_kernel (a chunk is whole 128-sample tiles)
constexpr int ST_CHUNK = 256;            // rows per partial of the statistics kernels, at the least
constexpr int ST_MAX_COPIES = 1024;

inline int dims_ok(int64_t N, int64_t L) {
    if (N <= 0 || L <= 0) return STOF_ERR_BAD_ARG;
    if (N * L >= (1ll << 31) - 64 || N * (L + GAP) + GAP >= (1ll << 31) - 64) return STOF_ERR_UNSUPPORTED;   // 32-bit rows
    if ((N * (L + GAP) + GAP) * C >= (1ll << 40)) return STOF_ERR_UNSUPPORTED;
    return STOF_OK;
}

// Blob of the training kernels (floats): frag0, frag1, frag2 as in the inference blob, bank_t [1024][128] (row 1023 zero),
// w3 [7][128].
struct TrainLayout {
    int64_t frag0, bank_t, frag1, frag2, w3, total;
};
inline TrainLayout train_layout() {
    TrainLayout o{};
    int64_t at = 0;
    o.frag0 = at; at = align_up(at + (int64_t)C * K0P);
    o.bank_t = at; at = align_up(at + (int64_t)C * K0P);
    o.frag1 = at; at = align_up(at + (int64_t)C * K1 * C);
    o.frag2 = at; at = align_up(at + (int64_t)C * K2 * C);
    o.w3 = at; at = align_up(at + K3 * C);
    o.total = at;
    return o;
}

// the 128-channel tensors as a view of bn_train.h: row m = n L + t of the GAP layout
struct GapRows {
    int L;
    __host__ __device__ int channels() const { return C; }
    __device__ long long at(long long m, int c) const { return ((long long)GAP + (long long)((int)m / L) * GAP + m) * C + c; }
    __device__ void split(long long e, long long& m, int& c) const { m = e / C; c = (int)(e % C); }
};

// ------------------------------------------------------------------------------------------------------------- packing
__global__ __launch_bounds__(256) void sn_pack_bank_kernel(double fs, const float* __restrict__ low_hz, const float* __restrict__ band_hz,
                                                           float* __restrict__ frag, float* __restrict__ bank_t) {
#pragma clang fp contract(off)                                    // the host packer's operations, one rounding each
    const int o = blockIdx.x * 256 + threadIdx.x;                 // (filter c, tap j = 0 .. 511)
    if (o >= C * (HALF0 + 1)) return;
    const int c = o / (HALF0 + 1), j = o - c * (HALF0 + 1);
    const SincBand b = sinc_band(fs, low_hz[c], band_hz[c]);
    const double pi = 3.14159265358979323846;
    float v;
    if (j == HALF0) {
        v = (float)(2.0 * b.band / (2.0 * b.band));
    } else {
        const double u = (double)j * (K0 / 2.0 - 1.0) / (HALF0 - 1);
        const double win = 0.54 - 0.46 * cos(2.0 * pi * u / K0);
        const double nn = 2.0 * pi * (double)(j - HALF0) / fs;
        v = (float)((sin(b.high * nn) - sin(b.low * nn)) / (nn / 2.0) * win / (2.0 * b.band));
    }
    constexpr int G = K0P / 8;
    const int nt = c >> 5, i = c & 31;
    for (int side = 0; side < (j == HALF0 ? 1 : 2); ++side) {
        const int k = side == 0 ? j : K0 - 1 - j;
        frag[(((long long)nt * G + (k >> 3)) * 64 + ((k >> 2) & 1) * 32 + i) * 4 + (k & 3)] = v;
        if (bank_t) bank_t[k * C + c] = v;
    }
}

// The forward image of a conv weight (128, 128, KT) is pack_frag32 of mfma32_frag.h with k = tap * 128 + c.  This is the data
// gradient's image in the same order: row oc = INPUT channel, W[c][oc][KT - 1 - tap].
__global__ __launch_bounds__(256) void sn_dgrad_image_kernel(const float* __restrict__ w, int KT, float* __restrict__ out, int total) {
    const int o = blockIdx.x * 256 + threadIdx.x;
    if (o >= total) return;
    int nt, oc, k;
    frag_decode(o, KT * C / 8, nt, oc, k);
    const int tap = k / C, c = k - tap * C;
    out[o] = w[((size_t)c * C + oc) * KT + (KT - 1 - tap)];
}

// the forward image of conv.1 / conv.2
inline void pack_conv_frag(hipStream_t s, const float* w, int KT, float* out) {
    pack_frag32_device(s, w, C, C, KT, C, KT * C / 8, out, C * KT * C);
}

__global__ __launch_bounds__(256) void sn_pack_w3_kernel(const float* __restrict__ w, float* __restrict__ out) {
    const int o = blockIdx.x * 256 + threadIdx.x;
    if (o >= K3 * C) return;
    const int j = o / C, ci = o - j * C;
    out[o] = w[ci * K3 + j];
}

// bn_affine of the host packer (sincnet.hip) for the `channels` channels of one layer: s, t of the eval-mode BatchNorm with the
// conv bias (NULL: none) folded in, the same operations in the same order, without contraction
__global__ __launch_bounds__(128) void sn_pack_affine_kernel(const float* __restrict__ gamma, const float* __restrict__ beta,
                                                             const float* __restrict__ mean, const float* __restrict__ var,
                                                             const float* __restrict__ bias, double eps, int channels,
                                                             float* __restrict__ s, float* __restrict__ t) {
#pragma clang fp contract(off)
    const int c = threadIdx.x;
    if (c >= channels) return;
    const double sc = (double)gamma[c] / sqrt((double)var[c] + eps);
    s[c] = (float)sc;
    t[c] = (float)(((bias ? (double)bias[c] : 0.0) - (double)mean[c]) * sc + (double)beta[c]);
}

// zero gap rows of one buffer in the GAP layout
__global__ __launch_bounds__(256) void sn_gaps1_kernel(float* __restrict__ b, long long L, long long total) {
    const long long o = (long long)blockIdx.x * 256 + threadIdx.x;
    if (o >= total) return;
    const long long g = o / (GAP * C), w = o % (GAP * C);
    b[g * (L + GAP) * C + w] = 0.f;
}

// ----------------------------------------------------------------------------------------------------------- BatchNorm
// What SincNet brings to bn_train.h.  Layers 0..2: SincAct<true> on the GAP layout, four channels per thread, two row parts
// per channel; layer 3: SincAct<false> (no activation, `a` is not read) on the flat tensor, 256 row parts.  Both fold their
// parts in ascending order and cut the rows by the balanced rule.
template <bool LEAKY>
struct SincAct {
    static constexpr bool reads_a = LEAKY;
    __device__ static double g(float da, float a) { return (double)(LEAKY ? (a > 0.f ? da : 0.2f * da) : da); }     // the slope in fp32
    __device__ static double seen(double xh) { return (double)(float)xh; }                                          // xhat rounded to fp32
    __device__ static double scale(const float* gamma, const double* stat, int C, int c) { return (double)gamma[c] * stat[C + c]; }
    __device__ static float out(double u) { return LEAKY ? leaky((float)u) : (float)u; }
};

// ------------------------------------------------------------------------------------------ weight gradient, layers 1, 2
// grid (chunk, KT, 4 co tiles); wave w of a work-group takes k tile 4 blockIdx.y + w (KT * 4 tiles of 32: all full).  MFMA
// operands: A[co][r] = dz of row pair member r = lane >> 5, B[r][k] = a_prev at GAP row R - P of that row, offset k (the same
// contiguous run the forward reads).  D: column (lane & 31) = k, rows = co.  Partial: dW [co][k], then db [co].
template <int KT>
__global__ __launch_bounds__(256) void sn_wgrad_kernel(const float* __restrict__ a_prev, const float* __restrict__ dz, int M, int L,
                                                       int rows_per, float* __restrict__ copies, int E) {
    constexpr int K = KT * C, P = (KT - 1) / 2;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int i = lane & 31, h = lane >> 5;
    const int kt = blockIdx.y * 4 + wave;
    const int k = kt * 32 + i, co = blockIdx.z * 32 + i;
    const int m_begin = blockIdx.x * rows_per;
    const int m_end = m_begin + rows_per < M ? m_begin + rows_per : M;
    f32x16 acc = {};
    float sb = 0.f;
    for (int mm = m_begin; mm < m_end; mm += 8) {                 // four row pairs per trip; a row past the chunk adds 0 x 0
        float av[4], bv[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int row = mm + 2 * u + h;
            av[u] = bv[u] = 0.f;
            if (row < m_end) {
                const long long R = (long long)GAP + (long long)(row / L) * GAP + row;
                av[u] = dz[R * C + co];
                bv[u] = a_prev[(R - P) * C + k];
            }
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            acc = MFMA32(av[u], bv[u], acc);
            sb += av[u];
        }
    }
    float* copy = copies + (size_t)blockIdx.x * E;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int c = blockIdx.z * 32 + (r & 3) + 8 * (r >> 2) + 4 * h;
        copy[(size_t)c * K + k] = acc[r];
    }
    if (kt == 0) {
        const float s = sb + __shfl_xor(sb, 32);
        if (h == 0) copy[(size_t)C * K + co] = s;
    }
}

// --------------------------------------------------------------------------------------------------- layer 3, backward
// dw3[ci][j] = sum over rows of dz3[m] a2[m + j - 3][ci], db3 = sum dz3.  Thread (ci = tid & 127, part = tid >> 7) walks rows
// part, part + 2, ... of the chunk; part 1 is added to part 0 through LDS.  Partial: dw [ci * 7 + j], then db.
__global__ __launch_bounds__(256) void sn_out_wgrad_kernel(const float* __restrict__ a2, const float* __restrict__ dz3, int M, int L,
                                                           int rows_per, float* __restrict__ copies, int E) {
    __shared__ float red[C][K3 + 1];
    const int ci = threadIdx.x & 127, part = threadIdx.x >> 7;
    const int m_begin = blockIdx.x * rows_per;
    const int m_end = m_begin + rows_per < M ? m_begin + rows_per : M;
    float acc[K3 + 1];
#pragma unroll
    for (int j = 0; j <= K3; ++j) acc[j] = 0.f;
    for (int m = m_begin + part; m < m_end; m += 2) {
        const float d = dz3[m];
        const float* row = a2 + ((long long)GAP + (long long)(m / L) * GAP + m - 3) * C + ci;
#pragma unroll
        for (int j = 0; j < K3; ++j) acc[j] = fmaf(d, row[j * C], acc[j]);
        acc[K3] += d;
    }
    if (part == 1) {
#pragma unroll
        for (int j = 0; j <= K3; ++j) red[ci][j] = acc[j];
    }
    __syncthreads();
    if (part != 0) return;
    float* copy = copies + (size_t)blockIdx.x * E;
#pragma unroll
    for (int j = 0; j < K3; ++j) copy[ci * K3 + j] = acc[j] + red[ci][j];
    if (ci == 0) copy[C * K3] = acc[K3] + red[0][K3];
}

// da2[m][ci] = sum over taps j, in order, of w3[ci][j] dz3[n][t - j + 3]
__global__ __launch_bounds__(256) void sn_out_dgrad_kernel(const float* __restrict__ dz3, const float* __restrict__ w, long long total, int L,
                                                           float* __restrict__ da2) {
    const long long o = (long long)blockIdx.x * 256 + threadIdx.x;
    if (o >= total) return;
    const int m = (int)(o >> 7), ci = (int)(o & 127);
    const int n = m / L, t = m - n * L;
    float acc = 0.f;
#pragma unroll
    for (int j = 0; j < K3; ++j) {
        const int tt = t - j + 3;
        if (tt >= 0 && tt < L) acc = fmaf(w[ci * K3 + j], dz3[(long long)n * L + tt], acc);
    }
    da2[GapRows{L}.at(m, ci)] = acc;
}

// --------------------------------------------------------------------------------------------------- layer 0, backward
// grid (chunk of tiles, 8, 4 filter tiles); wave w takes tap tile kt = 4 blockIdx.y + w (32 tiles of 32 taps; tap 1023 is
// computed and dropped by the reduce).  Per 128-sample tile (n, t0) the work-group stages x[t0 - 511 .. t0 + 640] as
// sn_sinc_kernel does; A[c][r] = dz0[n][t0 + r][c] (0 past L), B[r][k] = xs[r + k].
__global__ __launch_bounds__(256) void sn_bank_grad_kernel(const float* __restrict__ x, const float* __restrict__ dz0, long long L,
                                                           long long tblocks, long long tiles, int tiles_per, float* __restrict__ copies) {
    __shared__ float xs[XS0];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int i = lane & 31, h = lane >> 5;
    const int k = (blockIdx.y * 4 + wave) * 32 + i, c = blockIdx.z * 32 + i;
    const long long tile_begin = (long long)blockIdx.x * tiles_per;
    const long long tile_end = tile_begin + tiles_per < tiles ? tile_begin + tiles_per : tiles;
    f32x16 acc = {};
    for (long long tile = tile_begin; tile < tile_end; ++tile) {
        const long long n = tile / tblocks, t0 = (tile % tblocks) * TILE0;
        const float* xr = x + n * L;
        __syncthreads();                                          // the previous tile's readers are done
        for (int j = threadIdx.x; j < XS0; j += 256) {
            const long long t = t0 - HALF0 + j;
            xs[j] = (t >= 0 && t < L) ? xr[t] : 0.f;
        }
        __syncthreads();
        const float* drow = dz0 + (GAP + n * (L + GAP) + t0) * C + c;
        for (int r = 0; r < TILE0 && t0 + r < L; r += 8) {
            float av[4], bv[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int rr = r + 2 * u + h;
                av[u] = t0 + rr < L ? drow[(long long)rr * C] : 0.f;
                bv[u] = xs[rr + k];                                // rr + k <= 127 + 1023 < XS0
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) acc = MFMA32(av[u], bv[u], acc);
        }
    }
    float* copy = copies + (size_t)blockIdx.x * C * K0P;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int cr = blockIdx.z * 32 + (r & 3) + 8 * (r >> 2) + 4 * h;
        copy[(size_t)cr * K0P + k] = acc[r];
    }
}

// one work-group (a wave) per filter: lane l sums taps l, l + 64, ...; lane 0 adds the 64 sums in order and finishes
__global__ __launch_bounds__(64) void sn_band_grad_kernel(double fs, const float* __restrict__ low_hz, const float* __restrict__ band_hz,
                                                          const float* __restrict__ G, float* __restrict__ dlow_hz,
                                                          float* __restrict__ dband_hz) {
    __shared__ double red[2][64];
    const int c = blockIdx.x, l = threadIdx.x;
    const SincBand b = sinc_band(fs, low_hz[c], band_hz[c]);
    double dh = 0.0, dl = 0.0;
    sinc_band_grad_taps(fs, b, G + (size_t)c * K0, l, 64, &dh, &dl);
    red[0][l] = dh;
    red[1][l] = dl;
    __syncthreads();
    if (l != 0) return;
    for (int j = 1; j < 64; ++j) {
        dh += red[0][j];
        dl += red[1][j];
    }
    double o_low, o_band;
    sinc_band_grad_finish(b, low_hz[c], band_hz[c], dh, dl, &o_low, &o_band);
    dlow_hz[c] = (float)o_low;
    dband_hz[c] = (float)o_band;
}

// dx[n][s] = sum over taps k and filters c of dz0[n][s + 511 - k][c] bank[c][k].  Work-group = one sample; thread (c = tid &
// 127, half = tid >> 7) runs one fmaf chain over its taps k = k_lo + half, + 2, ...; the 256 chains fold through LDS in a fixed
// tree.
__global__ __launch_bounds__(256) void sn_in_dgrad_kernel(const float* __restrict__ dz0, const float* __restrict__ bank_t, int L,
                                                          float* __restrict__ dx) {
    __shared__ float red[256];
    const int m = blockIdx.x, n = m / L, s = m - n * L;
    const int c = threadIdx.x & 127, half = threadIdx.x >> 7;
    const int k_lo = s + HALF0 - (L - 1) > 0 ? s + HALF0 - (L - 1) : 0;           // t = s + 511 - k in [0, L)
    const int k_hi = s + HALF0 < K0 - 1 ? s + HALF0 : K0 - 1;
    const float* base = dz0 + ((long long)GAP + (long long)n * (L + GAP)) * C + c;
    float acc = 0.f;
    for (int k = k_lo + half; k <= k_hi; k += 2) acc = fmaf(base[(long long)(s + HALF0 - k) * C], bank_t[k * C + c], acc);
    red[threadIdx.x] = acc;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if (threadIdx.x < w) red[threadIdx.x] += red[threadIdx.x + w];
        __syncthreads();
    }
    if (threadIdx.x == 0) dx[m] = red[0];
}

int zero_gaps(hipStream_t s, float* buf, int64_t N, int64_t L) {
    const int64_t gaps = (N + 1) * GAP * C;
    hipLaunchKernelGGL(sn_gaps1_kernel, dim3((unsigned)((gaps + 255) / 256)), dim3(256), 0, s, buf, (long long)L, (long long)gaps);
    return launched();
}

}  // namespace

extern "C" size_t stof_sincnet_train_buffer_floats(int64_t N, int64_t L) {
    return dims_ok(N, L) == STOF_OK ? (size_t)buffer_floats(N, L) : 0;
}

// out[0 .. 5]: float offsets of frag0, bank_t, frag1, frag2, w3 in the training blob and its total
extern "C" int stof_sincnet_train_blob_layout(int64_t* out) {
    if (!out) return STOF_ERR_BAD_ARG;
    const TrainLayout o = train_layout();
    out[0] = o.frag0; out[1] = o.bank_t; out[2] = o.frag1; out[3] = o.frag2; out[4] = o.w3; out[5] = o.total;
    return STOF_OK;
}

// params: low_hz_, band_hz_, conv.1.weight, conv.2.weight, conv.3.weight (device)
extern "C" int stof_sincnet_train_pack(const stof_sincnet_desc* desc, const float* const* params, void* out, size_t out_bytes, void* stream) {
    if (!desc_ok(desc) || !params || !out) return STOF_ERR_BAD_ARG;
    for (int i = 0; i < 5; ++i)
        if (!params[i]) return STOF_ERR_BAD_ARG;
    const TrainLayout o = train_layout();
    if (out_bytes < (size_t)o.total * sizeof(float)) return STOF_ERR_WORKSPACE;
    float* const blob = static_cast<float*>(out);
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (hipMemsetAsync(blob, 0, (size_t)o.total * sizeof(float), s) != hipSuccess) return STOF_ERR_HIP;
    hipLaunchKernelGGL(sn_pack_bank_kernel, dim3((C * (HALF0 + 1) + 255) / 256), dim3(256), 0, s, desc->fs, params[0], params[1],
                       blob + o.frag0, blob + o.bank_t);
    pack_conv_frag(s, params[2], K1, blob + o.frag1);
    pack_conv_frag(s, params[3], K2, blob + o.frag2);
    hipLaunchKernelGGL(sn_pack_w3_kernel, dim3((K3 * C + 255) / 256), dim3(256), 0, s, params[4], blob + o.w3);
    return launched();
}

// stof_sincnet_pack_weights on the device: the 24 arrays in device memory -> the inference blob (the host packer's layout)
extern "C" int stof_sincnet_device_pack(const stof_sincnet_desc* desc, const float* const* params, void* out, size_t out_bytes,
                                        void* stream) {
    if (!desc_ok(desc) || !params || !out) return STOF_ERR_BAD_ARG;
    for (int i = 0; i < NUM_PARAMS; ++i)
        if (!params[i]) return STOF_ERR_BAD_ARG;
    const Layout o = layout();
    if (out_bytes < (size_t)o.total * sizeof(float)) return STOF_ERR_WORKSPACE;
    float* const blob = static_cast<float*>(out);
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (hipMemsetAsync(blob, 0, (size_t)o.total * sizeof(float), s) != hipSuccess) return STOF_ERR_HIP;
    hipLaunchKernelGGL(sn_pack_bank_kernel, dim3((C * (HALF0 + 1) + 255) / 256), dim3(256), 0, s, desc->fs, params[0], params[1],
                       blob + o.frag0, (float*)nullptr);
    pack_conv_frag(s, params[2], K1, blob + o.frag1);
    pack_conv_frag(s, params[4], K2, blob + o.frag2);
    hipLaunchKernelGGL(sn_pack_w3_kernel, dim3((K3 * C + 255) / 256), dim3(256), 0, s, params[6], blob + o.w3);
    const int64_t st_at[4] = {o.st0, o.st1, o.st2, o.st3};
    for (int l = 0; l < 4; ++l) {                                 // params 8 + 4 l ..: bn.l weight, bias, running_mean, running_var
        const int ch = l < 3 ? C : 1;
        hipLaunchKernelGGL(sn_pack_affine_kernel, dim3(1), dim3(128), 0, s, params[8 + 4 * l], params[9 + 4 * l], params[10 + 4 * l],
                           params[11 + 4 * l], l == 0 ? (const float*)nullptr : params[3 + 2 * (l - 1)], desc->bn_eps, ch, blob + st_at[l],
                           blob + st_at[l] + ch);
    }
    return launched();
}

// the data gradient's image of conv.`layer`.weight (layer 1 or 2): 128 * KT * 128 floats
extern "C" int stof_sincnet_train_dgrad_image(int32_t layer, const float* w, float* out, void* stream) {
    if ((layer != 1 && layer != 2) || !w || !out) return STOF_ERR_BAD_ARG;
    const int KT = layer == 1 ? K1 : K2, total = C * KT * C;
    hipLaunchKernelGGL(sn_dgrad_image_kernel, dim3((total + 255) / 256), dim3(256), 0, static_cast<hipStream_t>(stream), w, KT, out, total);
    return launched();
}

// Layer `layer`'s convolution without BatchNorm.  layer 0: in = x [N][L], bias ignored; 1, 2: in = a_{l-1} (GAP layout);
// 3: in = a_2, out = z_3 [N L] flat.  out of layers 0..2 is in the GAP layout; its gap rows are zeroed here.
extern "C" int stof_sincnet_train_conv(int32_t layer, const float* in, int64_t N, int64_t L, const void* blob_dev, const float* bias,
                                       float* out, void* stream) {
    if (layer < 0 || layer > 3 || !in || !blob_dev || !out || (layer > 0 && !bias)) return STOF_ERR_BAD_ARG;
    const int rc = dims_ok(N, L);
    if (rc != STOF_OK) return rc;
    const TrainLayout o = train_layout();
    const float* const blob = static_cast<const float*>(blob_dev);
    hipStream_t s = static_cast<hipStream_t>(stream);
    const bool narrow = N * L < NARROW_M;
    if (layer < 3 && zero_gaps(s, out, N, L) != STOF_OK) return STOF_ERR_HIP;
    if (layer == 0) {
        const int64_t tb0 = (L + TILE0 - 1) / TILE0;
        const dim3 grid((unsigned)(N * tb0), narrow ? 4 : 1);
        const float4* fr = reinterpret_cast<const float4*>(blob + o.frag0);
        if (narrow) hipLaunchKernelGGL((sn_sinc_kernel<1, EPI_BIAS>), grid, dim3(256), 0, s, in, (long long)L, (long long)tb0, fr, nullptr, out);
        else hipLaunchKernelGGL((sn_sinc_kernel<4, EPI_BIAS>), grid, dim3(256), 0, s, in, (long long)L, (long long)tb0, fr, nullptr, out);
        return launched();
    }
    const unsigned M = (unsigned)(N * L);
    if (layer == 3) {
        const int64_t tblocks = (L + OUT_T - 1) / OUT_T, waves = N * tblocks;
        hipLaunchKernelGGL(sn_out_kernel<EPI_BIAS>, dim3((unsigned)((waves + 3) / 4)), dim3(256), 0, s, in, (long long)N, (long long)L,
                           (long long)tblocks, blob + o.w3, bias, out);
        return launched();
    }
    const dim3 grid((unsigned)((M + 127) / 128), narrow ? 4 : 1);
    const float4* fr = reinterpret_cast<const float4*>(blob + (layer == 1 ? o.frag1 : o.frag2));
    if (layer == 1 && narrow) hipLaunchKernelGGL((sn_conv_kernel<K1, 1, EPI_BIAS>), grid, dim3(256), 0, s, in, M, (unsigned)L, fr, bias, out);
    if (layer == 1 && !narrow) hipLaunchKernelGGL((sn_conv_kernel<K1, 4, EPI_BIAS>), grid, dim3(256), 0, s, in, M, (unsigned)L, fr, bias, out);
    if (layer == 2 && narrow) hipLaunchKernelGGL((sn_conv_kernel<K2, 1, EPI_BIAS>), grid, dim3(256), 0, s, in, M, (unsigned)L, fr, bias, out);
    if (layer == 2 && !narrow) hipLaunchKernelGGL((sn_conv_kernel<K2, 4, EPI_BIAS>), grid, dim3(256), 0, s, in, M, (unsigned)L, fr, bias, out);
    return launched();
}

// da_{l-1} = the "same" convolution of dz_l (GAP layout, zero gap rows) with the image of stof_sincnet_train_dgrad_image
extern "C" int stof_sincnet_train_conv_dgrad(int32_t layer, const float* dz, int64_t N, int64_t L, const float* image, float* da,
                                             void* stream) {
    if ((layer != 1 && layer != 2) || !dz || !image || !da) return STOF_ERR_BAD_ARG;
    const int rc = dims_ok(N, L);
    if (rc != STOF_OK) return rc;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const bool narrow = N * L < NARROW_M;
    const unsigned M = (unsigned)(N * L);
    const dim3 grid((unsigned)((M + 127) / 128), narrow ? 4 : 1);
    const float4* fr = reinterpret_cast<const float4*>(image);
    if (zero_gaps(s, da, N, L) != STOF_OK) return STOF_ERR_HIP;
    if (layer == 1 && narrow) hipLaunchKernelGGL((sn_conv_kernel<K1, 1, EPI_NONE>), grid, dim3(256), 0, s, dz, M, (unsigned)L, fr, nullptr, da);
    if (layer == 1 && !narrow) hipLaunchKernelGGL((sn_conv_kernel<K1, 4, EPI_NONE>), grid, dim3(256), 0, s, dz, M, (unsigned)L, fr, nullptr, da);
    if (layer == 2 && narrow) hipLaunchKernelGGL((sn_conv_kernel<K2, 1, EPI_NONE>), grid, dim3(256), 0, s, dz, M, (unsigned)L, fr, nullptr, da);
    if (layer == 2 && !narrow) hipLaunchKernelGGL((sn_conv_kernel<K2, 4, EPI_NONE>), grid, dim3(256), 0, s, dz, M, (unsigned)L, fr, nullptr, da);
    return launched();
}

// workspace of the statistics and the BatchNorm backward, bytes (any channel count)
extern "C" size_t stof_sincnet_train_stats_workspace_bytes(void) { return ((size_t)ST_MAX_COPIES * 2 * C + 2 * C) * sizeof(double); }

// Batch statistics of z (channels = 128: GAP layout, channels = 1: flat [N L]) -> stat [4][channels] doubles (mean, rstd, s, t)
// and the new running statistics (temporaries: the module's buffers are not written).  N L >= 2.
extern "C" int stof_sincnet_train_stats(const stof_sincnet_desc* desc, const float* z, int64_t N, int64_t L, int32_t channels,
                                        const float* gamma, const float* beta, const float* run_mean, const float* run_var,
                                        double momentum, double* stat, float* new_mean, float* new_var, void* workspace,
                                        size_t workspace_bytes, void* stream) {
    if (!desc_ok(desc) || !z || !gamma || !beta || !run_mean || !run_var || !stat || !new_mean || !new_var || !workspace ||
        (channels != C && channels != 1))
        return STOF_ERR_BAD_ARG;
    const int rc = dims_ok(N, L);
    if (rc != STOF_OK) return rc;
    if (N * L < 2) return STOF_ERR_BAD_ARG;
    if (workspace_bytes < stof_sincnet_train_stats_workspace_bytes()) return STOF_ERR_WORKSPACE;
    hipStream_t s = static_cast<hipStream_t>(stream);
    double* part = static_cast<double*>(workspace);
    const Chunks ch = balanced_chunks(N * L, ST_CHUNK, ST_MAX_COPIES, 1);
    if (channels == C)
        return bn_stats_launch<C, FoldAscending>(s, z, N * L, GapRows{(int)L}, ch, desc->bn_eps, momentum, gamma, beta, run_mean, run_var, stat,
                                                 new_mean, new_var, part);
    return bn_stats_launch<1, FoldAscending>(s, z, N * L, Rows{1}, ch, desc->bn_eps, momentum, gamma, beta, run_mean, run_var, stat, new_mean,
                                             new_var, part);
}

// a = leaky(z s + t) into the GAP layout with zeroed gap rows (channels = 128) or y = z s + t flat (channels = 1)
extern "C" int stof_sincnet_train_apply(const float* z, int64_t N, int64_t L, int32_t channels, const double* stat, float* out, void* stream) {
    if (!z || !stat || !out || (channels != C && channels != 1)) return STOF_ERR_BAD_ARG;
    const int rc = dims_ok(N, L);
    if (rc != STOF_OK) return rc;
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (channels == 1) return bn_apply_launch<1, SincAct<false>>(s, z, N * L, Rows{1}, stat, out);
    if (zero_gaps(s, out, N, L) != STOF_OK) return STOF_ERR_HIP;
    return bn_apply_launch<4, SincAct<true>>(s, z, N * L, GapRows{(int)L}, stat, out);
}

// BatchNorm + LeakyReLU backward of one layer: da (the gradient of a; channels = 1: dy), a (NULL for channels = 1), z, stat of
// the forward -> dgamma, dbeta [channels] and dz (GAP layout with zeroed gap rows / flat)
extern "C" int stof_sincnet_train_bn_bwd(const float* da, const float* a, const float* z, const double* stat, const float* gamma,
                                         int64_t N, int64_t L, int32_t channels, float* dgamma, float* dbeta, float* dz,
                                         void* workspace, size_t workspace_bytes, void* stream) {
    if (!da || !z || !stat || !gamma || !dgamma || !dbeta || !dz || !workspace || (channels != C && channels != 1) ||
        (channels == C && !a))
        return STOF_ERR_BAD_ARG;
    const int rc = dims_ok(N, L);
    if (rc != STOF_OK) return rc;
    if (workspace_bytes < stof_sincnet_train_stats_workspace_bytes()) return STOF_ERR_WORKSPACE;
    hipStream_t s = static_cast<hipStream_t>(stream);
    double* part = static_cast<double*>(workspace);
    double* coef = part + (size_t)ST_MAX_COPIES * 2 * channels;
    const Chunks ch = balanced_chunks(N * L, ST_CHUNK, ST_MAX_COPIES, 1);
    if (channels == 1)
        return bn_bnb_launch<1, 1, FoldAscending, SincAct<false>>(s, da, nullptr, z, stat, gamma, N * L, Rows{1}, ch, dgamma, dbeta, dz, part, coef);
    if (zero_gaps(s, dz, N, L) != STOF_OK) return STOF_ERR_HIP;
    return bn_bnb_launch<4, C, FoldAscending, SincAct<true>>(s, da, a, z, stat, gamma, N * L, GapRows{(int)L}, ch, dgamma, dbeta, dz, part, coef);
}

extern "C" size_t stof_sincnet_train_conv_wgrad_workspace_bytes(int32_t layer) {
    if (layer != 1 && layer != 2) return 0;
    const int KT = layer == 1 ? K1 : K2;
    return (size_t)SW_MAX_COPIES * ((size_t)C * KT * C + C) * sizeof(float);
}

// dW, db of conv.`layer` (1 or 2) from a_{l-1} and dz_l, both in the GAP layout with zero gap rows
extern "C" int stof_sincnet_train_conv_wgrad(int32_t layer, const float* a_prev, const float* dz, int64_t N, int64_t L, float* dw,
                                             float* db, void* workspace, size_t workspace_bytes, void* stream) {
    if ((layer != 1 && layer != 2) || !a_prev || !dz || !dw || !db || !workspace) return STOF_ERR_BAD_ARG;
    const int rc = dims_ok(N, L);
    if (rc != STOF_OK) return rc;
    if (workspace_bytes < stof_sincnet_train_conv_wgrad_workspace_bytes(layer)) return STOF_ERR_WORKSPACE;
    const int KT = layer == 1 ? K1 : K2, K = KT * C, E = C * K + C;
    const int M = (int)(N * L);
    const Chunks ch = balanced_chunks(M, SW_CHUNK, SW_MAX_COPIES, 1);
    float* copies = static_cast<float*>(workspace);
    hipStream_t s = static_cast<hipStream_t>(stream);
    const dim3 grid((unsigned)ch.n, (unsigned)KT, 4);
    if (layer == 1) hipLaunchKernelGGL(sn_wgrad_kernel<K1>, grid, dim3(256), 0, s, a_prev, dz, M, (int)L, (int)ch.per, copies, E);
    else hipLaunchKernelGGL(sn_wgrad_kernel<K2>, grid, dim3(256), 0, s, a_prev, dz, M, (int)L, (int)ch.per, copies, E);
    if (launched() != STOF_OK) return STOF_ERR_HIP;
    partial_reduce(s, copies, ch.n, E, E, ConvTapsThenBias{dw, db, C, C, C, K, KT}, 1.f);
    return launched();
}

extern "C" size_t stof_sincnet_train_out_wgrad_workspace_bytes(void) { return (size_t)OW_MAX_COPIES * (C * K3 + 1) * sizeof(float); }

extern "C" int stof_sincnet_train_out_wgrad(const float* a2, const float* dz3, int64_t N, int64_t L, float* dw, float* db, void* workspace,
                                            size_t workspace_bytes, void* stream) {
    if (!a2 || !dz3 || !dw || !db || !workspace) return STOF_ERR_BAD_ARG;
    const int rc = dims_ok(N, L);
    if (rc != STOF_OK) return rc;
    if (workspace_bytes < stof_sincnet_train_out_wgrad_workspace_bytes()) return STOF_ERR_WORKSPACE;
    const int E = C * K3 + 1, M = (int)(N * L);
    const Chunks ch = balanced_chunks(M, OW_CHUNK, OW_MAX_COPIES, 1);
    float* copies = static_cast<float*>(workspace);
    hipStream_t s = static_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(sn_out_wgrad_kernel, dim3((unsigned)ch.n), dim3(256), 0, s, a2, dz3, M, (int)L, (int)ch.per, copies, E);
    if (launched() != STOF_OK) return STOF_ERR_HIP;
    partial_reduce(s, copies, ch.n, E, E, DwThenDb{dw, db, C * K3}, 1.f);
    return launched();
}

// da_2 (GAP layout, zeroed gap rows) from dz_3 [N L] and conv.3.weight [1][128][7]
extern "C" int stof_sincnet_train_out_dgrad(const float* dz3, const float* w, int64_t N, int64_t L, float* da2, void* stream) {
    if (!dz3 || !w || !da2) return STOF_ERR_BAD_ARG;
    const int rc = dims_ok(N, L);
    if (rc != STOF_OK) return rc;
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (zero_gaps(s, da2, N, L) != STOF_OK) return STOF_ERR_HIP;
    const long long total = N * L * C;
    hipLaunchKernelGGL(sn_out_dgrad_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, dz3, w, total, (int)L, da2);
    return launched();
}

extern "C" size_t stof_sincnet_train_bank_grad_workspace_bytes(void) { return (size_t)BG_MAX_COPIES * C * K0P * sizeof(float); }

// G [128][1023] = d loss / d filter bank from x [N][L] and dz_0 (GAP layout)
extern "C" int stof_sincnet_train_bank_grad(const float* x, const float* dz0, int64_t N, int64_t L, float* G, void* workspace,
                                            size_t workspace_bytes, void* stream) {
    if (!x || !dz0 || !G || !workspace) return STOF_ERR_BAD_ARG;
    const int rc = dims_ok(N, L);
    if (rc != STOF_OK) return rc;
    if (workspace_bytes < stof_sincnet_train_bank_grad_workspace_bytes()) return STOF_ERR_WORKSPACE;
    const int64_t tblocks = (L + TILE0 - 1) / TILE0, tiles = N * tblocks;
    const Chunks ch = balanced_chunks(tiles, 1, BG_MAX_COPIES, 1);
    float* copies = static_cast<float*>(workspace);
    hipStream_t s = static_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(sn_bank_grad_kernel, dim3((unsigned)ch.n, 8, 4), dim3(256), 0, s, x, dz0, (long long)L, (long long)tblocks,
                       (long long)tiles, (int)ch.per, copies);
    if (launched() != STOF_OK) return STOF_ERR_HIP;
    partial_reduce(s, copies, ch.n, C * K0P, C * K0P, BankTaps{G, K0, K0P}, 1.f);      // the packed tap 1023 is dropped
    return launched();
}

// d low_hz_, d band_hz_ [128] from G [128][1023], all on the device
extern "C" int stof_sincnet_train_band_grad(const stof_sincnet_desc* desc, const float* low_hz, const float* band_hz, const float* G,
                                            float* dlow_hz, float* dband_hz, void* stream) {
    if (!desc_ok(desc) || !low_hz || !band_hz || !G || !dlow_hz || !dband_hz) return STOF_ERR_BAD_ARG;
    hipLaunchKernelGGL(sn_band_grad_kernel, dim3(C), dim3(64), 0, static_cast<hipStream_t>(stream), desc->fs, low_hz, band_hz, G, dlow_hz,
                       dband_hz);
    return launched();
}

// dx [N][L] from dz_0 (GAP layout) and the training blob (its bank_t)
extern "C" int stof_sincnet_train_in_dgrad(const float* dz0, const void* blob_dev, int64_t N, int64_t L, float* dx, void* stream) {
    if (!dz0 || !blob_dev || !dx) return STOF_ERR_BAD_ARG;
    const int rc = dims_ok(N, L);
    if (rc != STOF_OK) return rc;
    const TrainLayout o = train_layout();
    hipLaunchKernelGGL(sn_in_dgrad_kernel, dim3((unsigned)(N * L)), dim3(256), 0, static_cast<hipStream_t>(stream), dz0,
                       static_cast<const float*>(blob_dev) + o.bank_t, (int)L, dx);
    return launched();
}
