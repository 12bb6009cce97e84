// Kuleshov training on gfx950 (models/kuleshov.py with num_layers = 4 in train mode): the stages of one step, one kernel each,
// staged through device memory, exact fp32 (v_mfma_f32_32x32x2_f32 where the work is a wide convolution), no float atomic and
// no library call: every sum has an order that depends on the shape alone, so two runs are bitwise equal.  Activations are
// channel-last fp32 as in kuleshov.hip, whose convolution, final_conv and output_fc kernels are kuleshov_net.h.  The host side
// (stofnet_amd/kuleshov_training.py) chains the stages; every entry here works on one layer.
//
// Dropout that can be replayed.  The keep-mask is a pure function (philox.h, Philox4x32-10):
//     key = (seed lo, seed hi), counter = (e >> 2, row n, call, (rank << 3) | site), word e & 3
//     site = 0 for the bottleneck, 1 .. 4 for up 0 .. 3; e = t C + c indexes the layer's unshuffled [position][channel] output of row n
//     kept when word >= floor(p 2^32); kept values are scaled by 1.0f / (1.0f - p)
// The mask is never stored: the backward computes it again.  stof_kuleshov_dropout_keep returns it on the host.
//
// Forward:
//   kt_pack_frag_kernel     a raw weight [cout][cin][taps] -> the fragment image of ks_conv_kernel: the forward's (kind 0), the
//                           stride-1 data gradient's W'[ci][j cout + co] = W[co][ci][taps - 1 - j] (kind 1), and the two parity
//                           classes of the stride-2 data gradient, W'[ci][j cout + co] = W[co][ci][par + 2 (J - 1 - j)] with
//                           J = (taps + 1 - par) / 2 taps of parity par (kinds 2, 3)
//   kt_down0_kernel         down_conv0 on the vector pipe: u = leaky0.01(conv + b)
//   ks_conv_kernel<TRAIN>   down 1..3 (u = leaky0.01(conv + b)), the bottleneck and up 0..3 (z = conv + b), dense [N][Lout][Cout]
//   bn_train.h              the batch statistics of u (down) or z (up): double sums, fixed fold, never a module buffer
//   kt_apply_down_kernel    a = leaky0.2(u s + t), the affine in double, rounded once, into the skip rows of the concatenation
//   kt_apply_up_kernel      a = (z s + t) keep scale at the pixel-shuffled address of the concatenation
//   kt_apply_bott_kernel    leaky0.2(z keep scale)
//   ks_final_kernel, ks_fc_kernel   as in inference, on images packed on the device; flat is kept
// Backward:
//   kt_fc_dflat_kernel      dflat = dy W, W read in its natural [O][2 F] layout; four interleaved chains over o, folded in pairs
//   kt_fc_dw_kernel         dW = dy^T flat: every element once, one chain over the rows; kt_fc_db_kernel: db
//   kt_final_dgrad_kernel, kt_final_wgrad_kernel   final_conv (128 -> 2, 9 taps) on the vector pipe
//   kt_gather_up_kernel     g = (gradient at the shuffled address) keep scale
//   kt_gather_down_kernel   g = (skip rows' part, then + the next convolution's data gradient) (a > 0 ? 1 : 0.2)
//   kt_gather_bott_kernel   dz = g (z > 0 ? 1 : 0.2) keep scale
//   bn_train.h + kt_dz_kernel   dbeta, dgamma and dz = s (g - mean g - xhat mean(g xhat)) (u > 0 ? 1 : 0.01) in double
//   kt_wgrad_kernel         the eight wide convolutions: M = Cout, N = (tap, Cin), K over the rows (n, t), stride 1 or 2.  A wave owns
//                           32 output channels x 128 columns of one chunk of rows; one partial per chunk -> partial_reduce.  The
//                           bias gradient is the column sum of dz (double, bn_train.h's chunk skeleton).
//   ks_conv_kernel<TRAIN>   the data gradients: stride 1 on the flipped image over dz with taps - 1 zero rows on either side;
//                           stride 2 as two parity classes, each with its own image, over dz with (taps - 1) / 2 zero rows on either
//                           side.  Input rows that no output reaches read zero rows only.
// The training convolutions sum their K span in partial chains of CHAIN_GROUPS K groups (kuleshov_net.h), the weight gradient in
// partial chains of WG_CHAIN rows; each chain is added to a running total when it ends.
//   kt_down0_wgrad_kernel, kt_down0_dgrad_kernel   down_conv0 on the vector pipe
//
// Bounded chunks, cut by fill_chunks of wgrad_reduce.h (rows per partial at the least / partials at the most):
//   statistics, BN backward, column sums  ST_ROWS = 256 / ST_MAX = 256       wide weight gradients  WG_ROWS = 256 / WG_MAX = 8
//   final_conv weights                    FW_ROWS = 256 / FW_MAX = 256       down_conv0 weights     D0_ROWS = 256 / D0_MAX = 256
// WG_MAX bounds the weight-gradient workspace: up_conv1's weight is 35 MB, so its partials take 285 MB at the most.
#include "kuleshov_net.h"
#include "philox.h"
#include "bn_train.h"
#include "wgrad_reduce.h"

namespace {

constexpr int ST_ROWS = 256, ST_MAX = 256;
constexpr int WG_ROWS = 256, WG_MAX = 8;
constexpr int WG_CHAIN = 256;                   // rows per partial chain inside a chunk of kt_wgrad_kernel
constexpr int FW_ROWS = 256, FW_MAX = 256;
constexpr int D0_ROWS = 256, D0_MAX = 256;
constexpr int MAX_C = 1024;
constexpr int FW_E = 2 * KB * C0 + 2;            // final_conv's partial: [oc][tap][ci], then the two biases
constexpr int D0_E = C0 * FS0 + C0;              // down_conv0's partial: [c][tap], then the biases
constexpr int D0_SLOTS = 33;                     // (taps + bias) / 2 per thread of kt_down0_wgrad_kernel

bool rows_ok(int64_t N, int64_t L) { return N >= 1 && L >= 1 && L < (1ll << 24) && N < (1ll << 31) && N * L < (1ll << 31) - 256; }
// sizes that are served one by one but whose product leaves 32-bit indexing
bool rows_overflow(int64_t N, int64_t L) { return N >= 1 && L >= 1 && L < (1ll << 24) && N < (1ll << 31) && N * L >= (1ll << 31) - 256; }
bool chan_ok(int c) { return c >= 128 && c <= MAX_C && c % 128 == 0; }
bool taps_ok(int t) { return t == 9 || t == 17 || t == 33 || t == 65; }
bool p_ok(double p) { return p >= 0.0 && p < 1.0; }

struct Drop {
    uint32_t k0, k1, call, c3;
    uint32_t thr;                // kept when word >= thr
    float scale;
};

Drop make_drop(uint64_t seed, uint32_t call, uint32_t rank, int site, double p) {
    Drop d;
    d.k0 = (uint32_t)seed;
    d.k1 = (uint32_t)(seed >> 32);
    d.call = call;
    d.c3 = (rank << 3) | (uint32_t)site;
    d.thr = (uint32_t)(uint64_t)(p * 4294967296.0);
    d.scale = 1.0f / (1.0f - (float)p);
    return d;
}

// keep scale (or 0) of elements e .. e + 3 of row n, e a multiple of 4
__host__ __device__ __forceinline__ void drop4(const Drop& d, long long n, long long e, float (&m)[4]) {
    const Philox ph = philox4x32_10((uint32_t)(e >> 2), (uint32_t)n, d.call, d.c3, d.k0, d.k1);
#pragma unroll
    for (int k = 0; k < 4; ++k) m[k] = ph.v[k] >= d.thr ? d.scale : 0.f;
}

// ------------------------------------------------------------------------------------------------------------ packing
__global__ __launch_bounds__(256) void kt_pack_frag_kernel(const float* __restrict__ w, int cin, int cout, int taps, int kind, int groups,
                                                           float* __restrict__ out, int total) {
    const int o = blockIdx.x * 256 + threadIdx.x;
    if (o >= total) return;
    int nt, oc, k;
    frag_decode(o, groups, nt, oc, k);
    const int width = kind == 0 ? cin : cout, j = k / width, c = k - j * width;
    float v;
    if (kind == 0) {
        v = w[((long long)oc * cin + c) * taps + j];
    } else {
        const int par = kind - 2, J = (taps + 1 - par) / 2;
        const int tap = kind == 1 ? taps - 1 - j : par + 2 * (J - 1 - j);
        v = w[((long long)c * cin + oc) * taps + tap];
    }
    out[o] = v;
}

// final_conv: weight [2][128][9] -> wf[oc][tap][ci]
__global__ __launch_bounds__(256) void kt_pack_final_kernel(const float* __restrict__ w, float* __restrict__ out) {
    const int o = blockIdx.x * 256 + threadIdx.x;
    if (o >= 2 * KB * C0) return;
    const int ci = o % C0, j = (o / C0) % KB, oc = o / (C0 * KB);
    out[o] = w[(oc * C0 + ci) * KB + j];
}

int frag_rows(int taps, int kind) { return kind <= 1 ? taps : (taps + 1 - (kind - 2)) / 2; }

// ---------------------------------------------------------------------------------------------------------- down 0
// thread (n, t, c): the 65 taps in one fma chain, as ks_down0_kernel
__global__ __launch_bounds__(256) void kt_down0_kernel(const float* __restrict__ x, long long xstride, long long total, int D0,
                                                       const float* __restrict__ w, const float* __restrict__ b, float* __restrict__ u) {
    const long long at = (long long)blockIdx.x * 256 + threadIdx.x;
    if (at >= total) return;
    const int c = (int)(at % C0);
    const long long nt = at / C0, n = nt / D0, t = nt - n * D0;
    const float* xr = x + n * xstride + 2 * t;
    const float* wr = w + c * FS0;
    float acc = 0.f;
#pragma unroll 5
    for (int j = 0; j < FS0; ++j) acc = fmaf(wr[j], xr[j], acc);
    u[at] = leaky(acc + b[c], 0.01f);
}

// ----------------------------------------------------------------------------------------------------------- BatchNorm
// What Kuleshov brings to bn_train.h: dense [rows][C] tensors, 64 channels per work-group with four row parts folded in pairs,
// the rows cut by the fill-to-minimum rule; the gradient behind the activation and the Dropout is prepared by the gather kernels.
struct KsAct {
    static constexpr bool reads_a = false;
    __device__ static double g(float da, float) { return (double)da; }
    __device__ static double seen(double xh) { return xh; }
    __device__ static double scale(const float*, const double* stat, int C, int c) { return stat[2 * C + c]; }
    __device__ static float out(double u) { return (float)u; }
};

// thread: four channels of one row; slope01: zu is the down blocks' u = leaky0.01(z), whose decision is u > 0
__global__ __launch_bounds__(256) void kt_dz_kernel(const float* __restrict__ g, const float* __restrict__ zu, const double* __restrict__ stat,
                                                    const double* __restrict__ coef, long long threads, int C, int slope01,
                                                    float* __restrict__ dz) {
    const long long o = (long long)blockIdx.x * 256 + threadIdx.x;
    if (o >= threads) return;
    const long long at = o * 4;
    const int c = (int)(at % C);
    float g4[4], z4[4], res[4];
    bn_load<4>(g + at, g4);
    bn_load<4>(zu + at, z4);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const double xh = ((double)z4[k] - stat[c + k]) * stat[C + c + k];
        const double d = stat[2 * C + c + k] * ((double)g4[k] - coef[c + k] - xh * coef[C + c + k]);
        res[k] = (float)(slope01 && !(z4[k] > 0.f) ? 0.01 * d : d);
    }
    bn_store<4>(dz + at, res);
}

__global__ __launch_bounds__(256) void kt_colsum_partial_kernel(const float* __restrict__ dz, long long M, long long rows_per, int C,
                                                                double* __restrict__ part) {
    chunk_sums<64, FoldPairs>([&](long long m, int c, double& v, double& w) { v = (double)dz[m * C + c]; w = 0.0; }, M, rows_per, C, part);
}

__global__ __launch_bounds__(64) void kt_colsum_final_kernel(const double* __restrict__ part, int copies, int C, float* __restrict__ db) {
    const int c = blockIdx.x * 64 + threadIdx.x;
    if (c >= C) return;
    double s = 0.0;
    for (int k = 0; k < copies; ++k) s += part[(long long)k * 2 * C + c];
    db[c] = (float)s;
}

// thread: four channels of (n, t).  a = leaky0.2(u s + t) into out + n out_n_stride + t C + c
__global__ __launch_bounds__(256) void kt_apply_down_kernel(const float* __restrict__ u, long long threads, int D, int C,
                                                            const double* __restrict__ stat, float* __restrict__ out, long long out_n_stride) {
    const long long o = (long long)blockIdx.x * 256 + threadIdx.x;
    if (o >= threads) return;
    const long long at = o * 4, m = at / C, n = m / D, t = m - n * D;
    const int c = (int)(at - m * C);
    float in[4], res[4];
    bn_load<4>(u + at, in);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const double v = fma((double)in[k], stat[2 * C + c + k], stat[3 * C + c + k]);
        res[k] = (float)(v > 0.0 ? v : 0.2 * v);
    }
    bn_store<4>(out + n * out_n_stride + t * C + c, res);
}

// thread: four channels c .. c + 3 of (n, t) of z [N][U][C]: channels c, c + 2 go to row 2 t, channels c + 1, c + 3 to row 2 t + 1 of
// the concatenation [.][C / 2], at columns c / 2, c / 2 + 1
__global__ __launch_bounds__(256) void kt_apply_up_kernel(const float* __restrict__ z, long long threads, int U, int C,
                                                          const double* __restrict__ stat, Drop drop, float* __restrict__ out,
                                                          long long out_n_stride) {
    const long long o = (long long)blockIdx.x * 256 + threadIdx.x;
    if (o >= threads) return;
    const long long at = o * 4, m = at / C, n = m / U, t = m - n * U;
    const int c = (int)(at - m * C);
    float in[4], res[4], mk[4];
    bn_load<4>(z + at, in);
    drop4(drop, n, t * C + c, mk);
#pragma unroll
    for (int k = 0; k < 4; ++k) res[k] = (float)fma((double)in[k], stat[2 * C + c + k], stat[3 * C + c + k]) * mk[k];
    float* const row = out + n * out_n_stride + 2 * t * (C >> 1) + (c >> 1);
    *reinterpret_cast<float2*>(row) = make_float2(res[0], res[2]);
    *reinterpret_cast<float2*>(row + (C >> 1)) = make_float2(res[1], res[3]);
}

__global__ __launch_bounds__(256) void kt_apply_bott_kernel(const float* __restrict__ z, long long threads, int B, int C, Drop drop,
                                                            float* __restrict__ out) {
    const long long o = (long long)blockIdx.x * 256 + threadIdx.x;
    if (o >= threads) return;
    const long long at = o * 4, m = at / C, n = m / B, t = m - n * B;
    const int c = (int)(at - m * C);
    float in[4], res[4], mk[4];
    bn_load<4>(z + at, in);
    drop4(drop, n, t * C + c, mk);
#pragma unroll
    for (int k = 0; k < 4; ++k) res[k] = leaky(in[k] * mk[k], 0.2f);
    bn_store<4>(out + at, res);
}

// ----------------------------------------------------------------------------------------------------- gradient routing
__global__ __launch_bounds__(256) void kt_gather_up_kernel(const float* __restrict__ dcat, long long dcat_n_stride, long long threads, int U,
                                                           int C, Drop drop, float* __restrict__ g) {
    const long long o = (long long)blockIdx.x * 256 + threadIdx.x;
    if (o >= threads) return;
    const long long at = o * 4, m = at / C, n = m / U, t = m - n * U;
    const int c = (int)(at - m * C);
    float mk[4], res[4];
    drop4(drop, n, t * C + c, mk);
    const float* const row = dcat + n * dcat_n_stride + 2 * t * (C >> 1) + (c >> 1);
    const float2 e = *reinterpret_cast<const float2*>(row), od = *reinterpret_cast<const float2*>(row + (C >> 1));
    res[0] = e.x * mk[0]; res[1] = od.x * mk[1]; res[2] = e.y * mk[2]; res[3] = od.y * mk[3];
    bn_store<4>(g + at, res);
}

// g = (dskip (+ dnext)) (a > 0 ? 1 : 0.2); dskip and a are rows of a concatenation buffer (n strides), dnext dense or NULL
__global__ __launch_bounds__(256) void kt_gather_down_kernel(const float* __restrict__ dskip, long long dskip_n_stride,
                                                             const float* __restrict__ dnext, const float* __restrict__ a,
                                                             long long a_n_stride, long long threads, int D, int C, float* __restrict__ g) {
    const long long o = (long long)blockIdx.x * 256 + threadIdx.x;
    if (o >= threads) return;
    const long long at = o * 4, m = at / C, n = m / D, t = m - n * D;
    const int c = (int)(at - m * C);
    float d4[4], e4[4] = {0.f, 0.f, 0.f, 0.f}, a4[4], res[4];
    bn_load<4>(dskip + n * dskip_n_stride + t * C + c, d4);
    if (dnext) bn_load<4>(dnext + at, e4);
    bn_load<4>(a + n * a_n_stride + t * C + c, a4);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const float s = dnext ? d4[k] + e4[k] : d4[k];
        res[k] = a4[k] > 0.f ? s : (float)(0.2 * (double)s);
    }
    bn_store<4>(g + at, res);
}

// dz = g (z keep > 0 ? 1 : 0.2) keep scale: the bottleneck's leaky0.2 sits behind its Dropout
__global__ __launch_bounds__(256) void kt_gather_bott_kernel(const float* __restrict__ g, const float* __restrict__ z, long long threads, int B,
                                                             int C, Drop drop, float* __restrict__ dz) {
    const long long o = (long long)blockIdx.x * 256 + threadIdx.x;
    if (o >= threads) return;
    const long long at = o * 4, m = at / C, n = m / B, t = m - n * B;
    const int c = (int)(at - m * C);
    float g4[4], z4[4], mk[4], res[4];
    bn_load<4>(g + at, g4);
    bn_load<4>(z + at, z4);
    drop4(drop, n, t * C + c, mk);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const float d = z4[k] * mk[k] > 0.f ? g4[k] : (float)(0.2 * (double)g4[k]);
        res[k] = d * mk[k];
    }
    bn_store<4>(dz + at, res);
}

// ------------------------------------------------------------------------------------------------ wide weight gradients
struct WgradArgs {
    const float* in;             // row 0 of waveform 0 of the forward's input range
    long long in_n_stride;
    const float* dz;             // dense [M][Cout]
    float* part;                 // [chunks][Cout][K], K = taps Cin, column tap Cin + ci
    long long M, rows_per, E;
    int Lout, Cin, Cout, stride;
};

// grid (chunk, Cout / 128, K / 128); wave w owns output channels 128 blockIdx.y + 32 w .. + 31 and columns 128 blockIdx.z .. + 127
// (one tap: Cin is a multiple of 128).  MFMA: A[i = co][k = row] = dz, B[k = row][j = ci] = in[n][stride t + tap], two rows per
// MFMA, rows ascending, in partial chains of WG_CHAIN rows that are added to a running total in order (a grown chunk holds
// thousands of rows); a row past the chunk's end is a zero.  D[co = (r & 3) + 8 (r >> 2) + 4 h][column = lane & 31].
__global__ __launch_bounds__(256) void kt_wgrad_kernel(const WgradArgs w) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int i = lane & 31, h = lane >> 5;
    const int co0 = 128 * blockIdx.y + 32 * wave, col0 = 128 * blockIdx.z;
    const int tap = col0 / w.Cin, ci0 = col0 - tap * w.Cin;
    const long long r_begin = blockIdx.x * w.rows_per, r_end = r_begin + w.rows_per < w.M ? r_begin + w.rows_per : w.M;
    long long r = r_begin + h;
    long long n = r / w.Lout;
    int t = (int)(r - n * w.Lout);
    f32x16 acc[4] = {}, total[4] = {};
    const long long step = (long long)w.stride * w.Cin;
    int since = 0;
    for (long long base = r_begin; base < r_end; base += 2, r += 2) {
        float a = 0.f, b[4] = {0.f, 0.f, 0.f, 0.f};
        if (r < r_end) {
            a = w.dz[r * w.Cout + co0 + i];
            const float* row = w.in + n * w.in_n_stride + t * step + (long long)tap * w.Cin + ci0 + i;
#pragma unroll
            for (int nt = 0; nt < 4; ++nt) b[nt] = row[32 * nt];
        }
#pragma unroll
        for (int nt = 0; nt < 4; ++nt) acc[nt] = MFMA32(a, b[nt], acc[nt]);
        t += 2;
        while (t >= w.Lout) { t -= w.Lout; ++n; }
        if (++since == WG_CHAIN / 2 || base + 2 >= r_end) {              // a partial chain ends: into the running total, in order
#pragma unroll
            for (int nt = 0; nt < 4; ++nt) {
                total[nt] += acc[nt];
                acc[nt] = f32x16{};
            }
            since = 0;
        }
    }
    float* const part = w.part + blockIdx.x * w.E;
    const long long K = w.E / w.Cout;
#pragma unroll
    for (int nt = 0; nt < 4; ++nt)
#pragma unroll
        for (int q = 0; q < 16; ++q) part[(co0 + (q & 3) + 8 * (q >> 2) + 4 * h) * K + col0 + 32 * nt + i] = total[nt][q];
}

// --------------------------------------------------------------------------------------------------------- output_fc
// thread: column k of dflat for four rows n0 .. n0 + 3; chains o mod 4 over o ascending, folded (c0 + c1) + (c2 + c3)
__global__ __launch_bounds__(256) void kt_fc_dflat_kernel(const float* __restrict__ dy, const float* __restrict__ w, int N, int O, int K2, int Kp,
                                                          float* __restrict__ dflat) {
    const int k = blockIdx.x * 256 + threadIdx.x, n0 = blockIdx.y * 4;
    if (k >= Kp) return;
    float acc[4][4] = {};
    if (k < K2) {
        for (int o = 0; o < O; o += 4) {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                if (o + j < O) {
                    const float wv = w[(long long)(o + j) * K2 + k];
#pragma unroll
                    for (int rr = 0; rr < 4; ++rr)
                        if (n0 + rr < N) acc[rr][j] = fmaf(dy[(long long)(n0 + rr) * O + o + j], wv, acc[rr][j]);
                }
            }
        }
    }
#pragma unroll
    for (int rr = 0; rr < 4; ++rr)
        if (n0 + rr < N) dflat[(long long)(n0 + rr) * Kp + k] = (acc[rr][0] + acc[rr][1]) + (acc[rr][2] + acc[rr][3]);
}

// thread (o = blockIdx.x, k): dW[o][k] = sum_n dy[n][o] flat[n][k], rows ascending
__global__ __launch_bounds__(256) void kt_fc_dw_kernel(const float* __restrict__ dy, const float* __restrict__ flat, int N, int O, int K2, int Kp,
                                                       float* __restrict__ dw) {
    const int k = blockIdx.y * 256 + threadIdx.x, o = blockIdx.x;
    if (k >= K2) return;
    float acc = 0.f;
    for (int n = 0; n < N; ++n) acc = fmaf(dy[(long long)n * O + o], flat[(long long)n * Kp + k], acc);
    dw[(long long)o * K2 + k] = acc;
}

__global__ __launch_bounds__(256) void kt_fc_db_kernel(const float* __restrict__ dy, int N, int O, float* __restrict__ db) {
    const int o = blockIdx.x * 256 + threadIdx.x;
    if (o >= O) return;
    double acc = 0.0;
    for (int n = 0; n < N; ++n) acc += (double)dy[(long long)n * O + o];
    db[o] = (float)acc;
}

// -------------------------------------------------------------------------------------------------------- final_conv
// thread (n, s, ci): dcat[n][s][ci] = sum_j sum_oc dflat[n][2 (s - j) + oc] w[oc][ci][j], taps ascending, one fma chain
__global__ __launch_bounds__(256) void kt_final_dgrad_kernel(const float* __restrict__ dflat, const float* __restrict__ w, long long total, int Lc,
                                                             int F, int Kp, float* __restrict__ dcat) {
    const long long at = (long long)blockIdx.x * 256 + threadIdx.x;
    if (at >= total) return;
    const int ci = (int)(at % C0);
    const long long ns = at / C0, n = ns / Lc;
    const int s = (int)(ns - n * Lc);
    const float* dr = dflat + n * Kp;
    float acc = 0.f;
#pragma unroll
    for (int j = 0; j < KB; ++j) {
        const int t = s - j;
        if (t < 0 || t >= F) continue;
        acc = fmaf(dr[2 * t], w[ci * KB + j], acc);
        acc = fmaf(dr[2 * t + 1], w[(C0 + ci) * KB + j], acc);
    }
    dcat[at] = acc;
}

// thread (ci = tid & 127, oc = tid >> 7) over the rows (n, t) of its chunk ascending: nine chains, and the bias (a double chain,
// rounded once per chunk) for ci = 0
__global__ __launch_bounds__(256) void kt_final_wgrad_kernel(const float* __restrict__ dflat, const float* __restrict__ cat, long long M, int Lc,
                                                             int F, int Kp, long long rows_per, float* __restrict__ part) {
    const int ci = threadIdx.x & 127, oc = threadIdx.x >> 7;
    const long long r0 = blockIdx.x * rows_per, r1 = r0 + rows_per < M ? r0 + rows_per : M;
    float acc[KB] = {};
    double bacc = 0.0;
    for (long long r = r0; r < r1; ++r) {
        const long long n = r / F, t = r - n * F;
        const float g = dflat[n * Kp + 2 * t + oc];
        const float* row = cat + (n * Lc + t) * C0 + ci;
#pragma unroll
        for (int j = 0; j < KB; ++j) acc[j] = fmaf(g, row[j * C0], acc[j]);
        bacc += (double)g;
    }
    float* const p = part + (long long)blockIdx.x * FW_E;
#pragma unroll
    for (int j = 0; j < KB; ++j) p[(oc * KB + j) * C0 + ci] = acc[j];
    if (ci == 0) p[2 * KB * C0 + oc] = (float)bacc;
}

// -------------------------------------------------------------------------------------------------- down 0, backward
// thread (c = tid & 127, half = tid >> 7): slots 33 half .. + 32 of (65 taps, bias) over the rows (n, t) of its chunk ascending
__global__ __launch_bounds__(256) void kt_down0_wgrad_kernel(const float* __restrict__ x, long long xstride, const float* __restrict__ dz,
                                                             long long M, int D0, long long rows_per, float* __restrict__ part) {
    const int c = threadIdx.x & 127, j0 = D0_SLOTS * (threadIdx.x >> 7);
    const long long r0 = blockIdx.x * rows_per, r1 = r0 + rows_per < M ? r0 + rows_per : M;
    float acc[D0_SLOTS] = {};
    for (long long r = r0; r < r1; ++r) {
        const long long n = r / D0, t = r - n * D0;
        const float g = dz[r * C0 + c];
        const float* xr = x + n * xstride + 2 * t + j0;
#pragma unroll
        for (int jj = 0; jj < D0_SLOTS; ++jj) acc[jj] = fmaf(g, j0 + jj < FS0 ? xr[jj] : 1.f, acc[jj]);
    }
    float* const p = part + (long long)blockIdx.x * D0_E;
#pragma unroll
    for (int jj = 0; jj < D0_SLOTS; ++jj) {
        const int j = j0 + jj;
        p[j < FS0 ? c * FS0 + j : C0 * FS0 + c] = acc[jj];
    }
}

// wave (n, s): dx[n][s] = sum over t ascending (0 <= s - 2 t <= 64) of sum_c dz[n][t][c] w[c][s - 2 t]; lane l owns channels 2 l,
// 2 l + 1, a fixed xor-butterfly sums the lanes
__global__ __launch_bounds__(256) void kt_down0_dgrad_kernel(const float* __restrict__ dz, const float* __restrict__ w, long long N, int L, int D0,
                                                             float* __restrict__ dx, long long dx_stride) {
    const int lane = threadIdx.x & 63;
    const long long wid = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (wid >= N * L) return;
    const long long n = wid / L;
    const int s = (int)(wid - n * L);
    int t_lo = (s - (FS0 - 1) + 1) / 2;
    if (t_lo < 0) t_lo = 0;
    int t_hi = s / 2;
    if (t_hi > D0 - 1) t_hi = D0 - 1;
    float acc = 0.f;
    for (int t = t_lo; t <= t_hi; ++t) {
        const int j = s - 2 * t;
        const float2 g = *reinterpret_cast<const float2*>(dz + (n * D0 + t) * C0 + 2 * lane);
        acc = fmaf(g.x, w[2 * lane * FS0 + j], acc);
        acc = fmaf(g.y, w[(2 * lane + 1) * FS0 + j], acc);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o);
    if (lane == 0) dx[n * dx_stride + s] = acc;
}

template <typename K, typename... A>
int go(K kernel, long long threads, hipStream_t s, A... args) {
    hipLaunchKernelGGL(kernel, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, s, args...);
    return launched();
}

size_t stats_ws_bytes() { return ((size_t)ST_MAX * 2 * MAX_C + 2 * MAX_C) * sizeof(double); }

}  // namespace

extern "C" int stof_kuleshov_dropout_keep(uint64_t seed, uint32_t call, uint32_t rank, int32_t site, int64_t n, int64_t count, double p,
                                          uint8_t* keep) {
    if (site < 0 || site > 4 || rank >= (1u << 29) || n < 0 || n >= (1ll << 32) || count < 0 || count >= (1ll << 34) || !p_ok(p) ||
        (count && !keep))
        return STOF_ERR_BAD_ARG;
    const Drop d = make_drop(seed, call, rank, site, p);
    for (int64_t e = 0; e < count; e += 4) {
        float m[4];
        drop4(d, n, e, m);
        for (int k = 0; k < 4 && e + k < count; ++k) keep[e + k] = m[k] != 0.f;
    }
    return STOF_OK;
}

extern "C" int stof_kuleshov_train_constants(int64_t* out) {
    if (!out) return STOF_ERR_BAD_ARG;
    const int64_t v[8] = {ST_ROWS, ST_MAX, WG_ROWS, WG_MAX, FW_ROWS, FW_MAX, D0_ROWS, D0_MAX};
    for (int i = 0; i < 8; ++i) out[i] = v[i];
    return STOF_OK;
}

extern "C" size_t stof_kuleshov_train_frag_floats(int32_t cin, int32_t cout, int32_t taps, int32_t kind) {
    if (!chan_ok(cin) || !chan_ok(cout) || !taps_ok(taps) || kind < 0 || kind > 3) return 0;
    return (size_t)cin * cout * frag_rows(taps, kind);
}

extern "C" int stof_kuleshov_train_pack_frag(const float* w, int32_t cin, int32_t cout, int32_t taps, int32_t kind, float* frag, void* stream) {
    const size_t total = stof_kuleshov_train_frag_floats(cin, cout, taps, kind);
    if (!total || !w || !frag) return STOF_ERR_BAD_ARG;
    const int width = kind == 0 ? cin : cout;
    return go(kt_pack_frag_kernel, (long long)total, static_cast<hipStream_t>(stream), w, (int)cin, (int)cout, (int)taps, (int)kind,
              frag_rows(taps, kind) * width / 8, frag, (int)total);
}

extern "C" int stof_kuleshov_train_pack_final(const float* w, float* image, void* stream) {
    if (!w || !image) return STOF_ERR_BAD_ARG;
    return go(kt_pack_final_kernel, 2 * KB * C0, static_cast<hipStream_t>(stream), w, image);
}

extern "C" size_t stof_kuleshov_train_fc_frag_floats(const stof_kuleshov_desc* desc) {
    Dims d;
    if (!dims(desc, &d) || d.OT * d.G * 256 >= (1ll << 31)) return 0;
    return (size_t)(d.OT * d.G * 256);
}

extern "C" int stof_kuleshov_train_pack_fc(const stof_kuleshov_desc* desc, const float* w, float* frag, void* stream) {
    Dims d;
    if (!dims(desc, &d) || !w || !frag) return STOF_ERR_BAD_ARG;
    if (d.OT * d.G * 256 >= (1ll << 31)) return STOF_ERR_UNSUPPORTED;
    pack_frag32_device(static_cast<hipStream_t>(stream), w, (int)d.O, 1, (int)(2 * d.F), 1, (int)d.G, frag, (int)(d.OT * d.G * 256));
    return launched();
}

extern "C" int stof_kuleshov_train_down0(const float* x, int64_t x_row_stride, int64_t N, int64_t L, const float* w, const float* b, float* u,
                                         void* stream) {
    if (rows_overflow(N, L)) return STOF_ERR_UNSUPPORTED;
    if (!rows_ok(N, L) || L < MIN_L || x_row_stride < L || !x || !w || !b || !u) return STOF_ERR_BAD_ARG;
    const int64_t D0 = (L - FS0) / 2 + 1;
    return go(kt_down0_kernel, N * D0 * C0, static_cast<hipStream_t>(stream), x, (long long)x_row_stride, (long long)(N * D0 * C0), (int)D0, w, b, u);
}

extern "C" int stof_kuleshov_train_conv(const float* in, int64_t in_n_stride, int64_t N, int64_t Lout, int32_t cin, int32_t cout, int32_t rows,
                                        int32_t stride, const float* frag, const float* bias, int32_t slope01, float* out,
                                        int64_t out_n_stride, int64_t out_t_stride, void* stream) {
    if (rows_overflow(N, Lout)) return STOF_ERR_UNSUPPORTED;
    if (!rows_ok(N, Lout) || !chan_ok(cin) || !chan_ok(cout) || rows < 1 || rows > 65 || (stride != 1 && stride != 2) || in_n_stride < 0 ||
        out_n_stride < 0 || out_t_stride < cout || !in || !frag || !out)
        return STOF_ERR_BAD_ARG;
    ConvArgs p{};
    p.in = in; p.in_n_stride = in_n_stride; p.out = out; p.out_n_stride = out_n_stride; p.out_t_stride = out_t_stride;
    p.frag = reinterpret_cast<const float4*>(frag); p.bias = bias; p.slope01 = slope01 ? 1 : 0;
    p.M = (unsigned)(N * Lout); p.Lout = (unsigned)Lout;
    p.Cin = cin; p.Cout = cout; p.stride = stride; p.G = rows * cin / 8;
    return launch_conv<true>(p, 0, static_cast<hipStream_t>(stream)) ? STOF_OK : STOF_ERR_HIP;
}

extern "C" size_t stof_kuleshov_train_stats_workspace_bytes(void) { return stats_ws_bytes(); }

extern "C" int stof_kuleshov_train_stats(const float* z, int64_t rows, int32_t ch, const float* gamma, const float* beta, const float* run_mean,
                                         const float* run_var, double eps, double momentum, double* stat, float* new_mean, float* new_var,
                                         void* workspace, size_t workspace_bytes, void* stream) {
    if (rows_overflow(rows, 1)) return STOF_ERR_UNSUPPORTED;
    if (!rows_ok(rows, 1) || rows < 2 || !chan_ok(ch) || !z || !gamma || !beta || !run_mean || !run_var || !stat || !new_mean || !new_var)
        return STOF_ERR_BAD_ARG;
    if (!workspace || workspace_bytes < stats_ws_bytes()) return STOF_ERR_WORKSPACE;
    return bn_stats_launch<64, FoldPairs>(static_cast<hipStream_t>(stream), z, rows, Rows{ch}, fill_chunks(rows, ST_ROWS, ST_MAX), eps, momentum,
                                          gamma, beta, run_mean, run_var, stat, new_mean, new_var, static_cast<double*>(workspace));
}

extern "C" int stof_kuleshov_train_apply_down(const float* u, int64_t N, int64_t D, int32_t ch, const double* stat, float* out,
                                              int64_t out_n_stride, void* stream) {
    if (rows_overflow(N, D)) return STOF_ERR_UNSUPPORTED;
    if (!rows_ok(N, D) || !chan_ok(ch) || out_n_stride < D * ch || !u || !stat || !out) return STOF_ERR_BAD_ARG;
    const long long threads = N * D * (ch / 4);
    return go(kt_apply_down_kernel, threads, static_cast<hipStream_t>(stream), u, threads, (int)D, (int)ch, stat, out, (long long)out_n_stride);
}

extern "C" int stof_kuleshov_train_apply_up(const float* z, int64_t N, int64_t U, int32_t ch, const double* stat, uint64_t seed, uint32_t call,
                                            uint32_t rank, int32_t site, double p, float* out, int64_t out_n_stride, void* stream) {
    if (rows_overflow(N, U)) return STOF_ERR_UNSUPPORTED;
    if (!rows_ok(N, U) || !chan_ok(ch) || out_n_stride < U * ch || site < 1 || site > 4 || rank >= (1u << 29) || !p_ok(p) || !z || !stat || !out)
        return STOF_ERR_BAD_ARG;
    const long long threads = N * U * (ch / 4);
    return go(kt_apply_up_kernel, threads, static_cast<hipStream_t>(stream), z, threads, (int)U, (int)ch, stat, make_drop(seed, call, rank, site, p),
              out, (long long)out_n_stride);
}

extern "C" int stof_kuleshov_train_apply_bott(const float* z, int64_t N, int64_t B, uint64_t seed, uint32_t call, uint32_t rank, double p,
                                              float* out, void* stream) {
    if (rows_overflow(N, B)) return STOF_ERR_UNSUPPORTED;
    if (!rows_ok(N, B) || rank >= (1u << 29) || !p_ok(p) || !z || !out) return STOF_ERR_BAD_ARG;
    const long long threads = N * B * (512 / 4);
    return go(kt_apply_bott_kernel, threads, static_cast<hipStream_t>(stream), z, threads, (int)B, 512, make_drop(seed, call, rank, 0, p), out);
}

extern "C" int stof_kuleshov_train_tail(const stof_kuleshov_desc* desc, const float* cat3, int64_t N, const float* final_image,
                                        const float* final_bias, const float* fc_frag, const float* fc_bias, float* flat, float* y,
                                        void* stream) {
    Dims d;
    if (!dims(desc, &d) || N < 1 || !cat3 || !final_image || !final_bias || !fc_frag || !fc_bias || !flat || !y) return STOF_ERR_BAD_ARG;
    if (N * d.Lc[NL - 1] >= (1ll << 31) - 256 || N * d.OT >= (1ll << 26)) return STOF_ERR_UNSUPPORTED;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int tbf = (int)((d.Kp / 2 + FIN_T - 1) / FIN_T);
    if (!launch(ks_final_kernel, dim3((unsigned)((N * tbf + 3) / 4)), s, cat3, (long long)N, (int)d.Lc[NL - 1], (int)d.F, (int)d.Kp, tbf,
                final_image, final_bias, flat, (float*)nullptr))
        return STOF_ERR_HIP;
    const float4* const fcfrag = reinterpret_cast<const float4*>(fc_frag);
    if (N <= 32)
        return launch(ks_fc_kernel<1, 8>, dim3((unsigned)d.OT), s, (const float*)flat, (int)d.Kp, (unsigned)N, 1, fcfrag, (int)d.G, fc_bias,
                      (int)d.O, y) ? STOF_OK : STOF_ERR_HIP;
    const int mg = (int)((N + 32 * FC_MT - 1) / (32 * FC_MT));
    return launch(ks_fc_kernel<FC_MT, 2>, dim3((unsigned)(d.OT * mg)), s, (const float*)flat, (int)d.Kp, (unsigned)N, mg, fcfrag, (int)d.G,
                  fc_bias, (int)d.O, y) ? STOF_OK : STOF_ERR_HIP;
}

extern "C" int stof_kuleshov_train_fc_bwd(const stof_kuleshov_desc* desc, const float* dy, const float* flat, const float* w, int64_t N,
                                          float* dflat, float* dw, float* db, void* stream) {
    Dims d;
    if (!dims(desc, &d) || N < 1 || !dy || !flat || !w || !dflat || !dw || !db) return STOF_ERR_BAD_ARG;
    if (N >= (1ll << 18) || d.Kp > 65535ll * 256) return STOF_ERR_UNSUPPORTED;          // the grids' second dimension
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int K2 = (int)(2 * d.F), Kp = (int)d.Kp, O = (int)d.O;
    hipLaunchKernelGGL(kt_fc_dflat_kernel, dim3((unsigned)((Kp + 255) / 256), (unsigned)((N + 3) / 4)), dim3(256), 0, s, dy, w, (int)N, O, K2, Kp,
                       dflat);
    if (launched() != STOF_OK) return STOF_ERR_HIP;
    hipLaunchKernelGGL(kt_fc_dw_kernel, dim3((unsigned)O, (unsigned)((K2 + 255) / 256)), dim3(256), 0, s, dy, flat, (int)N, O, K2, Kp, dw);
    if (launched() != STOF_OK) return STOF_ERR_HIP;
    return go(kt_fc_db_kernel, O, s, dy, (int)N, O, db);
}

extern "C" size_t stof_kuleshov_train_final_bwd_workspace_bytes(void) { return (size_t)FW_MAX * FW_E * sizeof(float); }

extern "C" int stof_kuleshov_train_final_bwd(const stof_kuleshov_desc* desc, const float* dflat, const float* cat3, const float* w, int64_t N,
                                             float* dcat3, float* dw, float* db, void* workspace, size_t workspace_bytes, void* stream) {
    Dims d;
    if (!dims(desc, &d) || N < 1 || !dflat || !cat3 || !w || !dcat3 || !dw || !db) return STOF_ERR_BAD_ARG;
    if (N * d.Lc[NL - 1] >= (1ll << 31) - 256) return STOF_ERR_UNSUPPORTED;
    if (!workspace || workspace_bytes < stof_kuleshov_train_final_bwd_workspace_bytes()) return STOF_ERR_WORKSPACE;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int Lc = (int)d.Lc[NL - 1], F = (int)d.F, Kp = (int)d.Kp;
    const long long total = N * Lc * C0, M = N * F;
    if (go(kt_final_dgrad_kernel, total, s, dflat, w, total, Lc, F, Kp, dcat3) != STOF_OK) return STOF_ERR_HIP;
    const Chunks cs = fill_chunks(M, FW_ROWS, FW_MAX);
    float* part = static_cast<float*>(workspace);
    hipLaunchKernelGGL(kt_final_wgrad_kernel, dim3(cs.n), dim3(256), 0, s, dflat, cat3, M, Lc, F, Kp, cs.per, part);
    if (launched() != STOF_OK) return STOF_ERR_HIP;
    partial_reduce(s, part, cs.n, FW_E, FW_E, ConvTapsThenBias{dw, db, 2, C0, C0, KB * C0, KB}, 1.f);
    return launched();
}

extern "C" int stof_kuleshov_train_gather_up(const float* dcat, int64_t dcat_n_stride, int64_t N, int64_t U, int32_t ch, uint64_t seed,
                                             uint32_t call, uint32_t rank, int32_t site, double p, float* g, void* stream) {
    if (rows_overflow(N, U)) return STOF_ERR_UNSUPPORTED;
    if (!rows_ok(N, U) || !chan_ok(ch) || dcat_n_stride < U * ch || site < 1 || site > 4 || rank >= (1u << 29) || !p_ok(p) || !dcat || !g)
        return STOF_ERR_BAD_ARG;
    const long long threads = N * U * (ch / 4);
    return go(kt_gather_up_kernel, threads, static_cast<hipStream_t>(stream), dcat, (long long)dcat_n_stride, threads, (int)U, (int)ch,
              make_drop(seed, call, rank, site, p), g);
}

extern "C" int stof_kuleshov_train_gather_down(const float* dskip, int64_t dskip_n_stride, const float* dnext, const float* a,
                                               int64_t a_n_stride, int64_t N, int64_t D, int32_t ch, float* g, void* stream) {
    if (rows_overflow(N, D)) return STOF_ERR_UNSUPPORTED;
    if (!rows_ok(N, D) || !chan_ok(ch) || dskip_n_stride < D * ch || a_n_stride < D * ch || !dskip || !a || !g) return STOF_ERR_BAD_ARG;
    const long long threads = N * D * (ch / 4);
    return go(kt_gather_down_kernel, threads, static_cast<hipStream_t>(stream), dskip, (long long)dskip_n_stride, dnext, a, (long long)a_n_stride,
              threads, (int)D, (int)ch, g);
}

extern "C" int stof_kuleshov_train_gather_bott(const float* g, const float* z, int64_t N, int64_t B, uint64_t seed, uint32_t call, uint32_t rank,
                                               double p, float* dz, void* stream) {
    if (rows_overflow(N, B)) return STOF_ERR_UNSUPPORTED;
    if (!rows_ok(N, B) || rank >= (1u << 29) || !p_ok(p) || !g || !z || !dz) return STOF_ERR_BAD_ARG;
    const long long threads = N * B * (512 / 4);
    return go(kt_gather_bott_kernel, threads, static_cast<hipStream_t>(stream), g, z, threads, (int)B, 512, make_drop(seed, call, rank, 0, p), dz);
}

extern "C" int stof_kuleshov_train_bn_bwd(const float* g, const float* zu, const double* stat, int64_t rows, int32_t ch, int32_t slope01,
                                          float* dgamma, float* dbeta, float* dz, void* workspace, size_t workspace_bytes, void* stream) {
    if (rows_overflow(rows, 1)) return STOF_ERR_UNSUPPORTED;
    if (!rows_ok(rows, 1) || rows < 2 || !chan_ok(ch) || !g || !zu || !stat || !dgamma || !dbeta || !dz) return STOF_ERR_BAD_ARG;
    if (!workspace || workspace_bytes < stats_ws_bytes()) return STOF_ERR_WORKSPACE;
    const Chunks cs = fill_chunks(rows, ST_ROWS, ST_MAX);
    double* part = static_cast<double*>(workspace);
    double* coef = part + (size_t)ST_MAX * 2 * MAX_C;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const Rows view{ch};
    hipLaunchKernelGGL((bn_bnb_partial_kernel<64, FoldPairs, KsAct, Rows>), dim3((unsigned)cs.n, (unsigned)((ch + 63) / 64)), dim3(256), 0, s, g,
                       (const float*)nullptr, zu, stat, (long long)rows, cs.per, view, part);
    if (launched() != STOF_OK) return STOF_ERR_HIP;
    hipLaunchKernelGGL(bn_bnb_final_kernel, dim3((unsigned)((ch + 63) / 64)), dim3(64), 0, s, part, cs.n, (int)ch, (long long)rows, dgamma, dbeta,
                       coef);
    if (launched() != STOF_OK) return STOF_ERR_HIP;
    const long long threads = rows * (ch / 4);
    return go(kt_dz_kernel, threads, s, g, zu, stat, (const double*)coef, threads, (int)ch, slope01 ? 1 : 0, dz);
}

extern "C" size_t stof_kuleshov_train_wgrad_workspace_bytes(int64_t N, int64_t Lout, int32_t cin, int32_t cout, int32_t taps) {
    if (!rows_ok(N, Lout) || !chan_ok(cin) || !chan_ok(cout) || !taps_ok(taps)) return 0;
    const Chunks cs = fill_chunks(N * Lout, WG_ROWS, WG_MAX);
    return (size_t)ST_MAX * 2 * MAX_C * sizeof(double) + (size_t)cs.n * cout * taps * cin * sizeof(float);
}

extern "C" int stof_kuleshov_train_wgrad(const float* in, int64_t in_n_stride, const float* dz, int64_t N, int64_t Lout, int32_t cin, int32_t cout,
                                         int32_t taps, int32_t stride, float* dw, float* db, void* workspace, size_t workspace_bytes,
                                         void* stream) {
    if (rows_overflow(N, Lout)) return STOF_ERR_UNSUPPORTED;
    if (!rows_ok(N, Lout) || !chan_ok(cin) || !chan_ok(cout) || !taps_ok(taps) || (stride != 1 && stride != 2) || in_n_stride < 0 || !in || !dz ||
        !dw || !db)
        return STOF_ERR_BAD_ARG;
    if (!workspace || workspace_bytes < stof_kuleshov_train_wgrad_workspace_bytes(N, Lout, cin, cout, taps)) return STOF_ERR_WORKSPACE;
    WgradArgs w{};
    w.in = in; w.in_n_stride = in_n_stride; w.dz = dz;
    w.M = N * Lout; w.Lout = (int)Lout; w.Cin = cin; w.Cout = cout; w.stride = stride;
    w.E = (long long)cout * taps * cin;
    if (w.E >= (1ll << 31)) return STOF_ERR_UNSUPPORTED;
    const Chunks cs = fill_chunks(w.M, WG_ROWS, WG_MAX);
    w.rows_per = cs.per;
    double* colpart = static_cast<double*>(workspace);
    w.part = reinterpret_cast<float*>(colpart + (size_t)ST_MAX * 2 * MAX_C);
    hipStream_t s = static_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(kt_wgrad_kernel, dim3((unsigned)cs.n, (unsigned)(cout / 128), (unsigned)(taps * cin / 128)), dim3(256), 0, s, w);
    if (launched() != STOF_OK) return STOF_ERR_HIP;
    partial_reduce(s, w.part, cs.n, (int)w.E, (int)w.E, ConvTapsThenBias{dw, db, cout, cin, cin, taps * cin, taps}, 1.f);
    if (launched() != STOF_OK) return STOF_ERR_HIP;
    const Chunks cc = fill_chunks(w.M, ST_ROWS, ST_MAX);
    hipLaunchKernelGGL(kt_colsum_partial_kernel, dim3((unsigned)cc.n, (unsigned)(cout / 64)), dim3(256), 0, s, dz, w.M, cc.per, (int)cout, colpart);
    if (launched() != STOF_OK) return STOF_ERR_HIP;
    hipLaunchKernelGGL(kt_colsum_final_kernel, dim3((unsigned)(cout / 64)), dim3(64), 0, s, (const double*)colpart, cc.n, (int)cout, db);
    return launched();
}

extern "C" size_t stof_kuleshov_train_dgrad_workspace_bytes(int64_t N, int64_t Lout, int32_t cout, int32_t taps, int32_t stride) {
    if (!rows_ok(N, Lout) || !chan_ok(cout) || !taps_ok(taps) || (stride != 1 && stride != 2)) return 0;
    const int64_t P = stride == 1 ? taps - 1 : (taps - 1) / 2;
    return (size_t)(N * (Lout + 2 * P) * cout) * sizeof(float);
}

// out [N][Lin][cin]: the gradient of the convolution's input from dz [N][Lout][cout]; frag0: the image of kind 1 (stride 1) or 2
// (stride 2), frag1: of kind 3 (stride 2 only)
extern "C" int stof_kuleshov_train_dgrad(const float* dz, int64_t N, int64_t Lout, int32_t cin, int32_t cout, int32_t taps, int32_t stride,
                                         const float* frag0, const float* frag1, int64_t Lin, float* out, void* workspace,
                                         size_t workspace_bytes, void* stream) {
    if (rows_overflow(N, Lout)) return STOF_ERR_UNSUPPORTED;
    if (!rows_ok(N, Lout) || !rows_ok(N, Lin) || !chan_ok(cin) || !chan_ok(cout) || !taps_ok(taps) || (stride != 1 && stride != 2) || !dz ||
        !frag0 || (stride == 2 && !frag1) || !out)
        return STOF_ERR_BAD_ARG;
    if (stride == 1 ? Lin != Lout + taps - 1 : (Lin < 2 * (Lout - 1) + taps || Lin > 2 * Lout + taps - 1)) return STOF_ERR_BAD_ARG;
    const size_t need = stof_kuleshov_train_dgrad_workspace_bytes(N, Lout, cout, taps, stride);
    if (!workspace || workspace_bytes < need) return STOF_ERR_WORKSPACE;
    const int64_t P = stride == 1 ? taps - 1 : (taps - 1) / 2, Lp = Lout + 2 * P;
    if (N * Lp >= (1ll << 31) - 256) return STOF_ERR_UNSUPPORTED;
    hipStream_t s = static_cast<hipStream_t>(stream);
    float* const pad = static_cast<float*>(workspace);
    if (hipMemsetAsync(pad, 0, need, s) != hipSuccess) return STOF_ERR_HIP;
    if (hipMemcpy2DAsync(pad + P * cout, sizeof(float) * (size_t)(Lp * cout), dz, sizeof(float) * (size_t)(Lout * cout),
                         sizeof(float) * (size_t)(Lout * cout), (size_t)N, hipMemcpyDeviceToDevice, s) != hipSuccess)
        return STOF_ERR_HIP;
    ConvArgs p{};
    p.in_n_stride = Lp * cout; p.out_n_stride = Lin * cin;
    p.Cin = cout; p.Cout = cin; p.stride = 1;
    if (stride == 1) {
        p.in = pad; p.out = out; p.out_t_stride = cin;
        p.frag = reinterpret_cast<const float4*>(frag0);
        p.M = (unsigned)(N * Lin); p.Lout = (unsigned)Lin; p.G = taps * cout / 8;
        return launch_conv<true>(p, 0, s) ? STOF_OK : STOF_ERR_HIP;
    }
    for (int par = 0; par < 2; ++par) {
        const int64_t J = (taps + 1 - par) / 2, Mp = (Lin - par + 1) / 2;
        p.in = pad + (P - J + 1) * cout; p.out = out + par * cin; p.out_t_stride = 2 * cin;
        p.frag = reinterpret_cast<const float4*>(par ? frag1 : frag0);
        p.M = (unsigned)(N * Mp); p.Lout = (unsigned)Mp; p.G = (int)(J * cout / 8);
        if (!launch_conv<true>(p, 0, s)) return STOF_ERR_HIP;
    }
    return STOF_OK;
}

extern "C" size_t stof_kuleshov_train_down0_bwd_workspace_bytes(void) { return (size_t)D0_MAX * D0_E * sizeof(float); }

// dx (NULL = not wanted): N rows of L floats, dx_row_stride apart
extern "C" int stof_kuleshov_train_down0_bwd(const float* x, int64_t x_row_stride, const float* dz, const float* w, int64_t N, int64_t L, float* dw,
                                             float* db, float* dx, int64_t dx_row_stride, void* workspace, size_t workspace_bytes,
                                             void* stream) {
    if (rows_overflow(N, L)) return STOF_ERR_UNSUPPORTED;
    if (!rows_ok(N, L) || L < MIN_L || x_row_stride < L || (dx && dx_row_stride < L) || !x || !dz || !w || !dw || !db) return STOF_ERR_BAD_ARG;
    if (!workspace || workspace_bytes < stof_kuleshov_train_down0_bwd_workspace_bytes()) return STOF_ERR_WORKSPACE;
    const int64_t D0 = (L - FS0) / 2 + 1, M = N * D0;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const Chunks cs = fill_chunks(M, D0_ROWS, D0_MAX);
    float* part = static_cast<float*>(workspace);
    hipLaunchKernelGGL(kt_down0_wgrad_kernel, dim3(cs.n), dim3(256), 0, s, x, (long long)x_row_stride, dz, (long long)M, (int)D0, cs.per, part);
    if (launched() != STOF_OK) return STOF_ERR_HIP;
    partial_reduce(s, part, cs.n, D0_E, D0_E, ConvTapsThenBias{dw, db, C0, 1, 1, FS0, FS0}, 1.f);
    if (launched() != STOF_OK) return STOF_ERR_HIP;
    if (!dx) return STOF_OK;
    hipLaunchKernelGGL(kt_down0_dgrad_kernel, dim3((unsigned)((N * L + 3) / 4)), dim3(256), 0, s, dz, w, (long long)N, (int)L, (int)D0, dx,
                       (long long)dx_row_stride);
    return launched();
}
