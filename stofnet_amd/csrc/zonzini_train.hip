// Training the Zonzini baselines (ZonziniNetSmall / ZonziniNetLarge) in exact fp32, one kernel per stage, on the layout of
// the inference file: act_l [N][Lp_l][cpad_l] channel-last with pad channels 0, sel_l [N][Lp_l][cpad_l] one selector byte per
// stored element (zonzini_net.h: 0 no gradient, 1 conv output 2p won the pool, 2 conv output 2p + 1 won).
//
//   forward               the kernels of zonzini_net.h with TRAIN = true: every pooled activation and its selectors are kept,
//                         the head also saves f [N][C] and h [N][1024] (post-ReLU).  y is bitwise the inference y.
//   zz_copy / zz_pack_fc1t_kernel, pack_frag32_kernel (mfma32_frag.h)
//                         the forward kernels' blob packed on the device from the parameters (bytes of the host packer)
//   zz_head_units_kernel  dfc2.weight, dfc2.bias, dfc1.bias: thread = fc1 unit, one chain over n = 0 .. N - 1
//   zz_head_w1_kernel     dfc1.weight [1024][C]: thread = element, one chain over n = 0 .. N - 1
//   zz_head_df_kernel     df [N][cpad] = dh W1 (pad 0), dh = dy w2 [h > 0]: four interleaved chains over the units (j mod 4),
//                         folded (s0 + s1) + (s2 + s3)
//   zz_wgrad_kernel       layers >= 2, v_mfma_f32_32x32x2_f32: dW[co][k] = sum over pooled rows m = (n, p) of
//                         dz_even[m][co] in[n][4p ..][k] + dz_odd[m][co] in[n][4p + 2 ..][k], k = tap * cpad_in + ci the same
//                         contiguous run the forward reads; dz_even = dOut where sel = 1, dz_odd = dOut where sel = 2, formed in
//                         the operand load (dz is never stored).  The reduction dimension is m: an MFMA takes two rows, the even
//                         then the odd window of each pair.  Work-group (chunk of rows, 4 k tiles, co tile) writes its tiles of
//                         the chunk's partial; db comes from the k tile 0 wave.  partial_reduce adds the partials.
//   zz_dgrad_kernel       layers >= 2, v_mfma_f32_32x32x2_f32: dIn[n][s][ci] = sum over the five taps j = s mod 2 + 2 jj and co of
//                         W[co][ci][j] dz[n][(s >> 1) - jj][co].  M = (n, u) with s = 2 u + parity (the two parities are separate
//                         row spaces with their own weight image), N = ci, K = 5 cpad_out.  Rows that no kept conv output reads
//                         are sums of exact zeros.  The ReLU / pool of the layer below is applied by whoever reads dIn, through
//                         that layer's selectors.
//   zz_in_wgrad_kernel    layer 1 (Cin = 1), vector pipe: thread = (channel, row part of 4), partials + partial_reduce
//   zz_in_dgrad_kernel    layer 1: dx [N][L], thread = sample; samples beyond the last kept window are exactly 0.0
//
// dOut of the last conv layer is the gradient of the global mean, df[n][c] / Lp for every p: its readers form it on the fly
// (`Grad`: strides and divisor), it is never stored.
//
// No float atomics and no library call.  A weight gradient's rows are cut into `copies` contiguous chunks of equal length (at
// least ZW_CHUNK / ZW1_CHUNK rows; the number of chunks is bounded by the workspace, so their length grows with the row count),
// every work-group owns one chunk (no work-group takes a second one) and writes one partial; the order of every sum depends on
// the shape alone, so two runs are bitwise equal.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "zonzini_net.h"
#include "wgrad_reduce.h"

namespace {

constexpr int ZW_CHUNK = 64;                          // pooled rows per partial of zz_wgrad_kernel, at the least
constexpr int ZW_MAX_COPIES = 64;                     // its partials, at the most, and ...
constexpr size_t ZW_WORKSPACE = (size_t)64 << 20;     // ... no more than fit in 64 MiB (Large's last layer: 32 of 250 x 2001 floats)
constexpr int ZW1_CHUNK = 256;                        // pooled rows per partial of zz_in_wgrad_kernel, at the least
constexpr int ZW1_MAX_COPIES = 512;

struct Shape {
    Geometry g;
    int64_t len[MAXL + 1];                            // len[l]: input length of conv layer l; len[l + 1] its pooled length
};

// geometry, batch and length checks of every entry, in the order of stof_zonzini_forward
int shape_of(const stof_zonzini_desc* desc, int64_t N, int64_t L, Shape& s) {
    if (!geometry(desc, s.g) || N <= 0) return STOF_ERR_BAD_ARG;
    if (L < s.g.min_len) return STOF_ERR_POOL_EMPTY;
    if (L > (1ll << 30) || N > (1ll << 30) || N * L > 0x7fffffffll) return STOF_ERR_UNSUPPORTED;     // rows are ints
    s.len[0] = L;
    for (int l = 0; l < s.g.layers; ++l) s.len[l + 1] = pooled_len(s.len[l]);
    return STOF_OK;
}

inline int64_t wgrad_e(const Geometry& g, int l) { return (int64_t)g.cout[l] * (KW * g.cpad[l - 1] + 1); }     // dW [co][k], then db
inline int wgrad_max_copies(const Geometry& g, int l) {
    const int64_t fit = (int64_t)(ZW_WORKSPACE / sizeof(float)) / wgrad_e(g, l);
    return (int)(fit < ZW_MAX_COPIES ? fit : ZW_MAX_COPIES);
}
inline int dgrad_groups(const Geometry& g, int l) { return (5 * g.cpad[l] + 7) / 8; }
inline int64_t dgrad_image_floats(const Geometry& g, int l) { return 2ll * ntiles(g.cpad[l - 1]) * dgrad_groups(g, l) * 256; }

// dOut[n][p][c] = g[n sn + p sp + c] / div: an inner layer's dIn (sn = Lp cpad, sp = cpad, div = 1: exact) or the mean's
// gradient (sn = cpad, sp = 0, div = Lp)
struct Grad {
    const float* g;
    long long sn, sp;
    float div;
};

// ---------------------------------------------------------------------------------------------------- the blob, on the device
// stof_zonzini_pack_weights' blob from parameters in device memory (after an optimizer step the next forward packs again: no
// trip through the host).  The blob is zeroed first; these kernels write the real elements, so it is the host packer's bytes.
__global__ __launch_bounds__(256) void zz_copy_kernel(const float* __restrict__ src, float* __restrict__ dst, int n) {
    const int o = blockIdx.x * 256 + threadIdx.x;
    if (o < n) dst[o] = src[o];
}

// fc1.weight [1024][C] -> fc1t [C][1024]
__global__ __launch_bounds__(256) void zz_pack_fc1t_kernel(const float* __restrict__ w1, int C, float* __restrict__ out) {
    const int o = blockIdx.x * 256 + threadIdx.x;
    if (o >= C * FC1) return;
    const int c = o / FC1, j = o - c * FC1;
    out[o] = w1[(size_t)j * C + c];
}

// ------------------------------------------------------------------------------------------------------------------ head
__global__ __launch_bounds__(256) void zz_head_units_kernel(const float* __restrict__ dy, const float* __restrict__ h,
                                                            const float* __restrict__ w2, int N, float* __restrict__ dw2,
                                                            float* __restrict__ db2, float* __restrict__ db1) {
    const int j = blockIdx.x * 256 + threadIdx.x;
    const float wj = w2[j];
    float s2 = 0.f, s1 = 0.f, sb = 0.f;
    for (int n = 0; n < N; ++n) {
        const float d = dy[n], hv = h[(size_t)n * FC1 + j];
        s2 = fmaf(d, hv, s2);
        s1 += hv > 0.f ? d * wj : 0.f;
        sb += d;
    }
    dw2[j] = s2;
    db1[j] = s1;
    if (j == 0) db2[0] = sb;
}

__global__ __launch_bounds__(256) void zz_head_w1_kernel(const float* __restrict__ dy, const float* __restrict__ h,
                                                         const float* __restrict__ w2, const float* __restrict__ f, int N, int C,
                                                         float* __restrict__ dw1) {
    const int o = blockIdx.x * 256 + threadIdx.x;
    if (o >= FC1 * C) return;
    const int j = o / C, c = o - j * C;
    const float wj = w2[j];
    float s = 0.f;
    for (int n = 0; n < N; ++n) {
        const float dh = h[(size_t)n * FC1 + j] > 0.f ? dy[n] * wj : 0.f;
        s = fmaf(dh, f[(size_t)n * C + c], s);
    }
    dw1[o] = s;
}

__global__ __launch_bounds__(256) void zz_head_df_kernel(const float* __restrict__ dy, const float* __restrict__ h,
                                                         const float* __restrict__ w2, const float* __restrict__ w1, int C, int cpad,
                                                         float* __restrict__ df) {
    __shared__ float dh[FC1];
    const int n = blockIdx.x, c = threadIdx.x;
    const float d = dy[n];
    for (int j = c; j < FC1; j += 256) dh[j] = h[(size_t)n * FC1 + j] > 0.f ? d * w2[j] : 0.f;
    __syncthreads();
    if (c >= cpad) return;
    float s[4] = {0.f, 0.f, 0.f, 0.f};
    if (c < C) {
        for (int j = 0; j < FC1; j += 4) {
#pragma unroll
            for (int e = 0; e < 4; ++e) s[e] = fmaf(dh[j + e], w1[(size_t)(j + e) * C + c], s[e]);
        }
    }
    df[(size_t)n * cpad + c] = (s[0] + s[1]) + (s[2] + s[3]);
}

// -------------------------------------------------------------------------------------------- weight gradient, layers >= 2
// grid (chunk, ceil(k tiles / 4), co tiles); wave w of a work-group takes k tile 4 blockIdx.y + w.  MFMA operands: A[co][r] =
// dz of row pair member r = lane >> 5, B[r][k] = the window of that row.  D: column (lane & 31) = k, rows = co.
__global__ __launch_bounds__(256) void zz_wgrad_kernel(const float* __restrict__ in, int Lin, int cpad_in, Grad dout,
                                                       const uint8_t* __restrict__ sel, int M, int Lp, int rows_per, int cout,
                                                       int cpad_out, int K, float* __restrict__ copies, int E) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int i = lane & 31, h = lane >> 5;
    const int kt = blockIdx.y * 4 + wave;
    if (kt * 32 >= K) return;
    const int k = kt * 32 + i, co = blockIdx.z * 32 + i;
    const bool k_ok = k < K, co_ok = co < cout;
    const int m_begin = blockIdx.x * rows_per;
    const int m_end = m_begin + rows_per < M ? m_begin + rows_per : M;
    f32x16 acc = {};
    float sb = 0.f;
    // four row pairs per trip: their operands are loaded before the first MFMA; a pair past the chunk's end adds 0 x 0
    for (int mm = m_begin; mm < m_end; mm += 8) {
        float ae[4], ao[4], be[4], bo[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int row = mm + 2 * u + h;
            ae[u] = ao[u] = be[u] = bo[u] = 0.f;
            if (row < m_end) {
                const int n = row / Lp, p = row - n * Lp;
                if (co_ok) {
                    const uint8_t s = sel[(size_t)row * cpad_out + co];
                    if (s != 0) {
                        const float d = dout.g[n * dout.sn + p * dout.sp + co] / dout.div;
                        ae[u] = s == 1 ? d : 0.f;
                        ao[u] = s == 2 ? d : 0.f;
                    }
                }
                if (k_ok) {
                    const float* w = in + ((size_t)n * Lin + 4 * p) * cpad_in + k;       // rows 4p .. 4p + 11 <= Lin - 1
                    be[u] = w[0];
                    bo[u] = w[2 * cpad_in];
                }
            }
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            acc = MFMA32(ae[u], be[u], acc);
            acc = MFMA32(ao[u], bo[u], acc);
            sb += ae[u] + ao[u];
        }
    }
    float* copy = copies + (size_t)blockIdx.x * E;
    if (k_ok) {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int c = blockIdx.z * 32 + (r & 3) + 8 * (r >> 2) + 4 * h;
            if (c < cout) copy[(size_t)c * K + k] = acc[r];
        }
    }
    if (kt == 0) {
        const float s = sb + __shfl_xor(sb, 32);
        if (h == 0 && co_ok) copy[(size_t)cout * K + co] = s;
    }
}

// --------------------------------------------------------------------------------------------- data gradient, layers >= 2
// Weight image of one layer: [parity][ci tile][K group][64 lanes][4] in the fragment order of mfma32_frag.h with
// k = jj * cpad_out + co: lane (i, h), element e of group q holds W[co][ci = 32 tile + i][tap 2 jj + parity] at
// k = 8 q + 4 h + e, 0 outside the real channels and past k = 5 cpad_out.
__global__ __launch_bounds__(256) void zz_dgrad_image_kernel(const float* __restrict__ w, int cout, int cin, int cpad_out, int nt_in,
                                                             int groups, float* __restrict__ out, int total) {
    const int o = blockIdx.x * 256 + threadIdx.x;
    if (o >= total) return;
    int tile, row, k;                                                 // tile = parity * nt_in + ci tile
    frag_decode(o, groups, tile, row, k);
    const int parity = tile / nt_in, ci = row - 32 * parity * nt_in;
    const int jj = k / cpad_out, co = k - jj * cpad_out;
    out[o] = (jj < 5 && co < cout && ci < cin) ? w[((size_t)co * cin + ci) * KW + 2 * jj + parity] : 0.f;
}

// grid (ceil(M tiles / 2), ceil(ci tiles / 2), parity); 4 waves = 2 M tiles x 2 ci tiles.  Row m = (n, u) of parity b is input
// row s = 2 u + b (U = ceil(Lin / 2) rows per waveform; s = Lin of an odd Lin computes and stores nothing).
__global__ __launch_bounds__(256) void zz_dgrad_kernel(Grad dout, const uint8_t* __restrict__ sel, int Lp, int cpad_out, int Mrows, int U,
                                                       int Lin, int cpad_in, int nt_in, int groups, const float4* __restrict__ image,
                                                       float* __restrict__ din) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int parity = blockIdx.z;
    const int nt = blockIdx.y * 2 + (wave & 1);
    if (nt >= nt_in) return;
    const int m0 = (blockIdx.x * 2 + (wave >> 1)) * 32;
    if (m0 >= Mrows) return;
    const int i = lane & 31, h = lane >> 5;
    const int m = m0 + i < Mrows ? m0 + i : Mrows - 1;
    const int n = m / U, u = m - n * U;
    const float4* bq = image + ((size_t)(parity * nt_in + nt) * groups) * 64 + lane;
    // the lane's A float4 of K group q: dz[n][u - jj][co0 .. co0 + 3], formed from dOut and the selectors
    auto load_a = [&](int q) {
        const int k0 = 8 * q + 4 * h;
        const int jj = k0 / cpad_out, co0 = k0 - jj * cpad_out;
        const int t = u - jj;                                         // conv output that tap 2 jj + parity of input row s feeds
        float4 a = make_float4(0.f, 0.f, 0.f, 0.f);
        if (jj < 5 && t >= 0 && t < 2 * Lp) {
            const int p = t >> 1;
            const uint32_t want = (uint32_t)(t & 1) + 1u;
            const uint32_t s4 = *reinterpret_cast<const uint32_t*>(sel + ((size_t)n * Lp + p) * cpad_out + co0);
            if (s4 != 0) {
                const float4 d = *reinterpret_cast<const float4*>(dout.g + n * dout.sn + p * dout.sp + co0);
                a.x = (s4 & 0xff) == want ? d.x / dout.div : 0.f;
                a.y = ((s4 >> 8) & 0xff) == want ? d.y / dout.div : 0.f;
                a.z = ((s4 >> 16) & 0xff) == want ? d.z / dout.div : 0.f;
                a.w = (s4 >> 24) == want ? d.w / dout.div : 0.f;
            }
        }
        return a;
    };
    f32x16 acc = {};
    float4 an = load_a(0), bn = bq[0];
    for (int q = 0; q < groups; ++q) {                                // the next group's operands are loaded before this group's MFMAs
        const float4 a = an, b = bn;
        if (q + 1 < groups) {
            an = load_a(q + 1);
            bn = bq[(size_t)(q + 1) * 64];
        }
        acc = MFMA32(a.x, b.x, acc);
        acc = MFMA32(a.y, b.y, acc);
        acc = MFMA32(a.z, b.z, acc);
        acc = MFMA32(a.w, b.w, acc);
    }
    const int ci = nt * 32 + i;
    if (ci >= cpad_in) return;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int row = m0 + (r & 3) + 8 * (r >> 2) + 4 * h;
        if (row >= Mrows) continue;
        const int rn = row / U, s = 2 * (row - rn * U) + parity;
        if (s < Lin) din[((size_t)rn * Lin + s) * cpad_in + ci] = acc[r];
    }
}

// ---------------------------------------------------------------------------------------------------------------- layer 1
// dw[c][j] = sum over pooled rows m = (n, p) with sel != 0 of dOut[m][c] x[n][4p + 2 (sel - 1) + j], db[c] = sum of the same
// dOut.  Thread (channel c = tid & 63, part = tid >> 6) walks rows part, part + 4, ... of the chunk; the four parts are added
// in order through LDS.  Partial: dw [c * 10 + j], then db [cout * 10 + c].
__global__ __launch_bounds__(256) void zz_in_wgrad_kernel(const float* __restrict__ x, int L, const float* __restrict__ dout,
                                                          const uint8_t* __restrict__ sel, int M, int Lp, int rows_per, int cout,
                                                          int cpad, float* __restrict__ copies, int E) {
    __shared__ float red[3][64][KW + 1];
    const int c = threadIdx.x & 63, part = threadIdx.x >> 6;
    const int m_begin = blockIdx.x * rows_per;
    const int m_end = m_begin + rows_per < M ? m_begin + rows_per : M;
    float acc[KW + 1];
#pragma unroll
    for (int j = 0; j <= KW; ++j) acc[j] = 0.f;
    if (c < cout) {
        for (int m = m_begin + part; m < m_end; m += 4) {
            const uint8_t s = sel[(size_t)m * cpad + c];
            if (s == 0) continue;
            const float d = dout[(size_t)m * cpad + c];
            const int n = m / Lp, p = m - n * Lp;
            const float* xs = x + (size_t)n * L + 4 * p + 2 * (s - 1);          // 4p + 2 + 9 <= L - 1
#pragma unroll
            for (int j = 0; j < KW; ++j) acc[j] = fmaf(d, xs[j], acc[j]);
            acc[KW] += d;
        }
    }
    if (part != 0) {
#pragma unroll
        for (int j = 0; j <= KW; ++j) red[part - 1][c][j] = acc[j];
    }
    __syncthreads();
    if (part != 0 || c >= cout) return;
    float* copy = copies + (size_t)blockIdx.x * E;
#pragma unroll
    for (int j = 0; j <= KW; ++j) {
        float s = acc[j];
        for (int q = 0; q < 3; ++q) s += red[q][c][j];
        if (j < KW) copy[c * KW + j] = s; else copy[cout * KW + c] = s;
    }
}

// dx[n][s] = sum over the five taps j = (s & 1) + 2 jj, in order, and the channels, in order, of w[c][j] dz[n][(s >> 1) - jj][c]
// as one fmaf chain from 0.0f.
__global__ __launch_bounds__(256) void zz_in_dgrad_kernel(const float* __restrict__ dout, const uint8_t* __restrict__ sel,
                                                          const float* __restrict__ w, float* __restrict__ dx, int total, int L, int Lp,
                                                          int cout, int cpad) {
    __shared__ float ws[KW][64];                                           // [tap][channel]
    for (int q = threadIdx.x; q < KW * 64; q += 256) {
        const int j = q >> 6, c = q & 63;
        ws[j][c] = c < cout ? w[c * KW + j] : 0.f;
    }
    __syncthreads();
    const int o = blockIdx.x * 256 + threadIdx.x;
    if (o >= total) return;
    const int n = o / L, s = o - n * L, parity = s & 1, u = s >> 1;
    float acc = 0.f;
    for (int jj = 0; jj < 5; ++jj) {
        const int t = u - jj;
        if (t < 0 || t >= 2 * Lp) continue;
        const uint32_t want = (uint32_t)(t & 1) + 1u;
        const size_t base = ((size_t)n * Lp + (t >> 1)) * cpad;
        const float* wj = ws[2 * jj + parity];
        for (int c = 0; c < cpad; c += 4) {
            const uint32_t s4 = *reinterpret_cast<const uint32_t*>(sel + base + c);
            if (s4 == 0) continue;
            const float4 d = *reinterpret_cast<const float4*>(dout + base + c);
            if ((s4 & 0xff) == want) acc = fmaf(wj[c], d.x, acc);
            if (((s4 >> 8) & 0xff) == want) acc = fmaf(wj[c + 1], d.y, acc);
            if (((s4 >> 16) & 0xff) == want) acc = fmaf(wj[c + 2], d.z, acc);
            if ((s4 >> 24) == want) acc = fmaf(wj[c + 3], d.w, acc);
        }
    }
    dx[o] = acc;
}

bool layer_ok(const Geometry& g, int32_t layer) { return layer >= 1 && layer < g.layers; }

// dOut of conv layer l as its readers see it
Grad grad_of(const Shape& s, int l, const float* dout) {
    const int64_t lp = s.len[l + 1];
    const int cp = s.g.cpad[l];
    if (l == s.g.layers - 1) return Grad{dout, cp, 0, (float)lp};
    return Grad{dout, lp * cp, cp, 1.f};
}

}  // namespace

extern "C" int stof_zonzini_train_pack(const stof_zonzini_desc* desc, const float* const* params, void* out, size_t out_bytes,
                                       void* stream) {
    Geometry g;
    if (!geometry(desc, g) || !params || !out) return STOF_ERR_BAD_ARG;
    const int np = 2 * g.layers + 4;
    for (int i = 0; i < np; ++i)
        if (!params[i]) return STOF_ERR_BAD_ARG;
    const Layout o = layout(g);
    if (out_bytes < (size_t)o.total * sizeof(float)) return STOF_ERR_WORKSPACE;
    float* const blob = static_cast<float*>(out);
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (hipMemsetAsync(blob, 0, (size_t)o.total * sizeof(float), s) != hipSuccess) return STOF_ERR_HIP;
    auto copy = [&](const float* src, int64_t at, int n) {
        hipLaunchKernelGGL(zz_copy_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, src, blob + at, n);
    };
    copy(params[0], o.c1w, g.cout[0] * KW);                    // [cout][1][10] is [c * 10 + j]; the pad rows stay 0
    copy(params[1], o.c1b, g.cout[0]);
    for (int l = 1; l < g.layers; ++l) {
        const int groups = KW * g.cpad[l - 1] / 8, total = ntiles(g.cout[l]) * groups * 256;
        pack_frag32_device(s, params[2 * l], g.cout[l], g.cout[l - 1], KW, g.cpad[l - 1], groups, blob + o.frag[l], total);
        copy(params[2 * l + 1], o.bias[l], g.cout[l]);
    }
    const int C = g.cout[g.layers - 1];
    hipLaunchKernelGGL(zz_pack_fc1t_kernel, dim3((unsigned)((C * FC1 + 255) / 256)), dim3(256), 0, s, params[2 * g.layers], C,
                       blob + o.fc1t);
    copy(params[2 * g.layers + 1], o.fc1b, FC1);
    copy(params[2 * g.layers + 2], o.fc2w, FC1);
    copy(params[2 * g.layers + 3], o.fc2b, 1);
    return launched();
}

extern "C" int stof_zonzini_train_forward(const stof_zonzini_desc* desc, const float* x, int64_t N, int64_t L, const void* packed,
                                          float* const* acts, uint8_t* const* sel, float* f, float* h, float* y, void* stream) {
    Shape sh;
    if (!x || !packed || !acts || !sel || !f || !h || !y) return STOF_ERR_BAD_ARG;
    const int rc = shape_of(desc, N, L, sh);
    if (rc != STOF_OK) return rc;
    const Geometry& g = sh.g;
    for (int l = 0; l < g.layers; ++l)
        if (!acts[l] || !sel[l]) return STOF_ERR_BAD_ARG;
    const Layout o = layout(g);
    const float* const blob = static_cast<const float*>(packed);
    hipStream_t s = static_cast<hipStream_t>(stream);
    {
        const int64_t lp = sh.len[1], cnt = N * lp * g.cpad[0];
        hipLaunchKernelGGL(zz_conv1_kernel<true>, dim3((unsigned)((cnt + 255) / 256)), dim3(256), 0, s, x, (long long)L, (long long)lp,
                           g.cout[0], g.cpad[0], blob + o.c1w, blob + o.c1b, acts[0], (long long)cnt, sel[0]);
        if (launched() != STOF_OK) return STOF_ERR_HIP;
    }
    for (int l = 1; l < g.layers; ++l) {
        const int64_t lin = sh.len[l], lp = sh.len[l + 1];
        const int64_t M = N * lp, mtiles = (M + 31) / 32;
        const int nt = ntiles(g.cout[l]);
        const dim3 grid((unsigned)((mtiles + 1) / 2), (unsigned)((nt + 1) / 2));
        hipLaunchKernelGGL(zz_conv_kernel<true>, grid, dim3(64 * CONV_WAVES), 0, s, acts[l - 1], (long long)lin, g.cpad[l - 1],
                           (long long)M, (long long)lp, g.cout[l], g.cpad[l], nt, reinterpret_cast<const float4*>(blob + o.frag[l]),
                           blob + o.bias[l], acts[l], sel[l]);
        if (launched() != STOF_OK) return STOF_ERR_HIP;
    }
    const int last = g.layers - 1;
    hipLaunchKernelGGL(zz_head_kernel<true>, dim3((unsigned)((N + HEAD_ROWS - 1) / HEAD_ROWS)), dim3(HEAD_THREADS), 0, s, acts[last],
                       (long long)N, (long long)sh.len[last + 1], g.cout[last], g.cpad[last], blob + o.fc1t, blob + o.fc1b,
                       blob + o.fc2w, blob + o.fc2b, y, f, h);
    return launched();
}

extern "C" int stof_zonzini_train_head_bwd(const stof_zonzini_desc* desc, const float* dy, const float* f, const float* h,
                                           const float* fc1w, const float* fc2w, float* dfc1w, float* dfc1b, float* dfc2w,
                                           float* dfc2b, float* df, int64_t N, void* stream) {
    Geometry g;
    if (!geometry(desc, g) || N <= 0 || !dy || !f || !h || !fc1w || !fc2w || !dfc1w || !dfc1b || !dfc2w || !dfc2b || !df)
        return STOF_ERR_BAD_ARG;
    if (N > (1ll << 20)) return STOF_ERR_UNSUPPORTED;
    const int C = g.cout[g.layers - 1], cpad = g.cpad[g.layers - 1];
    hipStream_t s = static_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(zz_head_units_kernel, dim3(FC1 / 256), dim3(256), 0, s, dy, h, fc2w, (int)N, dfc2w, dfc2b, dfc1b);
    if (launched() != STOF_OK) return STOF_ERR_HIP;
    hipLaunchKernelGGL(zz_head_w1_kernel, dim3((unsigned)((FC1 * C + 255) / 256)), dim3(256), 0, s, dy, h, fc2w, f, (int)N, C, dfc1w);
    if (launched() != STOF_OK) return STOF_ERR_HIP;
    hipLaunchKernelGGL(zz_head_df_kernel, dim3((unsigned)N), dim3(256), 0, s, dy, h, fc2w, fc1w, C, cpad, df);
    return launched();
}

extern "C" size_t stof_zonzini_train_conv_wgrad_workspace_bytes(const stof_zonzini_desc* desc, int32_t layer) {
    Geometry g;
    if (!geometry(desc, g) || !layer_ok(g, layer)) return 0;
    return (size_t)wgrad_max_copies(g, layer) * wgrad_e(g, layer) * sizeof(float);
}

extern "C" int stof_zonzini_train_conv_wgrad(const stof_zonzini_desc* desc, int32_t layer, const float* in, const float* dout,
                                             const uint8_t* sel, float* dw, float* db, int64_t N, int64_t L, void* workspace,
                                             size_t workspace_bytes, void* stream) {
    Shape sh;
    if (!in || !dout || !sel || !dw || !db || !workspace) return STOF_ERR_BAD_ARG;
    const int rc = shape_of(desc, N, L, sh);
    if (rc != STOF_OK) return rc;
    const Geometry& g = sh.g;
    if (!layer_ok(g, layer)) return STOF_ERR_BAD_ARG;
    if (workspace_bytes < stof_zonzini_train_conv_wgrad_workspace_bytes(desc, layer)) return STOF_ERR_WORKSPACE;
    const int l = layer, K = KW * g.cpad[l - 1], E = (int)wgrad_e(g, l);
    const int64_t lp = sh.len[l + 1], M = N * lp;
    const Chunks ch = balanced_chunks(M, ZW_CHUNK, wgrad_max_copies(g, l), 2);
    float* copies = static_cast<float*>(workspace);
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int ktiles = (K + 31) / 32;
    const dim3 grid((unsigned)ch.n, (unsigned)((ktiles + 3) / 4), (unsigned)ntiles(g.cout[l]));
    hipLaunchKernelGGL(zz_wgrad_kernel, grid, dim3(256), 0, s, in, (int)sh.len[l], g.cpad[l - 1], grad_of(sh, l, dout), sel, (int)M,
                       (int)lp, (int)ch.per, g.cout[l], g.cpad[l], K, copies, E);
    if (launched() != STOF_OK) return STOF_ERR_HIP;
    partial_reduce(s, copies, ch.n, E, E, ConvTapsThenBias{dw, db, g.cout[l], g.cout[l - 1], g.cpad[l - 1], K, KW}, 1.f);
    return launched();
}

extern "C" size_t stof_zonzini_train_dgrad_image_floats(const stof_zonzini_desc* desc, int32_t layer) {
    Geometry g;
    if (!geometry(desc, g) || !layer_ok(g, layer)) return 0;
    return (size_t)dgrad_image_floats(g, layer);
}

extern "C" int stof_zonzini_train_dgrad_image(const stof_zonzini_desc* desc, int32_t layer, const float* w, float* out, void* stream) {
    Geometry g;
    if (!geometry(desc, g) || !layer_ok(g, layer) || !w || !out) return STOF_ERR_BAD_ARG;
    const int total = (int)dgrad_image_floats(g, layer);
    hipLaunchKernelGGL(zz_dgrad_image_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, static_cast<hipStream_t>(stream), w,
                       g.cout[layer], g.cout[layer - 1], g.cpad[layer], ntiles(g.cpad[layer - 1]), dgrad_groups(g, layer), out, total);
    return launched();
}

extern "C" int stof_zonzini_train_conv_dgrad(const stof_zonzini_desc* desc, int32_t layer, const float* dout, const uint8_t* sel,
                                             const float* image, float* din, int64_t N, int64_t L, void* stream) {
    Shape sh;
    if (!dout || !sel || !image || !din) return STOF_ERR_BAD_ARG;
    const int rc = shape_of(desc, N, L, sh);
    if (rc != STOF_OK) return rc;
    const Geometry& g = sh.g;
    if (!layer_ok(g, layer)) return STOF_ERR_BAD_ARG;
    const int l = layer;
    const int64_t lin = sh.len[l], U = (lin + 1) / 2, Mrows = N * U, mtiles = (Mrows + 31) / 32;
    const int nt_in = ntiles(g.cpad[l - 1]);
    const dim3 grid((unsigned)((mtiles + 1) / 2), (unsigned)((nt_in + 1) / 2), 2);
    hipLaunchKernelGGL(zz_dgrad_kernel, grid, dim3(256), 0, static_cast<hipStream_t>(stream), grad_of(sh, l, dout), sel,
                       (int)sh.len[l + 1], g.cpad[l], (int)Mrows, (int)U, (int)lin, g.cpad[l - 1], nt_in, dgrad_groups(g, l),
                       reinterpret_cast<const float4*>(image), din);
    return launched();
}

extern "C" size_t stof_zonzini_train_in_wgrad_workspace_bytes(const stof_zonzini_desc* desc) {
    Geometry g;
    if (!geometry(desc, g)) return 0;
    return (size_t)ZW1_MAX_COPIES * g.cout[0] * (KW + 1) * sizeof(float);
}

extern "C" int stof_zonzini_train_in_wgrad(const stof_zonzini_desc* desc, const float* x, const float* dout, const uint8_t* sel,
                                           float* dw, float* db, int64_t N, int64_t L, void* workspace, size_t workspace_bytes,
                                           void* stream) {
    Shape sh;
    if (!x || !dout || !sel || !dw || !db || !workspace) return STOF_ERR_BAD_ARG;
    const int rc = shape_of(desc, N, L, sh);
    if (rc != STOF_OK) return rc;
    const Geometry& g = sh.g;
    if (workspace_bytes < stof_zonzini_train_in_wgrad_workspace_bytes(desc)) return STOF_ERR_WORKSPACE;
    const int64_t lp = sh.len[1], M = N * lp;
    const Chunks ch = balanced_chunks(M, ZW1_CHUNK, ZW1_MAX_COPIES, 2);
    const int E = g.cout[0] * (KW + 1);
    float* copies = static_cast<float*>(workspace);
    hipStream_t s = static_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(zz_in_wgrad_kernel, dim3((unsigned)ch.n), dim3(256), 0, s, x, (int)L, dout, sel, (int)M, (int)lp, (int)ch.per,
                       g.cout[0], g.cpad[0], copies, E);
    if (launched() != STOF_OK) return STOF_ERR_HIP;
    partial_reduce(s, copies, ch.n, E, E, DwThenDb{dw, db, g.cout[0] * KW}, 1.f);
    return launched();
}

extern "C" int stof_zonzini_train_in_dgrad(const stof_zonzini_desc* desc, const float* dout, const uint8_t* sel, const float* w,
                                           float* dx, int64_t N, int64_t L, void* stream) {
    Shape sh;
    if (!dout || !sel || !w || !dx) return STOF_ERR_BAD_ARG;
    const int rc = shape_of(desc, N, L, sh);
    if (rc != STOF_OK) return rc;
    const Geometry& g = sh.g;
    const int64_t total = N * L;
    hipLaunchKernelGGL(zz_in_dgrad_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, static_cast<hipStream_t>(stream), dout, sel,
                       w, dx, (int)total, (int)L, (int)sh.len[1], g.cout[0], g.cpad[0]);
    return launched();
}
