// The Kuleshov baseline (models/kuleshov.py of the reference with num_layers = 4; selected by main.py:137-138) on gfx950,
// inference only, exact fp32.  Eval mode: Dropout is the identity, BatchNorm uses its running statistics.
//
//   x [N, 1, >= L] -> x[:, :, :L]
//     down i = 0..3   Conv1d(Cin, nf, fs, stride 2), nf = 128, 256, 512, 512, fs = 65, 33, 17, 9
//                     -> lrelu0.2(BN(lrelu0.01(conv + b)))                                   lengths D0 .. D3
//     bottleneck      Conv1d(512, 512, 9, stride 2) -> lrelu0.2                              length B
//     up i = 0..3     Conv1d(Cin, 2 nf, fs) -> BN, (Cin, 2 nf, fs) = (512, 1024, 9), (512, 1024, 17), (512, 512, 33),
//                     (256, 256, 65); pixel shuffle out[ch >> 1][2 p + (ch & 1)] = in[ch][p]; concatenation ALONG THE
//                     LENGTH with down output 3 - i appended behind                          lengths Lc0 .. Lc3
//     final_conv      Conv1d(128, 2, 9)                                                      length F = Lc3 - 8
//     flat[2 pos + ch] -> Linear(2 F, O) -> y [N, 1, O]
//
// Activations are channel-last fp32.  The four concatenation buffers cat_i [N][Lc_i][C_i] hold the shuffled up output
// in rows 0 .. 2 U_i - 1 and the skip in rows 2 U_i .. Lc_i - 1: the down block writes its output there in the first
// place, the up convolution's epilogue stores at the shuffled address, and the next convolution reads the whole row
// range.  A convolution's K span (tap, input channel) of output t is the contiguous run of rows stride t .. + fs - 1,
// read straight into the A operand; the input of the Linear layer is final_conv's output as it lies in memory.
//
//   ks_down0_kernel  down_conv0 (1 -> 128, k 65, stride 2; 0.06 % of the work) on the vector pipe: one thread per
//                    (channel, half of 64 outputs), the 65 taps in registers, the input window in LDS.
//   ks_conv_kernel   the nine 128 .. 1024-wide convolutions as one implicit GEMM on v_mfma_f32_32x32x2_f32: M = (row, t)
//                    flattened over the batch, N = output channels, K = tap x Cin + ci.  A wave owns MT x 32 outputs x
//                    NTW x 32 channels; (MT, NTW) = (2, 4), (1, 4) or (1, 1) by the number of waves the layer gives, so
//                    that a short layer (up_conv0: 43 positions per row) still fills the GPU.  Every variant runs the
//                    same k order, so results are bitwise the same.  The epilogue is chosen per layer.
//   ks_final_kernel  final_conv (128 -> 2, k 9; 0.06 %) on the vector pipe: one wave per 16 positions, lane l owns
//                    channels 2 l, 2 l + 1, a fixed xor-butterfly sums the lanes.  Writes flat [N][Kp] (Kp = 2 F rounded
//                    up to 8, the tail zeroed).
//   ks_fc_kernel     output_fc: M = rows, N = O, K = Kp on the same MFMA.  A work-group owns one 32-output tile and up to
//                    128 rows, so the weight (636 MB at L = 2000, O = 20000) is streamed once per 128 rows; its four
//                    waves take K groups q = w, w + 4, .. and are summed in the fixed order ((w0 + w1) + w2) + w3.
//
// Every output element is one fixed-order chain (no atomics; the only split sum has a fixed order that does not depend
// on the shape), so a row's result does not depend on its batch, its chunk or its position there.  NaN propagates as in
// torch (convolution sums, BN and both leaky ReLUs are NaN-preserving).
#include "kuleshov_net.h"

namespace {

// Packed blob (floats, every section starts on a 256-byte boundary):
//   w0 [65][128] (w0[tap][c]), ep0 [3][128]
//   down 1..3, bottleneck, up 0..3:  frag [Cout / 32][fs Cin / 8][64 lanes][4], ep [3][Cout]
//   wf [2][9][128] (wf[oc][tap][ci]), bf [2]
//   fcfrag [OT][G][64][4] (rows >= O and columns >= 2 F are zero), fcb [O]
// ep = (b, s, t): down  lrelu0.2(s lrelu0.01(acc + b) + t)      s = gamma / sqrt(var + eps), t = beta - mean s
//                 bott  lrelu0.2(acc + b)                        (s = 1, t = 0, unused)
//                 up    s acc + t                                t = (bias - mean) s + beta  (b = 0, unused)
// Fragment lane l, element e of K group q holds W[32 tile + (l & 31)][k = 8 q + 4 (l >> 5) + e]; the A operand of lane
// l reads the activation at the same k with one float4.
struct Layout {
    int64_t w0, ep0, dfrag[NL], dep[NL], bfrag, bep, ufrag[NL], uep[NL], wf, bf, fcfrag, fcb, total;
};

Layout layout(const Dims& d) {
    Layout o{};
    int64_t at = 0;
    o.w0 = at; at = align_up(at + FS[0] * C0);
    o.ep0 = at; at = align_up(at + 3 * C0);
    for (int i = 1; i < NL; ++i) {
        o.dfrag[i] = at; at = align_up(at + (int64_t)NF[i] * NF[i - 1] * FS[i]);
        o.dep[i] = at; at = align_up(at + 3 * NF[i]);
    }
    o.bfrag = at; at = align_up(at + (int64_t)512 * 512 * KB);
    o.bep = at; at = align_up(at + 3 * 512);
    for (int i = 0; i < NL; ++i) {
        o.ufrag[i] = at; at = align_up(at + (int64_t)UP_COUT[i] * UP_CIN[i] * UP_FS[i]);
        o.uep[i] = at; at = align_up(at + 3 * UP_COUT[i]);
    }
    o.wf = at; at = align_up(at + 2 * KB * C0);
    o.bf = at; at = align_up(at + 2);
    o.fcfrag = at; at = align_up(at + d.OT * d.G * 256);
    o.fcb = at; at = align_up(at + d.O);
    o.total = at;
    return o;
}

// Workspace (floats): cat3 [N][Lc3][128], cat2 [N][Lc2][256], cat1 [N][Lc1][512], cat0 [N][Lc0][512], bott [N][B][512],
// flat [N][Kp]
struct Work {
    int64_t cat[NL], bott, flat, total;
};

Work work(const Dims& d, int64_t N) {
    Work o{};
    int64_t at = 0;
    for (int i = 0; i < NL; ++i) {
        o.cat[i] = at; at = align_up(at + N * d.Lc[i] * (UP_COUT[i] / 2));
    }
    o.bott = at; at = align_up(at + N * d.B * 512);
    o.flat = at; at = align_up(at + N * d.Kp);
    o.total = at;
    return o;
}

// ---------------------------------------------------------------------------------------------------------- down 0
// Work-group (row n, outputs t0 .. t0 + 63): thread (c = tid & 127, half = tid >> 7) owns channel c of outputs
// t0 + 32 half .. + 31.  xs[j] = x[n][2 t0 + j] (0 past the cropped length L).
__global__ __launch_bounds__(256) void ks_down0_kernel(const float* __restrict__ x, long long xstride, int L, int D0,
                                                       int tblocks, const float* __restrict__ w0,
                                                       const float* __restrict__ ep, float* __restrict__ out,
                                                       long long out_n_stride) {
    __shared__ float xs[XS0];
    const int n = blockIdx.x / tblocks, t0 = (blockIdx.x % tblocks) * T0;
    const float* xr = x + (long long)n * xstride;
    for (int j = threadIdx.x; j < XS0; j += 256) {
        const int t = 2 * t0 + j;
        xs[j] = t < L ? xr[t] : 0.f;
    }
    __syncthreads();
    const int c = threadIdx.x & 127, half = threadIdx.x >> 7;
    float w[FS0];
#pragma unroll
    for (int j = 0; j < FS0; ++j) w[j] = w0[j * C0 + c];
    const float b = ep[c], s = ep[C0 + c], t = ep[2 * C0 + c];
    float* const o = out + (long long)n * out_n_stride + c;
    for (int u = 32 * half; u < 32 * half + 32; ++u) {
        if (t0 + u >= D0) break;
        float acc = 0.f;
#pragma unroll
        for (int j = 0; j < FS0; ++j) acc = fmaf(w[j], xs[2 * u + j], acc);
        o[(long long)(t0 + u) * C0] = leaky(fmaf(leaky(acc + b, 0.01f), s, t), 0.2f);
    }
}

// --------------------------------------------------------------------------------------------------------- packing
// bn = {weight, bias, running_mean, running_var}
void bn_down(const float* const* bn, const float* bias, int C, double eps, float* ep) {
    for (int c = 0; c < C; ++c) {
        const double s = (double)bn[0][c] / sqrt((double)bn[3][c] + eps);
        ep[c] = bias[c];
        ep[C + c] = (float)s;
        ep[2 * C + c] = (float)((double)bn[1][c] - (double)bn[2][c] * s);
    }
}

void bn_up(const float* const* bn, const float* bias, int C, double eps, float* ep) {
    for (int c = 0; c < C; ++c) {
        const double s = (double)bn[0][c] / sqrt((double)bn[3][c] + eps);
        ep[c] = 0.f;
        ep[C + c] = (float)s;
        ep[2 * C + c] = (float)(((double)bias[c] - (double)bn[2][c]) * s + (double)bn[1][c]);
    }
}

}  // namespace

extern "C" size_t stof_kuleshov_packed_bytes(const stof_kuleshov_desc* desc) {
    Dims d;
    if (!dims(desc, &d)) return 0;
    return (size_t)layout(d).total * sizeof(float);
}

extern "C" int stof_kuleshov_pack_weights(const stof_kuleshov_desc* desc, const float* const* params, void* out,
                                          size_t out_bytes) {
    Dims d;
    if (!dims(desc, &d) || !params || !out) return STOF_ERR_BAD_ARG;
    for (int i = 0; i < NUM_PARAMS; ++i)
        if (!params[i]) return STOF_ERR_BAD_ARG;
    const Layout o = layout(d);
    if (out_bytes < (size_t)o.total * sizeof(float)) return STOF_ERR_WORKSPACE;
    float* const blob = static_cast<float*>(out);
    memset(blob, 0, (size_t)o.total * sizeof(float));
    const double eps = desc->bn_eps;
    // down 0: weight [128][1][65] -> w0[tap][c]
    for (int c = 0; c < C0; ++c)
        for (int j = 0; j < FS[0]; ++j) blob[o.w0 + j * C0 + c] = params[0][c * FS[0] + j];
    bn_down(params + 2, params[1], C0, eps, blob + o.ep0);
    for (int i = 1; i < NL; ++i) {
        pack_frag32(params[6 * i], NF[i], NF[i - 1], FS[i], NF[i - 1], NF[i] / 32, FS[i] * NF[i - 1] / 8, blob + o.dfrag[i]);
        bn_down(params + 6 * i + 2, params[6 * i + 1], NF[i], eps, blob + o.dep[i]);
    }
    pack_frag32(params[24], 512, 512, KB, 512, 512 / 32, KB * 512 / 8, blob + o.bfrag);
    for (int c = 0; c < 512; ++c) {
        blob[o.bep + c] = params[25][c];
        blob[o.bep + 512 + c] = 1.f;
    }
    for (int i = 0; i < NL; ++i) {
        pack_frag32(params[26 + 6 * i], UP_COUT[i], UP_CIN[i], UP_FS[i], UP_CIN[i], UP_COUT[i] / 32, UP_FS[i] * UP_CIN[i] / 8,
                    blob + o.ufrag[i]);
        bn_up(params + 26 + 6 * i + 2, params[26 + 6 * i + 1], UP_COUT[i], eps, blob + o.uep[i]);
    }
    // final_conv: weight [2][128][9] -> wf[oc][tap][ci]
    for (int oc = 0; oc < 2; ++oc)
        for (int ci = 0; ci < C0; ++ci)
            for (int j = 0; j < KB; ++j) blob[o.wf + (oc * KB + j) * C0 + ci] = params[50][(oc * C0 + ci) * KB + j];
    blob[o.bf] = params[51][0];
    blob[o.bf + 1] = params[51][1];
    // output_fc: weight [O][2 F] -> fragments, zero where o >= O or k >= 2 F
    pack_frag32(params[52], d.O, 1, 2 * d.F, 1, d.OT, d.G, blob + o.fcfrag);
    memcpy(blob + o.fcb, params[53], sizeof(float) * (size_t)d.O);
    return STOF_OK;
}

extern "C" size_t stof_kuleshov_workspace_bytes(const stof_kuleshov_desc* desc, int64_t N) {
    Dims d;
    if (!dims(desc, &d) || N <= 0) return 0;
    return (size_t)work(d, N).total * sizeof(float);
}

extern "C" int stof_kuleshov_forward(const stof_kuleshov_desc* desc, const float* x, int64_t N, int64_t x_row_stride,
                                     const void* packed, float* y, float* bottleneck, float* final_in, float* final_out,
                                     void* workspace, size_t workspace_bytes, void* stream) {
    Dims d;
    if (!dims(desc, &d) || N < 0 || x_row_stride < d.L) return STOF_ERR_BAD_ARG;
    if (N == 0) return STOF_OK;
    if (!x || !packed || !y || !workspace) return STOF_ERR_BAD_ARG;
    if (N * d.Lc[NL - 1] >= (1ll << 31) - 256 || N * d.OT >= (1ll << 26)) return STOF_ERR_UNSUPPORTED;   // 32-bit m
    const Work wk = work(d, N);
    if (workspace_bytes < (size_t)wk.total * sizeof(float)) return STOF_ERR_WORKSPACE;
    const Layout o = layout(d);
    const float* const blob = static_cast<const float*>(packed);
    float* const ws = static_cast<float*>(workspace);
    hipStream_t s = static_cast<hipStream_t>(stream);
    // cat[i] is the concatenation that up i writes: width UP_COUT[i] / 2, skip = down 3 - i behind 2 U[i] rows
    float* cat[NL];
    long long cat_stride[NL];
    float* skip[NL];                         // skip[j]: where down j writes
    for (int i = 0; i < NL; ++i) {
        cat[i] = ws + wk.cat[i];
        cat_stride[i] = d.Lc[i] * (UP_COUT[i] / 2);
        skip[NL - 1 - i] = cat[i] + 2 * d.U[i] * (UP_COUT[i] / 2);
    }
    float* const bott = ws + wk.bott;
    float* const flat = ws + wk.flat;

    const int tb0 = (int)((d.D[0] + T0 - 1) / T0);
    if (!launch(ks_down0_kernel, dim3((unsigned)(N * tb0)), s, x, (long long)x_row_stride, (int)d.L, (int)d.D[0], tb0,
                blob + o.w0, blob + o.ep0, skip[0], cat_stride[NL - 1]))
        return STOF_ERR_HIP;
    for (int i = 1; i < NL; ++i) {
        ConvArgs p{};
        p.in = skip[i - 1]; p.in_n_stride = cat_stride[NL - i];
        p.out = skip[i]; p.out_n_stride = cat_stride[NL - 1 - i];
        p.frag = reinterpret_cast<const float4*>(blob + o.dfrag[i]); p.ep = blob + o.dep[i];
        p.M = (unsigned)(N * d.D[i]); p.Lout = (unsigned)d.D[i];
        p.Cin = NF[i - 1]; p.Cout = NF[i]; p.stride = 2; p.G = FS[i] * NF[i - 1] / 8; p.mode = EP_DOWN;
        if (!launch_conv(p, desc->tile_variant, s)) return STOF_ERR_HIP;
    }
    {
        ConvArgs p{};
        p.in = skip[NL - 1]; p.in_n_stride = cat_stride[0];
        p.out = bott; p.out_n_stride = d.B * 512; p.out2 = bottleneck;
        p.frag = reinterpret_cast<const float4*>(blob + o.bfrag); p.ep = blob + o.bep;
        p.M = (unsigned)(N * d.B); p.Lout = (unsigned)d.B;
        p.Cin = 512; p.Cout = 512; p.stride = 2; p.G = KB * 512 / 8; p.mode = EP_BOTT;
        if (!launch_conv(p, desc->tile_variant, s)) return STOF_ERR_HIP;
    }
    for (int i = 0; i < NL; ++i) {
        ConvArgs p{};
        p.in = i == 0 ? bott : cat[i - 1]; p.in_n_stride = i == 0 ? d.B * 512 : cat_stride[i - 1];
        p.out = cat[i]; p.out_n_stride = cat_stride[i];
        p.frag = reinterpret_cast<const float4*>(blob + o.ufrag[i]); p.ep = blob + o.uep[i];
        p.M = (unsigned)(N * d.U[i]); p.Lout = (unsigned)d.U[i];
        p.Cin = UP_CIN[i]; p.Cout = UP_COUT[i]; p.stride = 1; p.G = UP_FS[i] * UP_CIN[i] / 8; p.mode = EP_UP;
        if (!launch_conv(p, desc->tile_variant, s)) return STOF_ERR_HIP;
    }
    if (final_in &&
        hipMemcpyAsync(final_in, cat[NL - 1], sizeof(float) * (size_t)(N * cat_stride[NL - 1]), hipMemcpyDeviceToDevice, s) != hipSuccess)
        return STOF_ERR_HIP;
    const int tbf = (int)((d.Kp / 2 + FIN_T - 1) / FIN_T);
    if (!launch(ks_final_kernel, dim3((unsigned)((N * tbf + 3) / 4)), s, (const float*)cat[NL - 1], (long long)N,
                (int)d.Lc[NL - 1], (int)d.F, (int)d.Kp, tbf, blob + o.wf, blob + o.bf, flat, final_out))
        return STOF_ERR_HIP;
    const float4* const fcfrag = reinterpret_cast<const float4*>(blob + o.fcfrag);
    if (N <= 32) {
        if (!launch(ks_fc_kernel<1, 8>, dim3((unsigned)d.OT), s, (const float*)flat, (int)d.Kp, (unsigned)N, 1, fcfrag, (int)d.G,
                    blob + o.fcb, (int)d.O, y))
            return STOF_ERR_HIP;
    } else {
        const int mg = (int)((N + 32 * FC_MT - 1) / (32 * FC_MT));
        if (!launch(ks_fc_kernel<FC_MT, 2>, dim3((unsigned)(d.OT * mg)), s, (const float*)flat, (int)d.Kp, (unsigned)N, mg, fcfrag,
                    (int)d.G, blob + o.fcb, (int)d.O, y))
            return STOF_ERR_HIP;
    }
    return STOF_OK;
}
