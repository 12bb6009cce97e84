// The SincNet baseline (models/sincnet.py of the reference: SincNet with the option dict of main.py:145-157) on gfx950,
// inference only, exact fp32.
//
//   x [N, 1, L] -> sinc band-pass conv 1 -> 128 (1023 taps, "same" zero padding 511/511) -> BN -> LeakyReLU(0.2)
//               -> Conv1d 128 -> 128 (k 11, pad 5/5) -> BN -> LeakyReLU(0.2)
//               -> Conv1d 128 -> 128 (k 9, pad 4/4)  -> BN -> LeakyReLU(0.2)
//               -> Conv1d 128 -> 1 (k 7, pad 3/3)    -> BN -> identity (LeakyReLU(1))        -> y [N, 1, L]
// BatchNorm runs in eval mode; each one (with the conv bias before it) is the per-channel affine acc * s + t that the
// packer precomputes in double.
//
// The kernels, the layout and the blob are in sincnet_net.h, shared with the training file (sincnet_train.hip); this file
// instantiates them with the inference epilogue (EPI_BN) and holds the host packer and the C entries.
//
// Activations between layers are channel-last fp32 with GAP zero rows around every waveform:
//   buffer row r = GAP + n (L + GAP) + t holds act[n][t][0 .. 128), rows GAP + n (L + GAP) - GAP .. - 1 are zero.
// The zero rows are the convolutions' padding, so the K span (tap, input channel) of output (n, t) is the contiguous
// run of rows t - P .. t + P of that layout, read straight into the A operand (as zz_conv_kernel in zonzini.hip does).
//
//   sn_gaps_kernel    zeroes the GAP rows of both ping-pong buffers (the workspace is not assumed to be clean)
//   sn_sinc_kernel    layer 0: implicit GEMM on v_mfma_f32_32x32x2_f32, M = time, N = 128 filters, K = 1024 taps (tap
//                     1023 is zero).  A work-group owns 128 samples of one row and stages x[t0 - 511 .. t0 + 639] in LDS
//                     with zeros outside [0, L); the A operand is the sliding window over that image.
//   sn_conv_kernel    layers 1 and 2: conv + bias + BN + LeakyReLU as one implicit GEMM, M = (row, t) flattened over the
//                     batch, N = 128, K = tap x 128 + input channel.  Each wave owns 32 outputs x all 128 channels (four
//                     32 x 32 accumulators share every A fragment); below NARROW_M outputs a wave owns one 32-channel
//                     tile, so that small batches still fill the GPU (the same k order: results are bitwise the same).
//   sn_out_kernel     layer 3 (128 -> 1, k 7, 0.2 % of the work) on the vector pipe: one wave per 16 samples of a row,
//                     lane l owns channels 2l, 2l + 1, a fixed xor-butterfly sums the lanes.
//
// Every output element is one fixed-order chain (MFMA k order, fixed loops and butterfly, no atomics), so a row's
// result does not depend on its batch, its chunk or its position there.  NaN propagates as in torch (conv sums, BN,
// LeakyReLU are all NaN-preserving).
#include "sincnet_net.h"

namespace {

// --------------------------------------------------------------------------------------------------------- packing
// The filter bank of SincConv_fast.forward (models/sincnet.py:147-188, min_low_hz = min_band_hz = 50), in double:
//   low = 50 + |low_hz_|, high = clamp(low + 50 + |band_hz_|, 50, fs / 2), band = high - low
//   n_j = 2 pi (j - 511) / fs, j = 0 .. 510; window_j = 0.54 - 0.46 cos(2 pi u_j / 1023), u = linspace(0, 510.5, 511)
//   left_j = (sin(high n_j) - sin(low n_j)) / (n_j / 2) window_j, centre 2 band, right = mirror of left; all / (2 band)
void sinc_bank(double fs, const float* low_hz, const float* band_hz, double* bank /* [C][K0] */) {
    const double pi = 3.14159265358979323846;
    double win[HALF0], nn[HALF0];
    for (int j = 0; j < HALF0; ++j) {
        const double u = (double)j * (K0 / 2.0 - 1.0) / (HALF0 - 1);
        win[j] = 0.54 - 0.46 * cos(2.0 * pi * u / K0);
        nn[j] = 2.0 * pi * (double)(j - HALF0) / fs;
    }
    for (int c = 0; c < C; ++c) {
        const double low = 50.0 + fabs((double)low_hz[c]);
        const double high = fmin(fmax(low + 50.0 + fabs((double)band_hz[c]), 50.0), fs / 2.0);
        const double band = high - low;
        double* f = bank + (int64_t)c * K0;
        for (int j = 0; j < HALF0; ++j) {
            const double v = (sin(high * nn[j]) - sin(low * nn[j])) / (nn[j] / 2.0) * win[j] / (2.0 * band);
            f[j] = v;
            f[K0 - 1 - j] = v;
        }
        f[HALF0] = 2.0 * band / (2.0 * band);
    }
}

// BN (eval) after a conv with bias `bias` (NULL: none): y = (acc + bias - mean) / sqrt(var + eps) * gamma + beta
void bn_affine(const float* const* bn, const float* bias, int c, double eps, float* s, float* t) {
    const double sc = (double)bn[0][c] / sqrt((double)bn[3][c] + eps);
    *s = (float)sc;
    *t = (float)(((bias ? (double)bias[c] : 0.0) - (double)bn[2][c]) * sc + (double)bn[1][c]);
}

}  // namespace

extern "C" size_t stof_sincnet_packed_bytes(const stof_sincnet_desc* desc) {
    if (!desc_ok(desc)) return 0;
    return (size_t)layout().total * sizeof(float);
}

extern "C" int stof_sincnet_filter_bank(const stof_sincnet_desc* desc, const float* low_hz, const float* band_hz, float* bank) {
    if (!desc_ok(desc) || !low_hz || !band_hz || !bank) return STOF_ERR_BAD_ARG;
    double* d = static_cast<double*>(malloc(sizeof(double) * C * K0));
    if (!d) return STOF_ERR_WORKSPACE;
    sinc_bank(desc->fs, low_hz, band_hz, d);
    for (int64_t i = 0; i < (int64_t)C * K0; ++i) bank[i] = (float)d[i];
    free(d);
    return STOF_OK;
}

extern "C" int stof_sincnet_band_grad(const stof_sincnet_desc* desc, const float* low_hz, const float* band_hz, const float* bank_grad,
                                      double* dlow_hz, double* dband_hz) {
    if (!desc_ok(desc) || !low_hz || !band_hz || !bank_grad || !dlow_hz || !dband_hz) return STOF_ERR_BAD_ARG;
    for (int c = 0; c < C; ++c) {
        const SincBand b = sinc_band(desc->fs, low_hz[c], band_hz[c]);
        double dh = 0.0, dl = 0.0;
        sinc_band_grad_taps(desc->fs, b, bank_grad + (int64_t)c * K0, 0, 1, &dh, &dl);
        sinc_band_grad_finish(b, low_hz[c], band_hz[c], dh, dl, dlow_hz + c, dband_hz + c);
    }
    return STOF_OK;
}

extern "C" int stof_sincnet_pack_weights(const stof_sincnet_desc* desc, const float* const* params, void* out, size_t out_bytes) {
    if (!desc_ok(desc) || !params || !out) return STOF_ERR_BAD_ARG;
    for (int i = 0; i < NUM_PARAMS; ++i)
        if (!params[i]) return STOF_ERR_BAD_ARG;
    const Layout o = layout();
    if (out_bytes < (size_t)o.total * sizeof(float)) return STOF_ERR_WORKSPACE;
    float* const blob = static_cast<float*>(out);
    memset(blob, 0, (size_t)o.total * sizeof(float));
    // layer 0: bank [C][1][1023] -> k = tap, the last tap of the 1024 zero
    {
        float* bank = static_cast<float*>(malloc(sizeof(float) * C * K0));
        if (!bank) return STOF_ERR_WORKSPACE;
        stof_sincnet_filter_bank(desc, params[0], params[1], bank);
        pack_frag32(bank, C, 1, K0, 1, C / 32, K0P / 8, blob + o.frag0);
        free(bank);
    }
    // layers 1, 2: weight [C][C][K] -> k = tap * C + ci
    pack_frag32(params[2], C, C, K1, C, C / 32, K1 * C / 8, blob + o.frag1);
    pack_frag32(params[4], C, C, K2, C, C / 32, K2 * C / 8, blob + o.frag2);
    // layer 3: weight [1][C][7] -> w3[tap][ci]
    for (int ci = 0; ci < C; ++ci)
        for (int j = 0; j < K3; ++j) blob[o.w3 + j * C + ci] = params[6][ci * K3 + j];
    // BN affines: params 8 + 4 i .. 11 + 4 i = bn.i weight, bias, running_mean, running_var
    const int64_t st_at[3] = {o.st0, o.st1, o.st2};
    for (int l = 0; l < 3; ++l)
        for (int c = 0; c < C; ++c)
            bn_affine(params + 8 + 4 * l, l == 0 ? nullptr : params[3 + 2 * (l - 1)], c, desc->bn_eps, blob + st_at[l] + c,
                      blob + st_at[l] + C + c);
    bn_affine(params + 20, params[7], 0, desc->bn_eps, blob + o.st3, blob + o.st3 + 1);
    return STOF_OK;
}

extern "C" size_t stof_sincnet_workspace_bytes(const stof_sincnet_desc* desc, int64_t N, int64_t L) {
    if (!desc_ok(desc) || N <= 0 || L <= 0) return 0;
    return 2 * (size_t)buffer_floats(N, L) * sizeof(float);
}

extern "C" int stof_sincnet_forward(const stof_sincnet_desc* desc, const float* x, int64_t N, int64_t L, const void* packed,
                                    float* y, void* workspace, size_t workspace_bytes, void* stream) {
    if (!desc_ok(desc) || !x || !packed || !workspace || N <= 0 || L <= 0) return STOF_ERR_BAD_ARG;
    if (desc->stop_after < 0 || desc->stop_after > 3 || (!y && desc->stop_after == 0)) return STOF_ERR_BAD_ARG;
    if (N * L >= (1ll << 31) - 64 || N * (L + GAP) + GAP >= (1ll << 31) - 64) return STOF_ERR_UNSUPPORTED;   // 32-bit m
    const int64_t bf = buffer_floats(N, L);
    if (workspace_bytes < 2 * (size_t)bf * sizeof(float)) return STOF_ERR_WORKSPACE;
    const Layout o = layout();
    const float* const blob = static_cast<const float*>(packed);
    float* const buf[2] = {static_cast<float*>(workspace), static_cast<float*>(workspace) + bf};
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int layers = desc->stop_after == 0 ? 4 : desc->stop_after;

    const int64_t gaps = (N + 1) * GAP * C;
    hipLaunchKernelGGL(sn_gaps_kernel, dim3((unsigned)((gaps + 255) / 256)), dim3(256), 0, s, buf[0], buf[1], (long long)L,
                       (long long)gaps);
    if (hipGetLastError() != hipSuccess) return STOF_ERR_HIP;
    // Small batches: one N tile per wave (4x the waves, each A fragment loaded 4x) so that the GPU fills up.
    const bool narrow = N * L < NARROW_M;
    const int64_t tb0 = (L + TILE0 - 1) / TILE0;
    const dim3 sgrid((unsigned)(N * tb0), narrow ? 4 : 1);
    if (narrow)
        hipLaunchKernelGGL((sn_sinc_kernel<1, EPI_BN>), sgrid, dim3(256), 0, s, x, (long long)L, (long long)tb0,
                           reinterpret_cast<const float4*>(blob + o.frag0), blob + o.st0, buf[0]);
    else
        hipLaunchKernelGGL((sn_sinc_kernel<4, EPI_BN>), sgrid, dim3(256), 0, s, x, (long long)L, (long long)tb0,
                           reinterpret_cast<const float4*>(blob + o.frag0), blob + o.st0, buf[0]);
    if (hipGetLastError() != hipSuccess) return STOF_ERR_HIP;
    if (layers == 1) return STOF_OK;
    const unsigned M = (unsigned)(N * L);
    const dim3 cgrid((unsigned)((M + 127) / 128), narrow ? 4 : 1);
    for (int l = 1; l <= 2; ++l) {
        const float* in = buf[(l - 1) & 1];
        const float4* fr = reinterpret_cast<const float4*>(blob + (l == 1 ? o.frag1 : o.frag2));
        const float* st = blob + (l == 1 ? o.st1 : o.st2);
        float* out = buf[l & 1];
        if (l == 1 && narrow) hipLaunchKernelGGL((sn_conv_kernel<K1, 1, EPI_BN>), cgrid, dim3(256), 0, s, in, M, (unsigned)L, fr, st, out);
        if (l == 1 && !narrow) hipLaunchKernelGGL((sn_conv_kernel<K1, 4, EPI_BN>), cgrid, dim3(256), 0, s, in, M, (unsigned)L, fr, st, out);
        if (l == 2 && narrow) hipLaunchKernelGGL((sn_conv_kernel<K2, 1, EPI_BN>), cgrid, dim3(256), 0, s, in, M, (unsigned)L, fr, st, out);
        if (l == 2 && !narrow) hipLaunchKernelGGL((sn_conv_kernel<K2, 4, EPI_BN>), cgrid, dim3(256), 0, s, in, M, (unsigned)L, fr, st, out);
        if (hipGetLastError() != hipSuccess) return STOF_ERR_HIP;
        if (layers == l + 1) return STOF_OK;
    }
    const int64_t tblocks = (L + OUT_T - 1) / OUT_T, waves = N * tblocks;
    hipLaunchKernelGGL(sn_out_kernel<EPI_BN>, dim3((unsigned)((waves + 3) / 4)), dim3(256), 0, s, buf[0], (long long)N, (long long)L,
                       (long long)tblocks, blob + o.w3, blob + o.st3, y);
    return hipGetLastError() == hipSuccess ? STOF_OK : STOF_ERR_HIP;
}
