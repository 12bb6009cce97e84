// The Zonzini baselines (models/zonzini.py of the reference: ZonziniNetSmall / ZonziniNetLarge) on gfx950, inference: the
// host side (packer, workspace, launch chain) of the kernels of zonzini_net.h, instantiated without the training outputs.
#include <hip/hip_runtime.h>
#include <math.h>
#include <string.h>
#include "zonzini_net.h"

namespace {

// Workspace: two ping-pong buffers; buffer (i & 1) holds the output of conv layer i for all N rows.
void workspace_split(const Geometry& g, int64_t N, int64_t L, int64_t& off1, int64_t& total) {
    int64_t len = L, need[2] = {0, 0};
    for (int i = 0; i < g.layers; ++i) {
        len = pooled_len(len);
        const int64_t f = align_up(N * len * g.cpad[i]);
        need[i & 1] = need[i & 1] > f ? need[i & 1] : f;
    }
    off1 = need[0];
    total = need[0] + need[1];
}

}  // namespace

extern "C" size_t stof_zonzini_packed_bytes(const stof_zonzini_desc* desc) {
    Geometry g;
    if (!geometry(desc, g)) return 0;
    return (size_t)layout(g).total * sizeof(float);
}

extern "C" int stof_zonzini_pack_weights(const stof_zonzini_desc* desc, const float* const* params, void* out, size_t out_bytes) {
    Geometry g;
    if (!geometry(desc, g) || !params || !out) return STOF_ERR_BAD_ARG;
    const int np = 2 * g.layers + 4;
    for (int i = 0; i < np; ++i)
        if (!params[i]) return STOF_ERR_BAD_ARG;
    const Layout o = layout(g);
    if (out_bytes < (size_t)o.total * sizeof(float)) return STOF_ERR_WORKSPACE;
    float* const blob = static_cast<float*>(out);
    memset(blob, 0, (size_t)o.total * sizeof(float));
    // conv1: weight [cout][1][10]
    for (int c = 0; c < g.cout[0]; ++c) {
        for (int j = 0; j < KW; ++j) blob[o.c1w + c * KW + j] = params[0][c * KW + j];
        blob[o.c1b + c] = params[1][c];
    }
    for (int l = 1; l < g.layers; ++l) {                       // weight [cout][cin][10]
        const float* w = params[2 * l];
        const int cin = g.cout[l - 1], cp = g.cpad[l - 1], co = g.cout[l];
        pack_frag32(w, co, cin, KW, cp, ntiles(co), (int64_t)KW * cp / 8, blob + o.frag[l]);
        for (int c = 0; c < co; ++c) blob[o.bias[l] + c] = params[2 * l + 1][c];
    }
    const int C = g.cout[g.layers - 1];
    const float *w1 = params[2 * g.layers], *b1 = params[2 * g.layers + 1], *w2 = params[2 * g.layers + 2],
                *b2 = params[2 * g.layers + 3];
    for (int j = 0; j < FC1; ++j) {
        for (int c = 0; c < C; ++c) blob[o.fc1t + (int64_t)c * FC1 + j] = w1[(int64_t)j * C + c];
        blob[o.fc1b + j] = b1[j];
        blob[o.fc2w + j] = w2[j];
    }
    blob[o.fc2b] = b2[0];
    return STOF_OK;
}

extern "C" size_t stof_zonzini_workspace_bytes(const stof_zonzini_desc* desc, int64_t N, int64_t L) {
    Geometry g;
    if (!geometry(desc, g) || N <= 0 || L < g.min_len) return 0;
    int64_t off1, total;
    workspace_split(g, N, L, off1, total);
    return (size_t)total * sizeof(float);
}

extern "C" int stof_zonzini_forward(const stof_zonzini_desc* desc, const float* x, int64_t N, int64_t L, const void* packed,
                                    float* y, float* features, void* workspace, size_t workspace_bytes, void* stream) {
    Geometry g;
    if (!geometry(desc, g) || !x || !packed || !y || !workspace || N <= 0) return STOF_ERR_BAD_ARG;
    if (L < g.min_len) return STOF_ERR_POOL_EMPTY;              // the reference's max_pool1d (or conv) raises
    if (L > (1ll << 30) || N > (1ll << 30)) return STOF_ERR_UNSUPPORTED;
    int64_t off1, total;
    workspace_split(g, N, L, off1, total);
    if (workspace_bytes < (size_t)total * sizeof(float)) return STOF_ERR_WORKSPACE;
    const Layout o = layout(g);
    const float* const blob = static_cast<const float*>(packed);
    float* const buf[2] = {static_cast<float*>(workspace), static_cast<float*>(workspace) + off1};
    hipStream_t s = static_cast<hipStream_t>(stream);

    int64_t lin = L, lp = pooled_len(L);
    {
        const int64_t cnt = N * lp * g.cpad[0];
        hipLaunchKernelGGL(zz_conv1_kernel<false>, dim3((unsigned)((cnt + 255) / 256)), dim3(256), 0, s, x, (long long)L, (long long)lp,
                           g.cout[0], g.cpad[0], blob + o.c1w, blob + o.c1b, buf[0], (long long)cnt, (uint8_t*)nullptr);
        if (hipGetLastError() != hipSuccess) return STOF_ERR_HIP;
    }
    for (int l = 1; l < g.layers; ++l) {
        lin = lp;
        lp = pooled_len(lin);
        const int64_t M = N * lp, mtiles = (M + 31) / 32;
        const int nt = ntiles(g.cout[l]);
        const dim3 grid((unsigned)((mtiles + 1) / 2), (unsigned)((nt + 1) / 2));
        hipLaunchKernelGGL(zz_conv_kernel<false>, grid, dim3(64 * CONV_WAVES), 0, s, buf[(l - 1) & 1], (long long)lin, g.cpad[l - 1],
                           (long long)M, (long long)lp, g.cout[l], g.cpad[l], nt,
                           reinterpret_cast<const float4*>(blob + o.frag[l]), blob + o.bias[l], buf[l & 1], (uint8_t*)nullptr);
        if (hipGetLastError() != hipSuccess) return STOF_ERR_HIP;
    }
    const int last = g.layers - 1;
    hipLaunchKernelGGL(zz_head_kernel<false>, dim3((unsigned)((N + HEAD_ROWS - 1) / HEAD_ROWS)), dim3(HEAD_THREADS), 0, s, buf[last & 1],
                       (long long)N, (long long)lp, g.cout[last], g.cpad[last], blob + o.fc1t, blob + o.fc1b, blob + o.fc2w,
                       blob + o.fc2b, y, features, (float*)nullptr);
    return hipGetLastError() == hipSuccess ? STOF_OK : STOF_ERR_HIP;
}
