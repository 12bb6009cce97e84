// SemiGlobalBlock expand conv of the inference forward (models/stofnet.py:106-107), split fp16:
//
//   pooled[N][P][512] -> expand_conv 512->64 k5 (same padding) -> lrelu => sgb[N][P][64]
//
// A GEMM of N (P + 2) rows x 64 x 2560.  The arithmetic is that of conv_cl_kernel<F16X3, BLOCKSUM> (train.hip), which
// served this conv before and still serves training: v_mfma_f32_32x32x16_f16 with the weights on M and time on N; per
// 64-channel input block an accumulator of its own over taps 0..4 and k-groups 0..3 in the order w_hi x_hi, w_hi x_lo,
// w_lo x_hi; blocks folded in order 0..7; bias; leaky ReLU.  Every output element sees the same operations in the same
// order, so the map is bit-identical.  What differs is the data movement:
//
//   * a work-group takes 256 rows of the row stream (the P pooled rows of a waveform followed by 2 zero gap rows, which
//     are the conv's padding; gap rows and rows past the ends are zeroed by predicate when the tile is loaded, so no
//     output row ever sees another waveform's pooled rows) and all 64 output channels;
//   * per input block, the 260 activation rows (split into fp16 hi | lo once, on the way into LDS) and ALL FIVE weight
//     taps are staged in LDS between one pair of barriers; a tap is then a row offset into the resident activations;
//   * wave (mi, ni) owns output channels 32 mi.. and rows 128 ni..: a weight fragment read from LDS feeds four 32-row
//     accumulator tiles, 10 ds_read_b128 per 12 MFMAs (the LDS array sustains 2 per MFMA, MI355X_MICROARCH.md);
//   * the next block's activations and weights travel HBM / L2 -> registers while the 480 MFMAs of the current block
//     run (15 k cycles against a load latency of 1-2 k), so the single LDS buffer costs no wait.
//
// LDS rows are 272 B (68 floats) as in conv_cl_kernel: a lane reads 16 B of row (lane & 31) + const, and the
// ds_read_b128 lane groups {0-3, 12-15, 20-27} / {4-11, 16-19, 28-31} then cover all 64 banks once (row r starts at bank
// 4 r mod 64).  LDS = (260 + 5 * 64) * 272 B = 157,760 B of the 163,840 B: one work-group (one wave per SIMD) per CU.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "stof_common.h"
#include "stof_hip_util.h"

typedef float floatx16 __attribute__((ext_vector_type(16)));
typedef _Float16 half8 __attribute__((ext_vector_type(8)));
typedef _Float16 half4v __attribute__((ext_vector_type(4)));
typedef float float4v __attribute__((ext_vector_type(4)));

namespace {

constexpr int EX_ROWS = 256;              // stream rows per work-group
constexpr int EX_K = 5, EX_PAD = 2;
constexpr int EX_XR = EX_ROWS + EX_K - 1; // activation rows resident per block
constexpr int EX_CIN = 512, EX_COUT = 64, EX_NCB = EX_CIN / 64;
constexpr int EX_RF = 68;                 // LDS row stride in floats (272 B)
constexpr int EX_RB = EX_RF * 4;
constexpr int EX_NXR = (EX_XR * 16 + 255) / 256;          // float4 per thread of an activation block (17)
constexpr int EX_NWR = EX_K * EX_COUT * 16 / 256;         // float4 per thread of a block's five weight taps (20)
constexpr size_t EX_LDS_BYTES = (size_t)(EX_XR + EX_K * EX_COUT) * EX_RB;

struct ExpandParams {
    const float* pooled;   // [nb][P][512] fp32
    const float* w;        // split layout [5][64][8][64 hi | 64 lo halfs] (pack_weights.cpp)
    const float* bias;     // [64]
    float* sgb;            // [nb][P][64]
    int P, period;         // period = P + 2
    int total;             // nb * period stream rows
    const int* run_if;     // as BodyParams::run_if
};

__device__ __forceinline__ float4 ld4(const float* p) { return *reinterpret_cast<const float4*>(p); }
__device__ __forceinline__ uint4 ldq(const char* p) { return *reinterpret_cast<const uint4*>(p); }

__device__ __forceinline__ floatx16 mfma_h(uint4 a, uint4 b, floatx16 c) {
    union U { uint4 u; half8 h; };
    U x, y;
    x.u = a; y.u = b;
    return __builtin_amdgcn_mfma_f32_32x32x16_f16(x.h, y.h, c, 0, 0, 0);
}

// 4 fp32 values -> (hi, lo) fp16 quads packed as two 8-byte words (as split4 of train.hip)
__device__ __forceinline__ void split4(float4 v, uint2& hi, uint2& lo) {
    const float4v f = {v.x, v.y, v.z, v.w};
    const half4v h = __builtin_convertvector(f, half4v);
    const float4v d = f - __builtin_convertvector(h, float4v);
    const half4v l = __builtin_convertvector(d, half4v);
    union { half4v h; uint2 u; } a, b;
    a.h = h; b.h = l;
    hi = a.u; lo = b.u;
}

__global__ __launch_bounds__(256) void sgb_expand_kernel(const ExpandParams p) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    char* const xs = reinterpret_cast<char*>(smem);                       // [EX_XR] rows
    char* const ws = xs + EX_XR * EX_RB;                                  // [5][64] rows
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int mi = wave & 1, ni = wave >> 1, ln = lane & 31, lh = lane >> 5;
    if (p.run_if != nullptr && *p.run_if == 0) return;
    const int t0 = blockIdx.x * EX_ROWS;

    // this thread's activation pieces: LDS row r = (tid + 256 u) / 16 holds stream row t0 - 2 + r; 4 channels at 4 q
    const int xq = tid & 15;
    int xsrc[EX_NXR];          // pooled row of the piece, -1: zero (gap row, outside the stream, or past the tile)
#pragma unroll
    for (int u = 0; u < EX_NXR; ++u) {
        const int r = (tid + 256 * u) >> 4;
        const int t = t0 - EX_PAD + r;
        int src = -1;
        if (r < EX_XR && t >= 0 && t < p.total) {
            const int nn = t / p.period, pp = t - nn * p.period;
            if (pp < p.P) src = nn * p.P + pp;
        }
        xsrc[u] = src;
    }
    float4 xreg[EX_NXR], wreg[EX_NWR];
    auto fetch = [&](int cb) {
#pragma unroll
        for (int u = 0; u < EX_NXR; ++u) {
            float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
            if (xsrc[u] >= 0) v = ld4(p.pooled + (size_t)xsrc[u] * EX_CIN + 64 * cb + 4 * xq);
            xreg[u] = v;
        }
#pragma unroll
        for (int u = 0; u < EX_NWR; ++u) {
            const int i = tid + 256 * u;                                  // (tap, o) = i / 16: a 256-byte row of the split layout
            wreg[u] = ld4(p.w + ((size_t)(i >> 4) * EX_NCB + cb) * 64 + 4 * (i & 15));
        }
    };
    fetch(0);

    floatx16 acc[4], tot[4];
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int e = 0; e < 16; ++e) { acc[j][e] = 0.f; tot[j][e] = 0.f; }

    for (int cb = 0; cb < EX_NCB; ++cb) {
        if (cb > 0) {
#pragma unroll
            for (int j = 0; j < 4; ++j)
#pragma unroll
                for (int e = 0; e < 16; ++e) { tot[j][e] += acc[j][e]; acc[j][e] = 0.f; }
            __syncthreads();                                              // every wave has read the previous block
        }
#pragma unroll
        for (int u = 0; u < EX_NXR; ++u) {
            const int r = (tid + 256 * u) >> 4;
            if (r >= EX_XR) continue;
            uint2 hi, lo;
            split4(xreg[u], hi, lo);
            char* row = xs + r * EX_RB;
            *reinterpret_cast<uint2*>(row + 8 * xq) = hi;
            *reinterpret_cast<uint2*>(row + 128 + 8 * xq) = lo;
        }
#pragma unroll
        for (int u = 0; u < EX_NWR; ++u) {
            const int i = tid + 256 * u;
            *reinterpret_cast<float4*>(ws + (i >> 4) * EX_RB + 16 * (i & 15)) = wreg[u];
        }
        if (cb + 1 < EX_NCB) fetch(cb + 1);
        __syncthreads();

        const char* const ar0 = ws + (32 * mi + ln) * EX_RB + 16 * lh;
        const char* const br0 = xs + (128 * ni + ln) * EX_RB + 16 * lh;
#pragma unroll
        for (int d = 0; d < EX_K; ++d) {
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const char* ar = ar0 + d * EX_COUT * EX_RB + 32 * q;
                const char* br = br0 + d * EX_RB + 32 * q;
                const uint4 ah = ldq(ar), al = ldq(ar + 128);
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const uint4 bh = ldq(br + 32 * j * EX_RB), bl = ldq(br + 32 * j * EX_RB + 128);
                    acc[j] = mfma_h(ah, bh, acc[j]);
                    acc[j] = mfma_h(ah, bl, acc[j]);
                    acc[j] = mfma_h(al, bh, acc[j]);
                }
            }
        }
    }
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int e = 0; e < 16; ++e) acc[j][e] += tot[j][e];

    // epilogue: lane (ln, lh) holds stream row t0 + 128 ni + 32 j + ln, channels 32 mi + 8 gg + 4 lh + e
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int t = t0 + 128 * ni + 32 * j + ln;
        if (t >= p.total) continue;
        const int nn = t / p.period, pp = t - nn * p.period;
        if (pp >= p.P) continue;
        float* const orow = p.sgb + ((size_t)nn * p.P + pp) * EX_COUT;
#pragma unroll
        for (int gg = 0; gg < 4; ++gg) {
            const int o = 32 * mi + 8 * gg + 4 * lh;
            const float4 b = ld4(p.bias + o);
            const float bi[4] = {b.x, b.y, b.z, b.w};
            float v[4];
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                float x = acc[j][4 * gg + e] + bi[e];
                x = x > 0.f ? x : 0.01f * x;
                v[e] = x + 0.f;                                           // conv_cl_kernel adds its (absent) residual: -0 -> +0
            }
            *reinterpret_cast<float4*>(orow + o) = make_float4(v[0], v[1], v[2], v[3]);
        }
    }
}

}  // namespace

namespace stof {

// split-fp16 expand conv of the inference forward on the pooled grid; `w` in the split layout of pack_weights.cpp
int launch_sgb_expand(const float* pooled, const float* w, const float* bias, float* sgb, int64_t nb, int64_t P,
                      hipStream_t stream, const int* run_if) {
    if (nb <= 0 || P <= 0) return STOF_OK;
    if (!pooled || !w || !bias || !sgb) return STOF_ERR_BAD_ARG;
    const int64_t total = nb * (P + 2);
    if (total + EX_ROWS > 0x7fffffffLL) return STOF_ERR_UNSUPPORTED;      // stream rows are int32
    static LdsLimitOnce lds;
    if (int st = lds.ensure(reinterpret_cast<const void*>(&sgb_expand_kernel), (int)EX_LDS_BYTES)) return st;
    ExpandParams p;
    p.pooled = pooled; p.w = w; p.bias = bias; p.sgb = sgb;
    p.P = (int)P; p.period = (int)(P + 2); p.total = (int)total;
    p.run_if = run_if;
    hipLaunchKernelGGL(sgb_expand_kernel, dim3((unsigned)((total + EX_ROWS - 1) / EX_ROWS)), dim3(256), EX_LDS_BYTES, stream, p);
    return hipGetLastError() == hipSuccess ? STOF_OK : STOF_ERR_HIP;
}

}  // namespace stof
