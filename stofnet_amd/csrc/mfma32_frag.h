// Shared by the baselines' kernel files (zonzini.hip, sincnet.hip, riders.hip, waveunet.hip, kuleshov.hip).  Host part:
// the alignment of packed sections and workspace buffers, and the packer of the A-operand fragment order of
// v_mfma_f32_32x32x2_f32; plain C++, so that it also compiles for the host alone (tests/test_frag_pack_cpu.py drives it
// through a g++-built harness; frag_decode and frag32_element are the same code on the device).  Device part, guarded, at
// the end: the packer as a kernel, the accumulator type, the MFMA itself and the K loop that sn_conv_kernel and
// ed_conv_kernel share.
//
// Fragment order: lane l (i = l & 31, h = l >> 5), element e of K group q of N tile nt holds
//   W[32 nt + i][k = 8 q + 4 h + e]
// so that the four elements are one float4 of the lane and the A operand of lane l reads the activation at the same k
// with one float4.
#pragma once
#include <stdint.h>

namespace stof_frag {

constexpr int64_t ALIGN_F = 64;            // float alignment of every packed section and workspace buffer (256 B)

inline int64_t align_up(int64_t v) { return (v + ALIGN_F - 1) / ALIGN_F * ALIGN_F; }

#if defined(__HIPCC__)
#define STOF_FRAG_HD __host__ __device__
#else
#define STOF_FRAG_HD
#endif

// The fragment order, decoded: element o of an image [N tiles][groups][64 lanes][4] is row oc of its N tile nt at k.  The host
// packer and every device packer go through this one function; each adds only what its k means (tap, channel).
template <class I>
STOF_FRAG_HD inline void frag_decode(I o, I groups, I& nt, I& oc, I& k) {
    const I e = o & 3, lane = (o >> 2) & 63, rest = o >> 8, q = rest % groups;
    nt = rest / groups;
    oc = 32 * nt + (lane & 31);
    k = 8 * q + 4 * (lane >> 5) + e;
}

// Element o of the image of a Conv1d weight w [cout][cin][taps] (torch layout; a Linear weight [cout][K] is cin = cin_pad = 1,
// taps = K) with k = tap * cin_pad + ci.  Zero wherever the element has no weight: output rows oc >= cout of the last tile, the
// pad channels ci >= cin of an activation stored cin_pad wide, and k past the real K (tap >= taps) of the last group.  w is read
// at real elements only.
template <class I>
STOF_FRAG_HD inline float frag32_element(const float* w, I cout, I cin, I taps, I cin_pad, I groups, I o) {
    I nt, oc, k;
    frag_decode(o, groups, nt, oc, k);
    const I tap = k / cin_pad, ci = k % cin_pad;
    return (oc < cout && ci < cin && tap < taps) ? w[((int64_t)oc * cin + ci) * taps + tap] : 0.f;
}

// w -> out [ntiles][groups][64 lanes][4] in fragment order, on the host
inline void pack_frag32(const float* w, int64_t cout, int64_t cin, int64_t taps, int64_t cin_pad, int64_t ntiles,
                        int64_t groups, float* out) {
    for (int64_t o = 0; o < ntiles * groups * 256; ++o) out[o] = frag32_element(w, cout, cin, taps, cin_pad, groups, o);
}

#if defined(__HIPCC__)
// the same image on the device, `total` = ntiles * groups * 256 elements
static __global__ __launch_bounds__(256) void pack_frag32_kernel(const float* __restrict__ w, int cout, int cin, int taps, int cin_pad, int groups,
                                                          float* __restrict__ out, int total) {
    const int o = blockIdx.x * 256 + threadIdx.x;
    if (o < total) out[o] = frag32_element(w, cout, cin, taps, cin_pad, groups, o);
}
inline void pack_frag32_device(hipStream_t s, const float* w, int cout, int cin, int taps, int cin_pad, int groups, float* out, int total) {
    hipLaunchKernelGGL(pack_frag32_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, w, cout, cin, taps, cin_pad, groups, out,
                       total);
}

typedef float f32x16 __attribute__((ext_vector_type(16)));
#define MFMA32(a, b, acc) __builtin_amdgcn_mfma_f32_32x32x2f32((a), (b), (acc), 0, 0, 0)

// The K loop of an implicit-GEMM convolution whose A operand is a straight run of global memory: acc[nt] += A B[nt] over
// `groups` K groups.  a is the lane's first A float4 (K group q at a + 8 q floats), bq its float4 of N tile 0, group 0
// (N tile nt, group q at bq[(nt * groups + q) * 64]).  The next group's operands are loaded before this group's MFMAs.
// `groups` is a template parameter: as a run-time argument one instantiation of sn_conv_kernel was allocated other
// registers than with the loop written in place.
template <int NTW, int groups>
__device__ __forceinline__ void mfma32_k_loop(const float* a, const float4* bq, f32x16 (&acc)[NTW]) {
    float4 av = *reinterpret_cast<const float4*>(a);
    float4 bv[NTW];
#pragma unroll
    for (int nt = 0; nt < NTW; ++nt) bv[nt] = bq[(long long)nt * groups * 64];
    for (int q = 0; q < groups; ++q) {
        const float4 ca = av;
        float4 cb[NTW];
#pragma unroll
        for (int nt = 0; nt < NTW; ++nt) cb[nt] = bv[nt];
        if (q + 1 < groups) {
            av = *reinterpret_cast<const float4*>(a + 8 * (q + 1));
#pragma unroll
            for (int nt = 0; nt < NTW; ++nt) bv[nt] = bq[((long long)nt * groups + q + 1) * 64];
        }
#pragma unroll
        for (int nt = 0; nt < NTW; ++nt) acc[nt] = MFMA32(ca.x, cb[nt].x, acc[nt]);
#pragma unroll
        for (int nt = 0; nt < NTW; ++nt) acc[nt] = MFMA32(ca.y, cb[nt].y, acc[nt]);
#pragma unroll
        for (int nt = 0; nt < NTW; ++nt) acc[nt] = MFMA32(ca.z, cb[nt].z, acc[nt]);
#pragma unroll
        for (int nt = 0; nt < NTW; ++nt) acc[nt] = MFMA32(ca.w, cb[nt].w, acc[nt]);
    }
}
#endif

}  // namespace stof_frag
