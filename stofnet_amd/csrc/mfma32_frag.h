// Shared by the baselines' kernel files (zonzini.hip, sincnet.hip, riders.hip, waveunet.hip, kuleshov.hip).  Host part:
// the alignment of packed sections and workspace buffers, and the packer of the A-operand fragment order of
// v_mfma_f32_32x32x2_f32; plain C++, so that it also compiles for the host alone (tests/test_frag_pack_cpu.py drives it
// through a g++-built harness).  Device part, guarded, at the end: the accumulator type, the MFMA itself and the K loop
// that sn_conv_kernel and ed_conv_kernel share.
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

// Conv1d weight w [cout][cin][taps] (torch layout; a Linear weight [cout][K] is cin = cin_pad = 1, taps = K)
// -> out [ntiles][groups][64 lanes][4] in fragment order with k = tap * cin_pad + ci.  Zero wherever the element has no
// weight: output rows oc >= cout of the last tile, the pad channels ci >= cin of an activation stored cin_pad wide, and
// k past the real K (tap >= taps) of the last group.  w is read at real elements only.
inline void pack_frag32(const float* w, int64_t cout, int64_t cin, int64_t taps, int64_t cin_pad, int64_t ntiles,
                        int64_t groups, float* out) {
    for (int64_t nt = 0; nt < ntiles; ++nt)
        for (int64_t q = 0; q < groups; ++q)
            for (int lane = 0; lane < 64; ++lane)
                for (int e = 0; e < 4; ++e) {
                    const int64_t oc = 32 * nt + (lane & 31), k = 8 * q + 4 * (lane >> 5) + e;
                    const int64_t tap = k / cin_pad, ci = k % cin_pad;
                    const bool real = oc < cout && ci < cin && tap < taps;
                    out[((nt * groups + q) * 64 + lane) * 4 + e] = real ? w[(oc * cin + ci) * taps + tap] : 0.f;
                }
}

#if defined(__HIPCC__)
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
