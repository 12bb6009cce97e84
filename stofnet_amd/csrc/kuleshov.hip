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
#include <hip/hip_runtime.h>
#include <math.h>
#include <string.h>
#include "mfma32_frag.h"
#include "stof_common.h"

namespace {

using namespace stof_frag;

constexpr int NL = 4;
constexpr int NF[NL] = {128, 256, 512, 512};
constexpr int FS[NL] = {65, 33, 17, 9};
constexpr int FS0 = 65;                         // taps of down_conv0 (= FS[0]; a scalar for device code)
constexpr int KB = 9;                           // bottleneck and final_conv taps
constexpr int C0 = 128;                         // width of down 0 and of final_conv's input
constexpr int UP_CIN[NL] = {512, 512, 512, 256};
constexpr int UP_COUT[NL] = {1024, 1024, 512, 256};
constexpr int UP_FS[NL] = {9, 17, 33, 65};
constexpr int MIN_L = 641;                      // shortest input for which every convolution has an output
constexpr int T0 = 64;                          // outputs per work-group of ks_down0_kernel
constexpr int XS0 = 2 * T0 + 64;                // its LDS window (2 (T0 - 1) + 65 samples, rounded up)
constexpr int FIN_T = 16;                       // positions per wave of ks_final_kernel
constexpr int QU_WIDE = 1, QU_MID = 2, QU_NARROW = 4;   // K groups per step of the 64 x 128, 32 x 128 and 32 x 32 wave tile
constexpr int FC_MT = 4;                        // M tiles (of 32 rows) per work-group of ks_fc_kernel
constexpr int NUM_PARAMS = 54;                  // see stof_kuleshov_pack_weights in include/stofnet_amd.h
enum { EP_DOWN = 0, EP_BOTT = 1, EP_UP = 2 };

struct Dims {
    int64_t L, O, D[NL], B, U[NL], Lc[NL], F, Kp, G, OT;
};

bool dims(const stof_kuleshov_desc* d, Dims* o) {
    if (!d || d->input_length < MIN_L || d->output_length < 1 || !std::isfinite(d->bn_eps) || d->bn_eps < 0.0) return false;
    if (d->tile_variant < 0 || d->tile_variant > 3) return false;
    if (d->input_length >= (1ll << 24) || d->output_length >= (1ll << 24)) return false;
    o->L = d->input_length;
    o->O = d->output_length;
    int64_t w = o->L;
    for (int i = 0; i < NL; ++i) {
        w = (w - FS[i]) / 2 + 1;
        o->D[i] = w;
    }
    o->B = (w - KB) / 2 + 1;
    w = o->B;
    for (int i = 0; i < NL; ++i) {
        o->U[i] = w - UP_FS[i] + 1;
        if (o->U[i] < 1) return false;
        w = 2 * o->U[i] + o->D[NL - 1 - i];
        o->Lc[i] = w;
    }
    o->F = w - KB + 1;
    o->Kp = (2 * o->F + 7) / 8 * 8;
    o->G = o->Kp / 8;
    o->OT = (o->O + 31) / 32;
    return true;
}

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

__device__ __forceinline__ float leaky(float v, float slope) { return v > 0.f ? v : slope * v; }   // NaN stays NaN

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

// ----------------------------------------------------------------------------------------------- the implicit GEMM
struct ConvArgs {
    const float* in;             // row 0 of waveform 0 of the input range
    long long in_n_stride;       // floats between waveforms
    float* out;                  // row 0 of waveform 0 of the output range (for EP_UP: of the concatenation buffer)
    long long out_n_stride;
    float* out2;                 // optional second copy of the output (the bottleneck tap), dense [N][Lout][Cout]
    const float4* frag;
    const float* ep;             // [3][Cout]
    unsigned M, Lout;            // M = N Lout
    int Cin, Cout, stride, G, mode;
};

// Wave (blockIdx.x, w) owns flattened outputs m0 .. m0 + 32 MT - 1 (m = n Lout + t) and N tiles blockIdx.y NTW .. + NTW - 1.
// Lane (i = l & 31, h = l >> 5) of M tile mt reads its own output's K span at k = 8 q + 4 h .. + 3; a step takes QU K
// groups, and the next step's operands are loaded before this step's MFMAs (the small tiles have few MFMAs per group
// and few waves per SIMD, so they keep more loads in flight).  Tail lanes compute a duplicate of output M - 1 and store
// nothing.
template <int MT, int NTW, int QU>
__global__ __launch_bounds__(256) void ks_conv_kernel(const ConvArgs p) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const unsigned m0 = ((unsigned)blockIdx.x * 4 + wave) * (32 * MT);
    if (m0 >= p.M) return;
    const int i = lane & 31, h = lane >> 5;
    const int G = p.G;                                  // a multiple of 16 (Cin >= 128), so of QU
    const float* a[MT];
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) {
        unsigned m = m0 + 32 * mt + i;
        if (m >= p.M) m = p.M - 1;
        const unsigned n = m / p.Lout, t = m - n * p.Lout;
        a[mt] = p.in + (long long)n * p.in_n_stride + (long long)t * p.stride * p.Cin + 4 * h;
    }
    const int nt0 = blockIdx.y * NTW;
    const float4* bq = p.frag + (long long)nt0 * G * 64 + lane;
    f32x16 acc[MT][NTW] = {};
    float4 av[QU][MT], bv[QU][NTW];
#pragma unroll
    for (int u = 0; u < QU; ++u) {
#pragma unroll
        for (int mt = 0; mt < MT; ++mt) av[u][mt] = *reinterpret_cast<const float4*>(a[mt] + 8 * u);
#pragma unroll
        for (int nt = 0; nt < NTW; ++nt) bv[u][nt] = bq[((long long)nt * G + u) * 64];
    }
    for (int q = 0; q < G; q += QU) {
        float4 ca[QU][MT], cb[QU][NTW];
#pragma unroll
        for (int u = 0; u < QU; ++u) {
#pragma unroll
            for (int mt = 0; mt < MT; ++mt) ca[u][mt] = av[u][mt];
#pragma unroll
            for (int nt = 0; nt < NTW; ++nt) cb[u][nt] = bv[u][nt];
        }
        if (q + QU < G) {
#pragma unroll
            for (int u = 0; u < QU; ++u) {
#pragma unroll
                for (int mt = 0; mt < MT; ++mt) av[u][mt] = *reinterpret_cast<const float4*>(a[mt] + 8 * (q + QU + u));
#pragma unroll
                for (int nt = 0; nt < NTW; ++nt) bv[u][nt] = bq[((long long)nt * G + q + QU + u) * 64];
            }
        }
#pragma unroll
        for (int u = 0; u < QU; ++u) {
#pragma unroll
            for (int mt = 0; mt < MT; ++mt)
#pragma unroll
                for (int nt = 0; nt < NTW; ++nt) acc[mt][nt] = MFMA32(ca[u][mt].x, cb[u][nt].x, acc[mt][nt]);
#pragma unroll
            for (int mt = 0; mt < MT; ++mt)
#pragma unroll
                for (int nt = 0; nt < NTW; ++nt) acc[mt][nt] = MFMA32(ca[u][mt].y, cb[u][nt].y, acc[mt][nt]);
#pragma unroll
            for (int mt = 0; mt < MT; ++mt)
#pragma unroll
                for (int nt = 0; nt < NTW; ++nt) acc[mt][nt] = MFMA32(ca[u][mt].z, cb[u][nt].z, acc[mt][nt]);
#pragma unroll
            for (int mt = 0; mt < MT; ++mt)
#pragma unroll
                for (int nt = 0; nt < NTW; ++nt) acc[mt][nt] = MFMA32(ca[u][mt].w, cb[u][nt].w, acc[mt][nt]);
        }
    }
    // C/D map: column (channel) = lane & 31, row (output) = (r & 3) + 8 (r >> 2) + 4 h
    const int Cout = p.Cout;
#pragma unroll
    for (int nt = 0; nt < NTW; ++nt) {
        const int c = 32 * (nt0 + nt) + i;
        const float b = p.ep[c], s = p.ep[Cout + c], t = p.ep[2 * Cout + c];
#pragma unroll
        for (int mt = 0; mt < MT; ++mt) {
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const unsigned row = m0 + 32 * mt + (r & 3) + 8 * (r >> 2) + 4 * h;
                if (row >= p.M) continue;
                const unsigned rn = row / p.Lout, rt = row - rn * p.Lout;
                float* const o = p.out + (long long)rn * p.out_n_stride;
                const float v = acc[mt][nt][r];
                if (p.mode == EP_UP) {
                    o[(long long)(2 * rt + (c & 1)) * (Cout >> 1) + (c >> 1)] = fmaf(v, s, t);
                } else {
                    const float u = p.mode == EP_DOWN ? leaky(fmaf(leaky(v + b, 0.01f), s, t), 0.2f) : leaky(v + b, 0.2f);
                    o[(long long)rt * Cout + c] = u;
                    if (p.out2) p.out2[(long long)row * Cout + c] = u;
                }
            }
        }
    }
}

// ------------------------------------------------------------------------------------------------------ final_conv
// Wave: row n, positions t0 .. t0 + 15 of flat's Kp / 2 position pairs.  Lane l keeps channels 2 l, 2 l + 1 of rows
// t0 .. t0 + 23 (rows past Lc3 feed no stored output and are not read), then per position the fma chain over (tap,
// channel pair) for both output channels and the xor-butterfly over the lanes.  Positions >= F are flat's zero tail.
__global__ __launch_bounds__(256) void ks_final_kernel(const float* __restrict__ in, long long N, int Lc, int F, int Kp,
                                                       int tblocks, const float* __restrict__ wf,
                                                       const float* __restrict__ bf, float* __restrict__ flat,
                                                       float* __restrict__ tap) {
    const int lane = threadIdx.x & 63;
    const long long wid = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (wid >= N * tblocks) return;
    const long long n = wid / tblocks;
    const int t0 = (int)(wid % tblocks) * FIN_T;
    constexpr int R = FIN_T + KB - 1;
    const float* base = in + n * (long long)Lc * C0 + 2 * lane;
    float2 v[R];
#pragma unroll
    for (int j = 0; j < R; ++j) {
        const int t = t0 + j;
        v[j] = t < Lc ? *reinterpret_cast<const float2*>(base + (long long)t * C0) : make_float2(0.f, 0.f);
    }
    float2 w[2][KB];
#pragma unroll
    for (int oc = 0; oc < 2; ++oc)
#pragma unroll
        for (int j = 0; j < KB; ++j) w[oc][j] = *reinterpret_cast<const float2*>(wf + (oc * KB + j) * C0 + 2 * lane);
    const float b0 = bf[0], b1 = bf[1];
#pragma unroll
    for (int u = 0; u < FIN_T; ++u) {
        float a0 = 0.f, a1 = 0.f;
#pragma unroll
        for (int j = 0; j < KB; ++j) {
            a0 = fmaf(w[0][j].x, v[u + j].x, a0);
            a0 = fmaf(w[0][j].y, v[u + j].y, a0);
            a1 = fmaf(w[1][j].x, v[u + j].x, a1);
            a1 = fmaf(w[1][j].y, v[u + j].y, a1);
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            a0 += __shfl_xor(a0, o);
            a1 += __shfl_xor(a1, o);
        }
        const int pos = t0 + u;
        if (lane == u && 2 * pos < Kp) {
            const bool live = pos < F;
            const float2 r = live ? make_float2(a0 + b0, a1 + b1) : make_float2(0.f, 0.f);
            *reinterpret_cast<float2*>(flat + n * (long long)Kp + 2 * pos) = r;
            if (tap && live) *reinterpret_cast<float2*>(tap + n * 2ll * F + 2 * pos) = r;
        }
    }
}

// ------------------------------------------------------------------------------------------------------- output_fc
// Work-group bid: M group mg = bid % mgroups (rows 32 MTW mg ..), output tile ot = bid / mgroups (outputs 32 ot ..), so
// that the groups sharing a weight tile run together.  Wave w accumulates K groups q = w, w + 4, .., QU of them per
// step (a small batch is bound by streaming the weight, so 8 KiB per wave are in flight); waves 1..3 park their
// accumulators in LDS and wave 0 adds them in order and stores y = sum + bias.
template <int MTW, int QU>
__global__ __launch_bounds__(256) void ks_fc_kernel(const float* __restrict__ flat, int Kp, unsigned rows, int mgroups,
                                                    const float4* __restrict__ frag, int G, const float* __restrict__ bias,
                                                    int O, float* __restrict__ y) {
    __shared__ float part[3][MTW][16][64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int i = lane & 31, h = lane >> 5;
    const unsigned mg = blockIdx.x % mgroups, ot = blockIdx.x / mgroups;
    const unsigned m0 = mg * (32 * MTW);
    const float* a[MTW];
#pragma unroll
    for (int mt = 0; mt < MTW; ++mt) {
        unsigned m = m0 + 32 * mt + i;
        if (m >= rows) m = rows - 1;
        a[mt] = flat + (long long)m * Kp + 4 * h;
    }
    const float4* bq = frag + (long long)ot * G * 64 + lane;
    f32x16 acc[MTW] = {};
    // QU groups (q, q + 4, ..) per step; the loads of the next step are issued before this step's MFMAs
    float4 av[QU][MTW], bv[QU];
#pragma unroll
    for (int u = 0; u < QU; ++u) {
        const int qq = wave + 4 * u;
        if (qq < G) {
#pragma unroll
            for (int mt = 0; mt < MTW; ++mt) av[u][mt] = *reinterpret_cast<const float4*>(a[mt] + 8 * qq);
            bv[u] = bq[(long long)qq * 64];
        }
    }
    for (int q = wave; q < G; q += 4 * QU) {
        float4 ca[QU][MTW], cb[QU];
#pragma unroll
        for (int u = 0; u < QU; ++u) {
#pragma unroll
            for (int mt = 0; mt < MTW; ++mt) ca[u][mt] = av[u][mt];
            cb[u] = bv[u];
        }
#pragma unroll
        for (int u = 0; u < QU; ++u) {
            const int qq = q + 4 * (QU + u);
            if (qq < G) {
#pragma unroll
                for (int mt = 0; mt < MTW; ++mt) av[u][mt] = *reinterpret_cast<const float4*>(a[mt] + 8 * qq);
                bv[u] = bq[(long long)qq * 64];
            }
        }
#pragma unroll
        for (int u = 0; u < QU; ++u) {
            if (q + 4 * u < G) {
#pragma unroll
                for (int mt = 0; mt < MTW; ++mt) acc[mt] = MFMA32(ca[u][mt].x, cb[u].x, acc[mt]);
#pragma unroll
                for (int mt = 0; mt < MTW; ++mt) acc[mt] = MFMA32(ca[u][mt].y, cb[u].y, acc[mt]);
#pragma unroll
                for (int mt = 0; mt < MTW; ++mt) acc[mt] = MFMA32(ca[u][mt].z, cb[u].z, acc[mt]);
#pragma unroll
                for (int mt = 0; mt < MTW; ++mt) acc[mt] = MFMA32(ca[u][mt].w, cb[u].w, acc[mt]);
            }
        }
    }
    if (wave > 0) {
#pragma unroll
        for (int mt = 0; mt < MTW; ++mt)
#pragma unroll
            for (int r = 0; r < 16; ++r) part[wave - 1][mt][r][lane] = acc[mt][r];
    }
    __syncthreads();
    if (wave > 0) return;
    const int o = 32 * (int)ot + i;
    if (o >= O) return;
    const float b = bias[o];
#pragma unroll
    for (int mt = 0; mt < MTW; ++mt) {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const unsigned row = m0 + 32 * mt + (r & 3) + 8 * (r >> 2) + 4 * h;
            if (row >= rows) continue;
            const float sum = ((acc[mt][r] + part[0][mt][r][lane]) + part[1][mt][r][lane]) + part[2][mt][r][lane];
            y[(long long)row * O + o] = sum + b;
        }
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

template <typename K, typename... A>
bool launch(K kernel, dim3 grid, hipStream_t s, A... args) {
    hipLaunchKernelGGL(kernel, grid, dim3(256), 0, s, args...);
    return hipGetLastError() == hipSuccess;
}

bool launch_conv(const ConvArgs& p, int variant, hipStream_t s) {
    const int64_t M = p.M, nb = p.Cout / 128;
    if (variant == 0) variant = (M + 63) / 64 * nb >= 1536 ? 3 : (M + 31) / 32 * nb >= 1024 ? 2 : 1;
    if (variant == 3) return launch(ks_conv_kernel<2, 4, QU_WIDE>, dim3((unsigned)((M + 255) / 256), (unsigned)nb), s, p);
    if (variant == 2) return launch(ks_conv_kernel<1, 4, QU_MID>, dim3((unsigned)((M + 127) / 128), (unsigned)nb), s, p);
    return launch(ks_conv_kernel<1, 1, QU_NARROW>, dim3((unsigned)((M + 127) / 128), (unsigned)(p.Cout / 32)), s, p);
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
