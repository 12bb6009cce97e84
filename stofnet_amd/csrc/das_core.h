// Plane-wave delay-and-sum (utils/beamform.py: bf_das_rx of the reference): the arithmetic of ONE (pixel, element) term,
// host/device neutral.  The kernel (beamform.hip), the host entry and the CPU harness all run this text, so the delay,
// both masks, the interpolation weights and the phase cannot drift apart.
//
//   drx = hypot(x - xe[k], z)            tau = (dtx + drx) / c            i = (tau - t0) * fs          (all double)
//   cone mask   |x - xe[k]| < z / fnumber / 2   (strict; the two divisions in this order)
//   range mask  1 <= i <= S - 1, written so that NaN and +-inf fail it; f = floor(i)
//   term        sig[f, k] * (f + 1 - i) + sig[f + 1, k] * (i - f); at i == S - 1 the second weight is 0 and row S is
//               never read (second == false)
//   phase       exp(2 pi i f0 tau): f0 * tau is reduced to [0, 1) cycles in double before the sine and cosine are taken
//               in the scalar type
// dtx (the transmit distance of the pixel for one angle) comes from a table: it is a difference of two numbers near
// 1e6 m (das_tx_distance below) and has to be the same double everywhere.
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define DAS_HD __host__ __device__ __forceinline__
#else
#define DAS_HD inline
#endif

namespace das {

struct Geom {
    double c, t0, fs, f0, fnumber;
};

template <typename T>
struct Term {
    long long f;        // first sample row, 1 <= f <= S - 1
    bool second;        // row f + 1 exists (false only at i == S - 1)
    T w0, w1;           // weights of rows f and f + 1
    T cs, sn;           // cos / sin of the phase (filled when `rotate`)
};

DAS_HD void sincos_cycles(double cycles, float& s, float& c) {
    const float a = (float)(6.283185307179586476925 * cycles);
    s = sinf(a);
    c = cosf(a);
}
DAS_HD void sincos_cycles(double cycles, double& s, double& c) {
    const double a = 6.283185307179586476925 * cycles;
    s = sin(a);
    c = cos(a);
}

// false: the term is masked (nothing of `t` is valid).  No input value leads to f outside [1, S - 1].
template <typename T>
DAS_HD bool term(const Geom& g, double x, double z, double xek, double dtx, long long S, bool rotate, Term<T>& t) {
    if (!(fabs(x - xek) < z / g.fnumber / 2.0)) return false;
    const double drx = hypot(x - xek, z);
    const double tau = (dtx + drx) / g.c;
    const double i = (tau - g.t0) * g.fs;
    if (!(i >= 1.0 && i <= (double)(S - 1))) return false;
    const double fl = floor(i);
    t.f = (long long)fl;
    t.second = t.f + 1 < S;
    t.w0 = (T)(fl + 1.0 - i);
    t.w1 = (T)(i - fl);
    if (rotate) {
        double cyc = g.f0 * tau;
        cyc -= floor(cyc);
        if (!(cyc >= 0.0 && cyc < 1.0)) cyc = 0.0;       // |f0 tau| beyond 2^52, or not finite: no phase left to keep
        sincos_cycles(cyc, t.sn, t.cs);
    }
    return true;
}

// One real term: rows f and f + 1 of column k.
template <typename T>
DAS_HD T interp(const Term<T>& t, const T* col, long long stride) {
    const T s0 = col[t.f * stride];
    const T s1 = t.second ? col[(t.f + 1) * stride] : (T)0;
    return s0 * t.w0 + s1 * t.w1;
}

// One complex term (interleaved re, im; `stride` counts complex values), rotated by the phase when `rotate`.
template <typename T>
DAS_HD void interp_c(const Term<T>& t, const T* col, long long stride, bool rotate, T& re, T& im) {
    const T* p0 = col + 2 * t.f * stride;
    T r = p0[0] * t.w0, q = p0[1] * t.w0;
    if (t.second) {
        const T* p1 = p0 + 2 * stride;
        r = r + p1[0] * t.w1;
        q = q + p1[1] * t.w1;
    }
    if (rotate) {
        re = r * t.cs - q * t.sn;
        im = r * t.sn + q * t.cs;
    } else {
        re = r;
        im = q;
    }
}

// Transmit distance of pixel (x, z) for the virtual source of angle theta behind an aperture of width W (host only: libm).
struct Source {
    double v0, v1, edge;    // edge = hypot(g, v1), g = |v0| - W/2 when |v0| > W/2, else 0
};
inline Source source(double W, double theta) {
    const double beta = 1e-8, ct = cos(theta), st = sin(theta);
    Source s;
    s.v0 = -W * ct * st / beta;
    s.v1 = -W * (ct * ct) / beta;
    const double g = fabs(s.v0) > W / 2 ? fabs(s.v0) - W / 2 : 0.0;
    s.edge = hypot(g, s.v1);
    return s;
}
inline double tx_distance(const Source& s, double x, double z) { return hypot(x - s.v0, z - s.v1) - s.edge; }

}  // namespace das
