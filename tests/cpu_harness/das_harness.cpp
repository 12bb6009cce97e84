// Stand-alone program around the beamformer's host entries (stofnet_amd/csrc/beamform.hip compiles as plain C++: its kernels
// are behind __HIPCC__).  tests/test_beamform_cpu.py builds it with -fsanitize=address,undefined and runs it as a child
// process: every buffer is a heap block of exactly the size the entry may touch, so a read of sample row S, of row 0 - 1 or
// past the pixel list aborts the program.  Exit status 0 and a last line "ok" mean every check held.
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <limits>
#include <vector>
#include "../../stofnet_amd/csrc/beamform.hip"

static int failures = 0;
#define CHECK(cond)                                                     \
    do {                                                                \
        if (!(cond)) {                                                  \
            printf("FAILED line %d: %s\n", __LINE__, #cond);            \
            ++failures;                                                 \
        }                                                               \
    } while (0)

struct Problem {
    int64_t F = 1, A = 1, S = 8, Ne = 1, P = 1;
    std::vector<double> x{0.0}, z{1.0}, dtx{0.0}, xe{0.0};
    stof_das_desc d{1.0, 0.0, 1.0, 0.25, 1.9, STOF_DAS_F64, 1};
};

// run `pr` on a signal whose sample row s of every column holds (s + 1, 10 (s + 1)); returns re / im of every output value
template <typename T>
static std::vector<T> run(Problem pr, int dtype, bool imag_on = true) {
    const bool cplx = dtype == STOF_DAS_C64 || dtype == STOF_DAS_C128;
    const int C = cplx ? 2 : 1;
    pr.d.dtype = dtype;
    const size_t n = (size_t)(pr.F * pr.A * pr.S * pr.Ne * C);
    T* sig = (T*)malloc(n ? n * sizeof(T) : 1);
    for (int64_t fa = 0; fa < pr.F * pr.A; ++fa)
        for (int64_t s = 0; s < pr.S; ++s)
            for (int64_t k = 0; k < pr.Ne; ++k) {
                T* v = sig + ((fa * pr.S + s) * pr.Ne + k) * C;
                v[0] = (T)(s + 1);
                if (cplx) v[1] = imag_on ? (T)(10 * (s + 1)) : (T)0;
            }
    uint8_t* rot = (uint8_t*)malloc((size_t)(pr.F * pr.A * pr.Ne) + 1);
    for (int64_t j = 0; j < pr.F * pr.A * pr.Ne; ++j) rot[j] = cplx && imag_on;
    const size_t no = (size_t)(pr.F * (pr.d.compound ? 1 : pr.A) * pr.P * C);
    T* out = (T*)malloc(no ? no * sizeof(T) : 1);
    for (size_t j = 0; j < no; ++j) out[j] = (T)-777;
    double *x = (double*)malloc(pr.P * sizeof(double) + 1), *z = (double*)malloc(pr.P * sizeof(double) + 1);
    double *dtx = (double*)malloc(pr.A * pr.P * sizeof(double) + 1), *xe = (double*)malloc(pr.Ne * sizeof(double) + 1);
    for (int64_t p = 0; p < pr.P; ++p) { x[p] = pr.x[p]; z[p] = pr.z[p]; }
    for (int64_t j = 0; j < pr.A * pr.P; ++j) dtx[j] = pr.dtx[j];
    for (int64_t k = 0; k < pr.Ne; ++k) xe[k] = pr.xe[k];
    const int st = stof_das_beamform_host(&pr.d, sig, pr.F, pr.A, pr.S, pr.Ne, x, z, dtx, pr.P, xe, rot, out);
    CHECK(st == STOF_OK);
    std::vector<T> res(out, out + no);
    free(sig); free(rot); free(out); free(x); free(z); free(dtx); free(xe);
    return res;
}

template <typename T>
static bool all_zero(const std::vector<T>& v) {
    for (T e : v)
        if (!(e == (T)0)) return false;
    return !v.empty();
}

template <typename T>
static void typed_checks(int real_dtype, int cplx_dtype) {
    const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();
    // ---- i == S - 1 exactly: c = fs = 1, t0 = 0, dtx = 0, the pixel straight under the element at depth S - 1
    {
        Problem pr;
        pr.z[0] = (double)(pr.S - 1);
        std::vector<T> r = run<T>(pr, real_dtype);
        CHECK(r.size() == 1 && r[0] == (T)pr.S);                        // sig[S - 1] * 1 + (row S, not read) * 0
        std::vector<T> c = run<T>(pr, cplx_dtype, false);               // complex dtype, purely real column: no rotation
        CHECK(c.size() == 2 && c[0] == (T)pr.S && c[1] == (T)0);
        c = run<T>(pr, cplx_dtype);                                     // f0 tau = 0.25 * 7 = 1.75 cycles -> times -i
        CHECK(fabs((double)c[0] - 10.0 * pr.S) < 1e-4 && fabs((double)c[1] + (double)pr.S) < 1e-4);
        pr.z[0] = 1.0;                                                  // i == 1 exactly: row 1 alone
        r = run<T>(pr, real_dtype);
        CHECK(r[0] == (T)2);
        pr.z[0] = 2.5;                                                  // in between: (3 + 4) / 2
        r = run<T>(pr, real_dtype);
        CHECK(r[0] == (T)3.5);
        pr.z[0] = nextafter((double)(pr.S - 1), 1e9);                   // just past the last sample: masked
        CHECK(all_zero(run<T>(pr, real_dtype)));
        pr.z[0] = nextafter(1.0, 0.0);                                  // just before sample 1: masked
        CHECK(all_zero(run<T>(pr, real_dtype)));
    }
    // ---- geometries that mask every term, and values that must not turn into an index
    const double t0s[] = {1.0, -1.0, inf, -inf, nan, 1e300, -1e300};
    for (double t0 : t0s)
        for (int dt : {real_dtype, cplx_dtype}) {
            Problem pr;
            pr.A = 2; pr.P = 3; pr.Ne = 2; pr.F = 2;
            pr.x = {0.0, 0.1, -0.1}; pr.z = {3.0, 4.0, 5.0}; pr.dtx = {0, 0, 0, 0.5, 0.5, 0.5}; pr.xe = {-0.05, 0.05};
            pr.d.c = 1540.0; pr.d.fs = 20e6; pr.d.t0 = t0;
            CHECK(all_zero(run<T>(pr, dt)));
            pr.d.compound = 0;
            CHECK(all_zero(run<T>(pr, dt)));
        }
    const double fss[] = {0.0, inf, -inf, nan, 1e300, -20e6};
    for (double fs : fss) {
        Problem pr;
        pr.z[0] = 3.0; pr.d.fs = fs; pr.d.t0 = 1e-3;
        CHECK(all_zero(run<T>(pr, cplx_dtype)));
    }
    const double bad[] = {inf, -inf, nan, 1e300, -1e300};
    for (double b : bad) {
        Problem pr;
        pr.z[0] = 3.0;
        Problem q = pr; q.dtx[0] = b; CHECK(all_zero(run<T>(q, real_dtype)));
        q = pr; q.x[0] = b; CHECK(all_zero(run<T>(q, cplx_dtype)));
        q = pr; q.xe[0] = b; CHECK(all_zero(run<T>(q, real_dtype)));
        q = pr; q.d.c = b; CHECK(all_zero(run<T>(q, cplx_dtype)));
        q = pr; q.d.fnumber = b; run<T>(q, real_dtype);                  // (an infinite cone or none: only the reads matter)
        q = pr; q.d.f0 = b; run<T>(q, cplx_dtype);
    }
    {
        Problem pr;                                                     // z = +-inf: the cone test passes or fails, i does not
        pr.z[0] = inf; CHECK(all_zero(run<T>(pr, real_dtype)));
        pr.z[0] = -inf; CHECK(all_zero(run<T>(pr, real_dtype)));
        pr.z[0] = 3.0; pr.d.c = 0.0; CHECK(all_zero(run<T>(pr, real_dtype)));
        pr.d.c = 1.0; pr.d.fnumber = 0.0; run<T>(pr, real_dtype);
    }
    // ---- too few samples for any term
    for (int64_t S : {0, 1}) {
        Problem pr;
        pr.S = S; pr.z[0] = 1.0;
        CHECK(all_zero(run<T>(pr, real_dtype)));
        CHECK(all_zero(run<T>(pr, cplx_dtype)));
    }
    {
        Problem pr;                                                     // S = 2: i == 1 == S - 1 is the only index
        pr.S = 2; pr.z[0] = 1.0;
        std::vector<T> r = run<T>(pr, real_dtype);
        CHECK(r[0] == (T)2);
    }
}

int main() {
    typed_checks<float>(STOF_DAS_F32, STOF_DAS_C64);
    typed_checks<double>(STOF_DAS_F64, STOF_DAS_C128);
    // the transmit distance table, W = 0 and a plain case
    {
        double xe1[1] = {0.0}, ang[2] = {0.0, 0.1}, x[2] = {3.0, -1.0}, z[2] = {4.0, 2.0}, dtx[4];
        CHECK(stof_das_tx_distance(xe1, 1, ang, 2, x, z, 2, dtx) == STOF_OK);
        CHECK(dtx[0] == 5.0 && dtx[2] == 5.0 && dtx[1] == hypot(-1.0, 2.0));
        double xe2[2] = {-1e-3, 1e-3};
        CHECK(stof_das_tx_distance(xe2, 2, ang, 1, x, z, 2, dtx) == STOF_OK);
        CHECK(fabs(dtx[0] - 4.0) < 1e-3 && fabs(dtx[1] - 2.0) < 1e-3);       // theta = 0: the depth, nearly (source 2e5 m away)
        CHECK(stof_das_tx_distance(xe2, 0, ang, 1, x, z, 2, dtx) == STOF_ERR_BAD_ARG);
    }
    {
        stof_das_desc d{1.0, 0.0, 1.0, 0.0, 1.9, 7, 1};
        double v = 0;
        CHECK(stof_das_beamform_host(&d, &v, 1, 1, 1, 1, &v, &v, &v, 1, &v, nullptr, &v) == STOF_ERR_BAD_ARG);
        CHECK(stof_das_beamform_host(nullptr, &v, 1, 1, 1, 1, &v, &v, &v, 1, &v, nullptr, &v) == STOF_ERR_BAD_ARG);
        d.dtype = STOF_DAS_F64;
        CHECK(stof_das_beamform_host(&d, &v, -1, 1, 1, 1, &v, &v, &v, 1, &v, nullptr, &v) == STOF_ERR_BAD_ARG);
        CHECK(stof_das_workspace_bytes(0, 5) == 0 && stof_das_workspace_bytes(2, 5) == 2 * 2 * sizeof(double));
    }
    if (failures) {
        printf("%d check(s) failed\n", failures);
        return 1;
    }
    printf("ok\n");
    return 0;
}
