// Host harness for tests/test_frag_pack_cpu.py: runs pack_frag32 of stofnet_amd/csrc/mfma32_frag.h, the packer behind
// every stof_*_pack_weights of the baselines, on the CPU.  Built with -DFRAG_HARNESS_MAIN it is a stand-alone program
// that packs the test's five cases from weights allocated at their exact size and checks them against a dense [row][k]
// image, so that a sanitizer build (-fsanitize=address,undefined) shows a guard that reads past a weight.
#include "../../stofnet_amd/csrc/mfma32_frag.h"

extern "C" void frag_pack(const float* w, int cout, int cin, int taps, int cin_pad, int ntiles, int groups, float* out) {
    stof_frag::pack_frag32(w, cout, cin, taps, cin_pad, ntiles, groups, out);
}

#ifdef FRAG_HARNESS_MAIN
#include <stdio.h>
#include <vector>

// cout, cin, taps, cin_pad, ntiles, groups
static const int CASES[5][6] = {{64, 64, 3, 64, 2, 24}, {3, 32, 3, 32, 1, 12}, {50, 16, 10, 32, 2, 40}, {32, 1, 1024, 1, 1, 128},
                                {5, 1, 13, 1, 1, 2}};

int main() {
    for (const auto& c : CASES) {
        const int cout = c[0], cin = c[1], taps = c[2], cin_pad = c[3], ntiles = c[4], groups = c[5], K = 8 * groups;
        std::vector<float> w((size_t)cout * cin * taps), dense((size_t)32 * ntiles * K, 0.f), out((size_t)ntiles * groups * 256, -1.f);
        for (size_t i = 0; i < w.size(); ++i) w[i] = (float)(i + 1);
        for (int oc = 0; oc < cout; ++oc)
            for (int ci = 0; ci < cin; ++ci)
                for (int t = 0; t < taps; ++t)
                    if (t * cin_pad + ci < K) dense[(size_t)oc * K + t * cin_pad + ci] = w[((size_t)oc * cin + ci) * taps + t];
        frag_pack(w.data(), cout, cin, taps, cin_pad, ntiles, groups, out.data());
        for (int nt = 0; nt < ntiles; ++nt)
            for (int q = 0; q < groups; ++q)
                for (int l = 0; l < 64; ++l)
                    for (int e = 0; e < 4; ++e) {
                        const float want = dense[(size_t)(32 * nt + (l & 31)) * K + 8 * q + 4 * (l >> 5) + e];
                        if (out[(((size_t)nt * groups + q) * 64 + l) * 4 + e] != want) {
                            printf("case cout=%d cin=%d taps=%d: mismatch at tile %d group %d lane %d element %d\n", cout, cin, taps,
                                   nt, q, l, e);
                            return 1;
                        }
                    }
    }
    printf("frag_harness: 5 cases ok\n");
    return 0;
}
#endif
