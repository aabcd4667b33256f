// spline_fit.hpp at the bounds of its fixed arrays, stand-alone (tests/test_spline_fit_bounds_cpu.py builds this plain and
// with -fsanitize=address,undefined and compares the two outputs):
//   g++ -O1 -g -std=c++17 -ffp-contract=off -I m3p2i_aip_amd/csrc spline_fit_check.cpp -o spline_fit_check
// Every (m, k, s) with k in {1, 2, 3}, m in {k + 1, 63, 64} and s in {0, 0.5, 1e6} -- m = 64 with k = 3 puts t, c, z, fpint,
// nrdata, a, g, b and q at their declared sizes -- on the eleven fixed series of tests/spline_edge_series.py and 300 random
// ones; one checksum line per combination.  Then the refused arguments: -1 and `out` untouched.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>

#include "spline_fit.hpp"

static uint64_t lcg_state = 0x9E3779B97F4A7C15ull;
static double lcg_uniform() {   // (0, 1)
    lcg_state = lcg_state * 6364136223846793005ull + 1442695040888963407ull;
    return ((double)(lcg_state >> 11) + 0.5) * (1.0 / 9007199254740992.0);
}
static double lcg_normal() {    // Box-Muller
    const double u1 = lcg_uniform(), u2 = lcg_uniform();
    return std::sqrt(-2.0 * std::log(u1)) * std::cos(6.283185307179586 * u2);
}

static const int N_FIXED = 11, N_RANDOM = 300, MAX_OUT = 256;

// series r of m points (float values, as the device's knots are)
static void make_series(int r, int m, double* y) {
    for (int i = 0; i < m; ++i) {
        const double nrm = lcg_normal(), alt = (i % 2 == 0) ? 1.0 : -1.0;
        double v;
        switch (r) {
            case 0: v = 0.0; break;
            case 1: v = (double)i; break;
            case 2: v = nrm * 1e-3; break;
            case 3: v = nrm * 30.0; break;
            case 4: v = 7.5; break;
            case 5: v = 3.0 * alt; break;
            case 6: v = (i == m / 2) ? 50.0 : 0.0; break;
            case 7: v = (i < m / 2) ? -4.0 : 4.0; break;
            case 8: v = nrm * 1e4; break;
            case 9: v = nrm * 1e-20; break;
            case 10: v = std::sqrt(0.5 / m) * alt; break;
            default: v = nrm;
        }
        y[i] = (double)(float)v;
    }
}

static uint64_t mix(uint64_t h, uint64_t v) { return (h ^ v) * 0x100000001B3ull; }   // FNV-1a over 64-bit words

static int fails = 0;
static void expect(bool ok, const char* what, int m, int k, int n_out) {
    if (!ok) { std::printf("FAIL %s (m = %d, k = %d, n_out = %d)\n", what, m, k, n_out); ++fails; }
}

static void refused(int m, int k, int n_out) {
    double y[m3::SF_MAX_M + 2];
    for (int i = 0; i < m3::SF_MAX_M + 2; ++i) y[i] = 0.25 * i;
    float out[MAX_OUT];
    const float sentinel = -12345.5f;
    for (int i = 0; i < MAX_OUT; ++i) out[i] = sentinel;
    const int rc = m3::spline_fit_eval<float>(y, m, k, 0.5, n_out, out, 1);
    expect(rc == -1, "a refused argument must return -1", m, k, n_out);
    bool untouched = true;
    for (int i = 0; i < MAX_OUT; ++i) untouched = untouched && out[i] == sentinel;
    expect(untouched, "a refused call must not write", m, k, n_out);
}

int main() {
    const double smoothings[3] = {0.0, 0.5, 1e6};
    for (int k = 1; k <= 3; ++k) {
        const int ms[3] = {k + 1, 63, 64};
        for (int mi = 0; mi < 3; ++mi)
            for (int si = 0; si < 3; ++si) {
                const int m = ms[mi], n_out = (m < 16) ? 4 * m : MAX_OUT;
                const double s = smoothings[si];
                uint64_t h = 0xCBF29CE484222325ull;
                int n_min = 1 << 30, n_max = 0;
                for (int r = 0; r < N_FIXED + N_RANDOM; ++r) {
                    double y[m3::SF_MAX_M];
                    make_series(r, m, y);
                    // two guard elements on each side of the strided output: stride 2, n_out values
                    float out[2 * MAX_OUT + 4];
                    for (int i = 0; i < 2 * MAX_OUT + 4; ++i) out[i] = -777.0f;
                    const int n = m3::spline_fit_eval<float>(y, m, k, s, n_out, out + 2, 2);
                    expect(n >= 2 * k + 2 && n <= m + k + 1, "knot count out of range", m, k, n_out);
                    bool clean = out[0] == -777.0f && out[1] == -777.0f;
                    for (int i = 0; i < n_out; ++i) {
                        uint32_t bits;
                        std::memcpy(&bits, &out[2 + 2 * i], 4);
                        h = mix(h, bits);
                        expect(std::isfinite(out[2 + 2 * i]), "non-finite value", m, k, r);
                        if (i + 1 < n_out) clean = clean && out[3 + 2 * i] == -777.0f;     // between the strided values
                    }
                    for (int i = 2 + 2 * (n_out - 1) + 1; i < 2 * MAX_OUT + 4; ++i) clean = clean && out[i] == -777.0f;
                    expect(clean, "wrote outside its strided output", m, k, r);
                    h = mix(h, (uint64_t)n);
                    if (n < n_min) n_min = n;
                    if (n > n_max) n_max = n;
                }
                std::printf("k=%d m=%2d s=%-7g n_out=%3d knots %2d..%2d checksum %016llx\n", k, m, s, n_out, n_min, n_max,
                            (unsigned long long)h);
            }
    }
    for (int k = 1; k <= 3; ++k) {
        refused(65, k, 16);      // more points than SF_MAX_M
        refused(k, k, 16);       // m > k must hold
        refused(8, k, 0);        // nothing to evaluate
    }
    refused(8, 0, 16);
    refused(8, 4, 16);
    if (fails) return 1;
    std::printf("spline_fit_check: ok\n");
    return 0;
}
