// Host build of the product's noise_stream.hpp for the CPU test (tests/test_noise_stream_cpu.py): the header the rollout
// kernels and k_sample_noise compile, by g++ over the shim (test infrastructure, not product code).
//   g++ -O2 -std=c++17 -shared -fPIC -ffp-contract=off -fno-fast-math -Ishim noise_stream_host.cpp -o libnoise_stream_host.so
#include <hip/hip_runtime.h>
#include "../../m3p2i_aip_amd/csrc/noise_stream.hpp"

// The header's splitmix64 and xoshiro128++ under a COPY of gauss_pair's key line (the header does not expose the integers):
// this pins the two generators, not the key.  The key the kernels compile is pinned through nsh_gauss_pair's values at the
// same corners (test_header_key_at_the_corners_through_gauss_pair).
static void raw_pair(unsigned long long seed, unsigned call, unsigned k, unsigned t, unsigned pair, unsigned& r0, unsigned& r1) {
    unsigned long long x = seed ^ (0xD1B54A32D192ED03ULL * (unsigned long long)(call + 1u));
    x ^= ((unsigned long long)k << 32) | ((unsigned long long)t << 8) | (unsigned long long)pair;
    const unsigned long long a = m3::splitmix64(x), b = m3::splitmix64(x);
    unsigned s[4] = {(unsigned)a, (unsigned)(a >> 32), (unsigned)b, (unsigned)(b >> 32)};
    r0 = m3::xoshiro128pp(s);
    r1 = m3::xoshiro128pp(s);
}

// n tuples (call, k, t, pair) -> z0[n], z1[n]
extern "C" void nsh_gauss_pair(unsigned long long seed, long long n, const unsigned* call, const unsigned* k, const unsigned* t,
                               const unsigned* pair, float* z0, float* z1) {
    for (long long i = 0; i < n; ++i) m3::gauss_pair(seed, call[i], k[i], t[i], pair[i], z0[i], z1[i]);
}
extern "C" void nsh_raw(unsigned long long seed, long long n, const unsigned* call, const unsigned* k, const unsigned* t,
                        const unsigned* pair, unsigned* r0, unsigned* r1) {
    for (long long i = 0; i < n; ++i) raw_pair(seed, call[i], k[i], t[i], pair[i], r0[i], r1[i]);
}
// the whole standard-normal table of one call, z[T][K][2 * npair] for k in [k0, k0 + K) (the layout of m3_sample_noise)
extern "C" void nsh_gauss_table(unsigned long long seed, unsigned call, unsigned k0, int K, int T, int npair, float* z) {
    for (int t = 0; t < T; ++t)
        for (int i = 0; i < K; ++i)
            for (int p = 0; p < npair; ++p) {
                float* o = z + (((long long)t * K + i) * npair + p) * 2;
                m3::gauss_pair(seed, call, k0 + (unsigned)i, (unsigned)t, (unsigned)p, o[0], o[1]);
            }
}
