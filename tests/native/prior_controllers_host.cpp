// Host build of m3p2i_aip_amd/csrc/prior_controllers.hpp -- the arithmetic k_prior_controllers runs, compiled by g++ with
// contraction off: tests/test_prior_controllers_cpu.py holds it to priors.go_to / priors.push_behind (float64) within a derived
// bound, tests/test_prior_controllers_gpu.py holds the kernel's table to it bit for bit.  A program of its own (it also runs
// under -fsanitize=address,undefined).
//
// stdin: one case per line, every float as the 8 hex digits of its binary32 bits:
//     kind n T dt u_max0 u_max1 standoff reach rx ry bx by gx gy factor_0 .. factor_{n-1}
// stdout: per case one line of n * T * 2 words, the table rows [n][T][2] as the kernel lays them out.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../m3p2i_aip_amd/csrc/prior_controllers.hpp"

static bool read_float(float& v) {
    unsigned w;
    if (std::scanf("%x", &w) != 1) return false;
    const std::uint32_t bits = w;
    std::memcpy(&v, &bits, sizeof(v));
    return true;
}

int main() {
    int kind, n, T;
    while (std::scanf("%d %d %d", &kind, &n, &T) == 3) {
        if (n < 1 || n > 16 || T < 1 || T > 4096) return 2;
        float in[11];   // dt u_max0 u_max1 standoff reach rx ry bx by gx gy
        for (float& v : in)
            if (!read_float(v)) return 2;
        std::vector<float> factor((size_t)n), tab((size_t)n * T * 2);
        for (float& f : factor)
            if (!read_float(f)) return 2;
        for (int j = 0; j < n; ++j) {
            float* row = tab.data() + (size_t)j * T * 2;
            const float speed = m3::prior_controller_speed(factor[(size_t)j], in[1], in[2]);
            m3::prior_controller_sequence(kind, in[5], in[6], in[7], in[8], in[9], in[10], T, in[0], speed, in[3], in[4],
                                          [row](int t, float ux, float uy) { row[2 * t] = ux; row[2 * t + 1] = uy; });
        }
        for (size_t i = 0; i < tab.size(); ++i) {
            std::uint32_t bits;
            std::memcpy(&bits, &tab[i], sizeof(bits));
            std::printf("%08x%c", (unsigned)bits, i + 1 == tab.size() ? '\n' : ' ');
        }
    }
    return 0;
}
