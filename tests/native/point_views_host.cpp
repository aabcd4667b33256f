// Host build of m3p2i_aip_amd/csrc/point_views.hpp (the conversions between the point_env SoA world's (cos yaw, sin yaw) and
// the views' quaternion) for tests/test_point_views_cpu.py: the device source, one call per case.
#include "../../m3p2i_aip_amd/csrc/point_views.hpp"

extern "C" {
// rows: [n][13], filled by the caller; in: [n][7] = x, y, c, s, vx, vy, w
void pv_write_body13(int n, const float* in, float* rows) {
    for (int i = 0; i < n; ++i) {
        const float* a = in + (long)i * 7;
        m3::write_body13(rows + (long)i * 13, a[0], a[1], a[2], a[3], a[4], a[5], a[6]);
    }
}
// q: [n][2] = qz, qw; cs: [n][2]
void pv_yaw_from_quat(int n, const float* q, float* cs) {
    for (int i = 0; i < n; ++i) m3::yaw_from_quat(q[2 * i], q[2 * i + 1], &cs[2 * i], &cs[2 * i + 1]);
}
}
