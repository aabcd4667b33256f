// point_views.hpp -- the two conversions between the point_env SoA world and the wrapper's views, each written once: a body's
// orientation is (cos yaw, sin yaw) in the world and the Isaac Gym quaternion (0, 0, qz, qw) = (0, 0, sin(yaw/2), cos(yaw/2))
// in the 13-float rows of root_state / rigid_body_state.  Needs <hip/hip_runtime.h> for the function attributes only, so the
// host compiler builds it through tests/native/shim (tests/native/point_views_host.cpp, tests/test_point_views_cpu.py).
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>

namespace m3 {

// views -> world: yaw of the (0, 0, qz, qw) quaternion.  Well conditioned everywhere (products of the components only).
// Used by pull_env (rollout_point.hip), load_world_from_sim (rollout_point_kernel.hpp) and m3_set_world_point (m3_api.hip, on
// the host); the expression and its parentheses are part of the bit-exact pull-side tests.
__host__ __device__ __forceinline__ void yaw_from_quat(float qz, float qw, float* c, float* s) {
    *c = 1.0f - 2.0f * (qz * qz);
    *s = 2.0f * (qz * qw);
}

// world -> views: yaw (c, s) -> quaternion with qw = cos(yaw/2) >= 0.  The half-angle formulas give one component as
// sqrt(0.5 (1 + |c|)) >= 0.707 and the other as s over twice that: the LARGER component is the one under the root, so no
// cancellation enters the divisor -- cos(yaw/2) for c >= 0, |sin(yaw/2)| for c < 0 (where 1 + c cancels as yaw -> +-pi and
// the quotient s / (2 sqrt(0.5 (1 + c))) of two small noisy numbers was wrong by up to 2 in a component).  For c >= 0 these
// are the bits of the form this replaces.  At c = -1, s = +-0: qz = +-1, qw = 0.
__device__ __forceinline__ void quat_from_yaw(float c, float s, float* qz, float* qw) {
    const bool back = c < 0.0f;
    const float big = sqrtf(0.5f * (1.0f + fabsf(c)));
    const float small = (back ? fabsf(s) : s) / (2.0f * big);
    *qz = back ? copysignf(big, s) : small;
    *qw = back ? small : big;
}

// one 13-float row: pos3 quat4(xyzw) linvel3 angvel3 (isaacgym_wrapper.py:102-104)
__device__ __forceinline__ void write_body13(float* r, float x, float y, float c, float s,
                                             float vx, float vy, float wz) {
    float qz, qw;
    quat_from_yaw(c, s, &qz, &qw);
    r[0] = x; r[1] = y;  // r[2] (z) is left as set at init
    r[3] = 0.0f; r[4] = 0.0f; r[5] = qz; r[6] = qw;
    r[7] = vx; r[8] = vy; r[9] = 0.0f;
    r[10] = 0.0f; r[11] = 0.0f; r[12] = wz;
}

}  // namespace m3
