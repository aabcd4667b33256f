// Host build of csrc/planar_dyn.hpp for tests/test_lean_substep_rows_cpu.py: the three lean instances of point_substep
// called DIRECTLY, one lane per "wavefront" -- and, on request, as a lane of a wavefront whose OTHER lanes have every row:
// each ballot then also reports a lane that is not this one, so the substep takes its most general pass version and this
// lane's rows are switched by their per-lane flags alone (the merge a one-lane wavefront never reaches, because there the
// wave-uniform version and the lane's own flag are the same thing).
#include <hip/hip_runtime.h>   // (the shim of tests/native/shim)
static unsigned long long g_other_lanes = 0ull;
#undef __builtin_amdgcn_ballot_w64
#define __builtin_amdgcn_ballot_w64(p) (((p) ? 1ull : 0ull) | g_other_lanes)
#include "../../m3p2i_aip_amd/csrc/planar_dyn.hpp"

namespace {
void load(const float* w, m3::PointWorld& p) {   // oracle row (31 floats), as in planar_dyn_host.cpp
    p.rx = w[0]; p.ry = w[1]; p.rvx = w[4]; p.rvy = w[5];
    p.B = {w[7], w[8], w[9], w[10], w[11], w[12], w[13]};
    p.D = {w[14], w[15], w[16], w[17], w[18], w[19], w[20]};
    p.fRx = w[21]; p.fRy = w[22]; p.fBx = w[23]; p.fBy = w[24];
    p.fcRx = w[25]; p.fcRy = w[26]; p.fcBx = w[27]; p.fcBy = w[28]; p.fcDx = w[29]; p.fcDy = w[30];
}
void store(const m3::PointWorld& p, float* w) {
    w[0] = p.rx; w[1] = p.ry; w[4] = p.rvx; w[5] = p.rvy;
    const m3::Box* b[2] = {&p.B, &p.D};
    for (int i = 0; i < 2; ++i) {
        float* o = w + 7 + 7 * i;
        o[0] = b[i]->x; o[1] = b[i]->y; o[2] = b[i]->c; o[3] = b[i]->s; o[4] = b[i]->vx; o[5] = b[i]->vy; o[6] = b[i]->w;
    }
    w[21] = p.fRx; w[22] = p.fRy; w[23] = p.fBx; w[24] = p.fBy;
    w[29] = p.fcDx; w[30] = p.fcDy;
}
// this lane's own pair-group mask (the predicates of point_step's broad phase, without the ballots)
unsigned lane_mask(const m3::PointScene& sc, const m3::PointWorld& w) {
    using namespace m3;
    unsigned m = 0u;
    if (near_centres(sc, w.B.x, w.B.y, w.rx, w.ry, sc.robot_r, sc.rad_b)) m |= G_RB;
    if (near_centres(sc, w.D.x, w.D.y, w.rx, w.ry, sc.robot_r, sc.rad_d)) m |= G_RD;
    if (near_centres(sc, sc.obs_x, sc.obs_y, w.rx, w.ry, sc.robot_r, sc.rad_o)) m |= G_RO;
    if (near_walls_disc(sc, w.rx, w.ry)) m |= G_RW;
    if (near_walls_box(sc, w.B, sc.rad_b)) m |= G_BW;
    if (near_walls_box(sc, w.D, sc.rad_d)) m |= G_DW;
    if (near_centres(sc, w.B.x, w.B.y, w.D.x, w.D.y, sc.rad_b, sc.rad_d)) m |= G_BD;
    if (near_centres(sc, w.B.x, w.B.y, sc.obs_x, sc.obs_y, sc.rad_b, sc.rad_o)) m |= G_BO;
    if (near_centres(sc, w.D.x, w.D.y, sc.obs_x, sc.obs_y, sc.rad_d, sc.rad_o)) m |= G_DO;
    return m;
}
}  // namespace

// One world (a row of 31 floats, the oracle's layout) through one step with control (ux, uy): every substep runs the
// leanest of the three lean instances {0, G_RB, G_RB | G_RD} that is at least `min_instance` (0, 1, 2 in that order) and
// covers the lane's mask.  other_lanes != 0: as a lane of a wavefront whose other lanes have every row (above).
// info[2 * sub] = the lane's mask, info[2 * sub + 1] = the instance that ran.  Returns 0, or -1 if a substep's mask is
// not covered by any lean instance (the world is then left as it was before that substep).
extern "C" int pss_step(float dt, int substeps, int iters, float* world, float ux, float uy, int min_instance,
                        int other_lanes, int* info) {
    using namespace m3;
    PointScene sc;
    make_point_scene(sc, dt, substeps, iters);
    PointWorld p;
    load(world, p);
    g_other_lanes = other_lanes ? 2ull : 0ull;
    int rc = 0;
    for (int sub = 0; sub < substeps; ++sub) {
        const bool form = sub == substeps - 1;
        const unsigned m = lane_mask(sc, p);
        int inst = min_instance;
        if (inst < 1 && m != 0u) inst = 1;
        if (inst < 2 && (m & ~G_RB) != 0u) inst = 2;
        info[2 * sub] = (int)m; info[2 * sub + 1] = inst;
        if ((m & ~(G_RB | G_RD)) != 0u) { rc = -1; break; }
        if (inst == 0) point_substep<false, 0u>(sc, p, ux, uy, form);
        else if (inst == 1) point_substep<false, G_RB>(sc, p, ux, uy, form);
        else point_substep<false, G_RB | G_RD>(sc, p, ux, uy, form);
    }
    g_other_lanes = 0ull;
    store(p, world);
    return rc;
}
