// panda_episode_tables.hpp -- the two workspace tables of a lockstep panda_env episode set created with
// M3_PANDA_EPISODES_RUNTIME (m3_panda_episodes_create_ex): the planning side, row e the workspace planner
// e's own simulator steps its row 0 in, and the world side, row e the workspace of row e of the world.  Layout and content are
// those of panda_scene_rows.hpp -- word-major [PANDA_SCENE_ROW_WORDS][n], each row make_panda_scene_rt of its workspace formed
// here on the host, nothing derived on the device.  Host only, no HIP call: m3_api.hip refreshes the pinned mirrors with it,
// tests/native/panda_episode_tables_host.cpp builds it on its own.
#pragma once
#include "panda_scene.hpp"
#include "panda_scene_rows.hpp"

#include <cstring>

namespace m3 {

// Brings `table` (n rows) up to the workspaces scene_of(0 .. n - 1): a row whose 21 floats equal what `kept` holds of it, bit for
// bit, stays as it is (`all`: every row is packed; the first fill).  Returns the number of rows packed -- 0: the device copy
// is current, nothing to upload.  No allocation.
template <class SceneOf>
inline int panda_episode_table_refresh(float* table, m3_panda_scene* kept, bool all, int n, float dt, int substeps, SceneOf&& scene_of) {
    int packed = 0;
    for (int e = 0; e < n; ++e) {
        const m3_panda_scene& ws = scene_of(e);
        if (!all && std::memcmp(&kept[e], &ws, sizeof(ws)) == 0) continue;
        std::memcpy(&kept[e], &ws, sizeof(ws));
        panda_scene_row_pack(make_panda_scene_rt(ws, dt, substeps), table, n, e);
        ++packed;
    }
    return packed;
}

}  // namespace m3
