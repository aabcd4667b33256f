"""The inputs of the wavefront-order tests, generated in one place: the GPU tests (test_wave_order_gpu.py) run them on the
device, the CPU tests (test_wave_order_cpu.py) show on the same inputs that the float64 reference meets its own bound.

Noise: the planner's own Halton-spline sampler (sampling.halton_spline_delta), sigma_diag (3, 3).
Scenes (positions of box, dyn-obs; the obstacle stays at the arena's default (2, 2)):
  row      box (0, 2), dyn-obs (-2, 2): the reference's scene, all three in a row along x -- axis th = 0
  oblique  box (1, -1), dyn-obs (-2, -3): cxx = 78/9, cyy = 114/9, cxy = 87/9, so 2 cxy = 19.3 and cxx - cyy = -4.0 are
           both far from 0 and the branch of atan2 is not a matter of rounding; th = 0.887 rad
  bound    box (-1, 1), dyn-obs (1.5, -2.5), read from the bound simulator's root tensor (the handle's own world keeps
           the row scene): 2 cxy = -2.33, cxx - cyy = -6.0; th = -1.385 rad
"""
import functools

import numpy as np

SIGMA = (3.0, 3.0)
OBSTACLE = (2.0, 2.0)      # _lib.POINT_SCENE_DEFAULTS obs_x, obs_y
SCENES = {
    "row": dict(box=(0.0, 2.0), dyn=(-2.0, 2.0)),
    "oblique": dict(box=(1.0, -1.0), dyn=(-2.0, -3.0)),
    "bound": dict(box=(-1.0, 1.0), dyn=(1.5, -2.5)),
}
# name -> K_global, T, multi-modal, scene; blocks = (k_offset, K_local) of every shard that is ordered
CASES = {
    "single_K128": dict(K=128, T=12, mm=False, scene="row"),
    "single_K200": dict(K=200, T=12, mm=False, scene="row"),            # ragged last wavefront
    "multi_K256": dict(K=256, T=12, mm=True, scene="row"),              # two wavefronts per mode
    "multi_K512_T30": dict(K=512, T=30, mm=True, scene="row"),
    "oblique_single_K200": dict(K=200, T=12, mm=False, scene="oblique"),
    "oblique_multi_K256": dict(K=256, T=12, mm=True, scene="oblique"),
    "bound_single_K200": dict(K=200, T=12, mm=False, scene="bound"),
    "bound_multi_K256": dict(K=256, T=12, mm=True, scene="bound"),
    "shards_K512": dict(K=512, T=12, mm=True, scene="row", blocks=((0, 256), (256, 256))),
}


@functools.lru_cache(maxsize=None)
def _delta(K, T):
    from m3p2i_aip_amd import sampling
    d = sampling.halton_spline_delta(K, T, 2, workers=1).numpy()
    d.setflags(write=False)
    return d


def case(name):
    """dict(K, T, mm, box, dyn, obs, blocks, delta[K, T, 2] float32 (read-only, shared))"""
    c = dict(CASES[name])
    c.update(SCENES[c["scene"]], obs=OBSTACLE, delta=_delta(c["K"], c["T"]))
    c.setdefault("blocks", ((0, c["K"]),))
    return c


def world_raw(c, robot=(0.0, 1.5)):
    """the library's 18 floats: robot x y vx vy | box x y cos sin vx vy w | dyn-obs likewise"""
    return np.array([robot[0], robot[1], 0, 0, c["box"][0], c["box"][1], 1, 0, 0, 0, 0,
                     c["dyn"][0], c["dyn"][1], 1, 0, 0, 0, 0], np.float32)


def block_keys(c, k_offset, K_local):
    """(float64 keys of the block's samples, the bound that goes with them)"""
    from tests import wave_order_ref as R
    keys, M = R.keys64(c["delta"][k_offset:k_offset + K_local], SIGMA, c["box"], c["dyn"], c["obs"])
    return keys, R.tol(c["T"], M)
