"""HipEngine: thin object over one ``m3_handle`` of libm3p2i_hip.so.

PyTorch is plumbing here: it provides the HIP stream and wraps the library-owned device
buffers as zero-copy tensors (``__cuda_array_interface__``).  All arithmetic of the hot
path happens inside the HIP kernels.
"""
from __future__ import annotations

import collections
import os

import ctypes as C

import numpy as np
import torch

from . import _lib as L


class _DevArray:
    """Minimal __cuda_array_interface__ carrier for a library-owned device pointer."""

    def __init__(self, ptr, shape, typestr, owner):
        self.__cuda_array_interface__ = {"shape": tuple(shape), "typestr": typestr,
                                         "data": (int(ptr), False), "version": 2}
        self._owner = owner  # keeps the handle alive while views exist


def make_config(K, T, nu=2, env_type="point_env", multi_modal=False, mode_simple=False,
                sampling_random=False, sample_null_action=True, filter_u=True,
                u_per_command=None, u_min=None, u_max=None, noise_sigma_diag=None, u_scale=1.0,
                gamma=0.95, lambda_=1.0, kp_suction=400.0, pre_height_diff=0.05, dt=None,
                substeps=2, solver_iters=6, seed=0, device=0, K_local=None, k_offset=0,
                cube_on_shelf=False, sim_only=False, shard_mix=False, noise_mu=None, noise_sigma=None,
                noise_abs_cost=False, update_cov=False) -> L.Config:
    """noise_sigma: the full [nu][nu] matrix (sets noise_sigma_diag too; full_sigma when it has off-diagonal
    entries)."""
    lib = L.load()
    c = L.Config()
    env = L.ENV_POINT if env_type in ("point_env", 0) else L.ENV_PANDA
    lib.m3_default_config(C.byref(c), env)
    c.device = int(device)
    c.K_global = int(K)
    c.K_local = int(K if K_local is None else K_local)
    c.k_offset = int(k_offset)
    c.T, c.nu = int(T), int(nu)
    c.multi_modal = int(bool(multi_modal))
    c.mode_simple = int(bool(mode_simple))
    c.sampling_random = int(bool(sampling_random))
    c.sample_null_action = int(bool(sample_null_action))
    c.filter_u = int(bool(filter_u))
    c.u_per_command = int(T if u_per_command is None else u_per_command)
    for name, vals in (("u_min", u_min), ("u_max", u_max), ("noise_sigma_diag", noise_sigma_diag)):
        if vals is not None:
            arr = getattr(c, name)
            for j in range(nu):
                arr[j] = float(vals[j])
    c.u_scale, c.gamma, c.lambda_ = float(u_scale), float(gamma), float(lambda_)
    c.kp_suction, c.pre_height_diff = float(kp_suction), float(pre_height_diff)
    if dt is not None:
        c.dt = float(dt)
    c.substeps, c.solver_iters = int(substeps), int(solver_iters)
    c.cube_on_shelf = int(bool(cube_on_shelf))
    c.sim_only = int(bool(sim_only))
    if noise_sigma is not None:
        for i in range(nu):
            c.noise_sigma_diag[i] = float(noise_sigma[i][i])
            for j in range(nu):
                c.noise_sigma_full[i * nu + j] = float(noise_sigma[i][j])
                if i != j and float(noise_sigma[i][j]) != 0.0:
                    c.full_sigma = 1
    if noise_mu is not None:
        for j in range(nu):
            c.noise_mu[j] = float(noise_mu[j])
    c.noise_abs_cost, c.update_cov = int(bool(noise_abs_cost)), int(bool(update_cov))
    c.shard_mix = int(shard_mix)   # 0: gather + reduce; 1 (True): one collective; 2: ... with ladder tables (multi-modal);
                                   # 3: two small exchanges, O(K_local) work per rank (multi-modal)
    c.seed = int(seed)
    return c


class _CObject:
    """The lifetime and error reporting of one C object of the library.  A subclass names the attribute that holds its pointer
    and the library's destroy and last-error functions; the pointer is null until its create call succeeded and after close()."""
    _ptr = _destroy = _last_error = None

    def close(self):
        p = getattr(self, self._ptr, None)
        if p is not None and p:
            getattr(self.lib, self._destroy)(p)
            setattr(self, self._ptr, C.c_void_p())

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _ck(self, rc):
        if rc != 0:
            msg = getattr(self.lib, self._last_error)(getattr(self, self._ptr))   # (a null pointer: the create call's error)
            raise L.M3Error(f"m3p2i_hip error {rc}: {msg.decode() if msg else ''}")


def _point_scene_fields(fields, where=""):
    """PointSceneFields from field overrides over _lib.POINT_SCENE_DEFAULTS (None: the reference's arena)"""
    fields = dict(fields or {})
    unknown = sorted(set(fields) - set(L.POINT_SCENE_DEFAULTS))
    if unknown:
        raise ValueError(f"{where}unknown point scene field(s) {unknown}: one of {list(L.POINT_SCENE_DEFAULTS)}")
    return L.PointSceneFields(**{**L.POINT_SCENE_DEFAULTS, **{k: float(v) for k, v in fields.items()}})


def _point_scene_dict(sc):
    return {n: getattr(sc, n) for n in L.POINT_SCENE_DEFAULTS}


# A kind of scene rows, the point_env arena or the panda_env workspace: the C struct, row i's mapping -> struct (ValueError for an
# unknown field), struct -> mapping, and the C (setter, getter) per environment of a sim_only engine and per sample of a planner.
_SceneKind = collections.namedtuple("_SceneKind", "struct from_row to_dict env_rows sample_rows")
_POINT_ROWS = _SceneKind(L.PointSceneFields, lambda i, fields: _point_scene_fields(fields, f"row {i}: "), _point_scene_dict,
                         ("m3_set_point_scene_rows", "m3_get_point_scene_row"),
                         ("m3_set_point_rollout_scenes", "m3_get_point_rollout_scene"))
_PANDA_ROWS = _SceneKind(L.PandaSceneFields, lambda i, fields: L.panda_scene_fields(fields), L.panda_scene_dict,
                         ("m3_set_panda_scene_rows", "m3_get_panda_scene_row"),
                         ("m3_set_panda_rollout_scenes", "m3_get_panda_rollout_scene"))


class HipEngine(_CObject):
    _ptr, _destroy, _last_error = "_h", "m3_destroy", "m3_last_error"

    def __init__(self, cfg: L.Config):
        if not torch.cuda.is_available():
            raise L.M3Error("HipEngine needs a HIP device (torch.cuda.is_available() is False); "
                            "there is no CPU fallback")
        self.lib = L.load()
        self.cfg = cfg
        self._h = C.c_void_p()
        torch.cuda.set_device(cfg.device)
        torch.zeros(1, device=f"cuda:{cfg.device}")  # make sure the HIP context exists
        self._ck(self.lib.m3_create(C.byref(cfg), C.byref(self._h)))
        self.device = torch.device(f"cuda:{cfg.device}")
        self._views = {}
        self._action_out = None
        self.use_torch_stream()
        if os.environ.get("M3P2I_WAVE_ORDER", "1") == "0":   # experiments (tools/): samples to wavefronts by index
            self.set_wave_order(False)
        if os.environ.get("M3P2I_ROLLOUT_LANES"):            # experiments (tools/panda_lanes_sweep.py)
            self.set_rollout_lanes(int(os.environ["M3P2I_ROLLOUT_LANES"]))
        if os.environ.get("M3P2I_POINT_ROLLOUT_FORM"):       # experiments (tools/fuzz_parity.py, A/B runs)
            self.set_point_rollout_form(int(os.environ["M3P2I_POINT_ROLLOUT_FORM"]))

    # ---- lifetime ----
    def close(self):
        getattr(self, "_views", {}).clear()
        super().close()

    # ---- configuration ----
    def use_torch_stream(self, stream=None):
        s = stream if stream is not None else torch.cuda.current_stream(self.device)
        self._ck(self.lib.m3_set_stream(self._h, C.c_void_p(s.cuda_stream)))

    def set_rollout_lanes(self, lanes=0):
        self._ck(self.lib.m3_set_rollout_lanes(self._h, int(lanes)))

    def set_point_rollout_form(self, form=-1):
        """point_env rollout of navigation / push: 0 = one wavefront per 64 samples, 1 = dynamics + companion wavefront wherever
        that form exists, -1 = automatic; same results bit for bit."""
        self._ck(self.lib.m3_set_point_rollout_form(self._h, int(form)))

    def point_rollout_form_used(self):
        """The form of the last rollout launch (0, 1; -1 before the first)."""
        return int(self.lib.m3_point_rollout_form_used(self._h))

    def set_panda_lanes_per_sample(self, lps=0):
        """panda_env rollout: 1 = a lane per sample, 16 = the sixteen lanes of a DPP row share a sample (the contact rows run
        across them), 0 = by size; same results bit for bit."""
        self._ck(self.lib.m3_set_panda_lanes_per_sample(self._h, int(lps)))

    def panda_lanes_per_sample_used(self):
        """The form the last panda rollout ran in (automatic choice: by size; for reach, by whether the last commands' rollouts
        brought the gripper within reach of a box)."""
        return int(self.lib.m3_panda_lanes_per_sample_used(self._h))

    def set_panda_reach_cost_kernel(self, on=True):
        """reach, unsharded, K <= 8192, default sampler: the cost in a kernel of its own behind a rollout without shadow slots
        (default) or the shadow slots; same bits."""
        self._ck(self.lib.m3_set_panda_reach_cost_kernel(self._h, int(bool(on))))

    def panda_near_share(self):
        """1/1000 of the last finished panda rollout's (sample, substep) pairs with the gripper within reach of a box (-1: none yet)."""
        return int(self.lib.m3_panda_near_share(self._h))

    def set_update_launches(self, launches=0):
        """0 / 3: the three-launch multi-modal update beyond k_update_small's range; 5: round 3's five launches."""
        self._ck(self.lib.m3_set_update_launches(self._h, int(launches)))

    def set_ladder_spins(self, spins=-1):
        """Bound of the multi-modal update's in-launch waits: -1 default, 0 = every workgroup takes the give-up branch."""
        self._ck(self.lib.m3_set_ladder_spins(self._h, int(spins)))

    def set_wave_order(self, on=True):
        """Samples sorted into coherent wavefronts (default) or assigned by index; same results."""
        self._ck(self.lib.m3_set_wave_order(self._h, int(bool(on))))

    def wave_order(self):
        """The wavefront order the last rollout went by: int32 tensor [K_local] (a copy; slot -> local sample index), or None
        when it went by index (order off, relabelled, K_local < 128, random sampling, simple mode, noise churn, panda)."""
        p, n = C.c_void_p(), C.c_int()
        self._ck(self.lib.m3_wave_order(self._h, C.byref(p), C.byref(n)))
        if not p.value:
            return None
        return torch.as_tensor(_DevArray(p.value, (n.value,), "<i4", self), device=self.device).clone()

    def relabel_samples(self):
        """Permute the noise rows once into wavefront order (labels of a generated sample set carry
        no meaning): same sample set, coalesced stores.  See include/m3p2i_hip.h."""
        self._ck(self.lib.m3_relabel_samples(self._h))

    def enable_timing(self, on=True):
        self._ck(self.lib.m3_enable_timing(self._h, int(on)))

    @property
    def needs_global_noise(self):
        """One-collective multi-modal shard: the noise rows of ALL K_global samples live on every rank."""
        c = self.cfg
        return bool(c.shard_mix and c.K_local != c.K_global and c.multi_modal and not c.mode_simple)

    def set_noise(self, delta):
        """delta: [K_local, T, nu] (reference layout), torch (cpu/cuda) or numpy -- [K_global, T, nu] for a
        handle with `needs_global_noise`."""
        c = self.cfg
        rows, fn = (c.K_global, self.lib.m3_set_noise_global) if self.needs_global_noise else (c.K_local, self.lib.m3_set_noise)
        if isinstance(delta, torch.Tensor) and delta.is_cuda:
            d = delta.to(torch.float32).contiguous()
            assert tuple(d.shape) == (rows, c.T, c.nu), d.shape
            self._ck(fn(self._h, d.data_ptr(), 1))
            torch.cuda.current_stream(self.device).synchronize()
        else:
            d = np.ascontiguousarray(delta.cpu().numpy() if isinstance(delta, torch.Tensor)
                                     else delta, dtype=np.float32)
            assert d.shape == (rows, c.T, c.nu), d.shape
            self._ck(fn(self._h, d.ctypes.data, 0))

    def set_noise_knots(self, knots, degree=2, smoothing=0.5):
        """Halton-spline sampler on the device: knots [K_local, nu, n_knots] (Gaussian Halton values
        of this shard's samples; [K_global, ...] with `needs_global_noise`) -> smoothing-spline noise in
        the library's noise buffer."""
        c = self.cfg
        rows, fn = (c.K_global, self.lib.m3_set_noise_knots_global) if self.needs_global_noise \
            else (c.K_local, self.lib.m3_set_noise_knots)
        k = np.ascontiguousarray(knots.detach().cpu().numpy() if isinstance(knots, torch.Tensor) else knots,
                                 dtype=np.float32)
        assert k.ndim == 3 and k.shape[:2] == (rows, c.nu), k.shape
        self._ck(fn(self._h, k.ctypes.data, int(k.shape[2]), int(degree), float(smoothing), 0))

    def set_call_count(self, calls):
        self._ck(self.lib.m3_set_call_count(self._h, int(calls)))

    def sample_noise(self):
        """sampling_random / simple mode: this command's N(noise_mu, noise_sigma) draws into BUF_NOISE (what the
        fused rollout generates in registers) -- for the planner's STEP mode."""
        self._ck(self.lib.m3_sample_noise(self._h))
        return self.buffer(L.BUF_NOISE)

    def set_noise_halton(self, n_knots, degree=2, smoothing=0.5, scramble="none"):
        """The whole Halton-spline sampler on the device (knots included): include/m3p2i_hip.h.
        scramble: "none" (plain van der Corput, pinned by golden G8) or "faure" (generalized Halton)."""
        code = {"none": L.HALTON_PLAIN, "faure": L.HALTON_FAURE}[scramble]
        self._ck(self.lib.m3_set_noise_halton_scrambled(self._h, int(n_knots), int(degree), float(smoothing), code))

    def set_objective(self, task, goal, gripper_cmd=0):
        t = L.TASKS[task] if isinstance(task, str) else int(task)
        g = [float(x) for x in (goal.detach().cpu().reshape(-1).tolist()
                                if isinstance(goal, torch.Tensor) else np.ravel(goal))]
        arr = (C.c_float * len(g))(*g)
        self._ck(self.lib.m3_set_objective(self._h, t, arr, len(g), int(gripper_cmd)))

    def set_avoid_dyn_obs(self, on):
        """Extension (off = the reference): push / pull / push_pull add get_motion_cost like navigation does."""
        self._ck(self.lib.m3_set_avoid_dyn_obs(self._h, int(bool(on))))

    def set_point_cost_weights(self, weights=None):
        """Extension, point_env: the weights of the task costs (a mapping with keys of _lib.COST_WEIGHT_DEFAULTS, missing keys =
        the reference's literal; None = all defaults).  They apply from the next command / rollout / cost call."""
        if weights is None:
            self._ck(self.lib.m3_set_point_cost_weights(self._h, None))
            return
        unknown = sorted(set(weights) - set(L.COST_WEIGHT_DEFAULTS))
        if unknown:
            raise ValueError(f"unknown cost weight(s) {unknown}: one of {list(L.COST_WEIGHT_DEFAULTS)}")
        w = L.PointCostWeights(**{**L.COST_WEIGHT_DEFAULTS, **{k: float(v) for k, v in weights.items()}})
        self._ck(self.lib.m3_set_point_cost_weights(self._h, C.byref(w)))

    def point_cost_weights(self):
        w = L.PointCostWeights()
        self._ck(self.lib.m3_get_point_cost_weights(self._h, C.byref(w)))
        return {n: getattr(w, n) for n in L.COST_WEIGHT_DEFAULTS}

    def set_weighted_cost_instance(self, on=-1):
        """-1: the weighted kernels exactly when the weights are not the defaults (default); 1 / 0 forced (tests, A/B)."""
        self._ck(self.lib.m3_set_weighted_cost_instance(self._h, int(on)))

    def set_point_scene(self, scene=None, **overrides):
        """Extension, point_env: the arena (a mapping with keys of _lib.POINT_SCENE_DEFAULTS, missing keys = the reference's
        arena; keyword arguments override single fields; nothing at all = the defaults).  Applies from the next command /
        rollout / step / episode tick.  scenes.point_scene_from_actors derives the mapping from an actor list."""
        fields = {**(scene or {}), **overrides}
        if not fields:
            self._ck(self.lib.m3_set_point_scene(self._h, None))
            return
        sc = _point_scene_fields(fields)
        self._ck(self.lib.m3_set_point_scene(self._h, C.byref(sc)))

    def point_scene(self):
        sc = L.PointSceneFields()
        self._ck(self.lib.m3_get_point_scene(self._h, C.byref(sc)))
        return _point_scene_dict(sc)

    def _set_rows(self, kind, per_sample, rows):
        """one scene per environment (sim_only engines) or, per_sample, per sample of the fused rollout (planner engines);
        rows=None clears"""
        setter = getattr(self.lib, (kind.sample_rows if per_sample else kind.env_rows)[0])
        if rows is None:
            self._ck(setter(self._h, None, 0))
            return
        rows = list(rows)
        # (never a zero-length array, so that an empty list is a wrong length and not the null pointer that clears; the library
        # reads the rows only once n == K_local)
        arr = (kind.struct * max(len(rows), 1))()
        for i, fields in enumerate(rows):
            arr[i] = kind.from_row(i, fields)
        self._ck(setter(self._h, arr, len(rows)))

    def _get_row(self, kind, per_sample, i):
        sc = kind.struct()
        self._ck(getattr(self.lib, (kind.sample_rows if per_sample else kind.env_rows)[1])(self._h, int(i), C.byref(sc)))
        return kind.to_dict(sc)

    def set_point_scene_rows(self, rows=None):
        """Extension, sim_only point_env engines: one arena per environment -- rows[i] the field overrides of environment i
        over _lib.POINT_SCENE_DEFAULTS (None: the reference's arena); len(rows) == K_local.  rows=None clears: the engine is
        back on its single scene.  Applies from the next step / episode tick; set_point_scene afterwards clears the rows."""
        self._set_rows(_POINT_ROWS, False, rows)

    def point_scene_row(self, i):
        """environment i's arena as set by set_point_scene_rows (all fields)"""
        return self._get_row(_POINT_ROWS, False, i)

    def point_scene_rows_set(self):
        return self.lib.m3_point_scene_rows_set(self._h) == 1

    def set_point_rollout_scenes(self, rows=None):
        """Extension, point_env planner engines: one arena per SAMPLE of the fused rollout -- rows[i] the field overrides of
        local sample i (global k_offset + i) over _lib.POINT_SCENE_DEFAULTS (None: the reference's arena); len(rows) ==
        K_local.  rows=None clears: the engine is back on its single scene.  Applies from the next rollout / command;
        set_point_scene afterwards clears the rows.  The special samples (K - 1; multi-modal: 0 and K / 2) get their rows like
        any other: scenes.spread_point_scenes keeps them nominal."""
        self._set_rows(_POINT_ROWS, True, rows)

    def point_rollout_scene(self, i):
        """local sample i's arena as set by set_point_rollout_scenes (all fields)"""
        return self._get_row(_POINT_ROWS, True, i)

    def point_rollout_scenes_set(self):
        return self.lib.m3_point_rollout_scenes_set(self._h) == 1

    def set_prior_samples(self, seqs=None, indices=None):
        """Extension, unsharded point_env planner engines: PRIOR SAMPLES -- sample indices[j] of the next rollouts takes
        clamp(seqs[j], u_min, u_max) as its controls instead of clamp(mean + noise); seqs [n, T, nu] holds the controls of
        the steps of THIS command's horizon (nothing is shifted between commands), indices the n GLOBAL sample indices
        (default 0 .. n-1).  A torch tensor on the engine's device is copied device-to-device on the engine's stream (its
        values are not inspected); anything else goes through the host entry point, which refuses a non-finite value.
        seqs=None (or n = 0) clears.  See include/m3p2i_hip.h: m3_set_prior_samples."""
        self._set_prior_samples("set_prior_samples", self.lib.m3_set_prior_samples, self.lib.m3_set_prior_samples_device, seqs, indices)

    def _set_prior_samples(self, who, set_host, set_device, seqs, indices):
        if seqs is None or len(seqs) == 0:
            self._ck(set_host(self._h, None, None, 0))
            return
        c = self.cfg
        n = int(seqs.shape[0]) if hasattr(seqs, "shape") else len(seqs)
        idx = list(range(n)) if indices is None else [int(i) for i in indices]
        if len(idx) != n:
            raise ValueError(f"{who}: {n} sequences but {len(idx)} indices")
        arr = (C.c_int * max(n, 1))(*idx)
        if isinstance(seqs, torch.Tensor) and seqs.is_cuda and seqs.device == self.device:
            d = seqs.to(torch.float32).contiguous()
            if tuple(d.shape) != (n, c.T, c.nu):
                raise ValueError(f"{who}: seqs is {tuple(d.shape)}, expected (n, {c.T}, {c.nu})")
            # (the copy is ordered on the engine's stream, d lives until the call returns: keep it until that copy is over)
            self._ck(set_device(self._h, d.data_ptr(), arr, n))
            self._prior_src = d
            return
        d = np.ascontiguousarray(seqs.detach().cpu().numpy() if isinstance(seqs, torch.Tensor) else seqs, dtype=np.float32)
        if d.shape != (n, c.T, c.nu):
            raise ValueError(f"{who}: seqs is {d.shape}, expected (n, {c.T}, {c.nu})")
        self._ck(set_host(self._h, d.ctypes.data, arr, n))

    def set_panda_prior_samples(self, seqs=None, indices=None):
        """Extension, unsharded panda_env planner engines: PRIOR SAMPLES of the arm -- set_prior_samples with nu = 9 (seqs
        [n, T, 9]); behind the select the gripper command still overrides controls 7 and 8.  seqs=None (or n = 0) clears.
        See include/m3p2i_hip.h: m3_set_panda_prior_samples."""
        self._set_prior_samples("set_panda_prior_samples", self.lib.m3_set_panda_prior_samples,
                                self.lib.m3_set_panda_prior_samples_device, seqs, indices)

    def panda_prior_samples_set(self):
        """the number of panda_env prior samples set (0: none)"""
        return int(self.lib.m3_panda_prior_samples_set(self._h))

    def panda_prior_sample(self, j):
        """(global sample index, [T, 9] float32 array) of panda_env prior j as set through the host entry point"""
        k = C.c_int()
        seq = np.empty((self.cfg.T, self.cfg.nu), np.float32)
        self._ck_code(self.lib.m3_get_panda_prior_sample(self._h, int(j), C.byref(k), seq.ctypes.data), "m3_get_panda_prior_sample")
        return int(k.value), seq

    def panda_prior_samples_used(self):
        """1 / 0: the last rollout launched the panda_env prior kernels; -1 before the first"""
        return int(self.lib.m3_panda_prior_samples_used(self._h))

    def prior_samples_set(self):
        """the number of prior samples set (0: none)"""
        return int(self.lib.m3_prior_samples_set(self._h))

    def prior_sample(self, j):
        """(global sample index, [T, nu] float32 array) of prior j as set through the host entry point"""
        k = C.c_int()
        seq = np.empty((self.cfg.T, self.cfg.nu), np.float32)
        self._ck_code(self.lib.m3_get_prior_sample(self._h, int(j), C.byref(k), seq.ctypes.data), "m3_get_prior_sample")
        return int(k.value), seq

    def prior_samples_used(self):
        """1 / 0: the last rollout launched the prior build; -1 before the first"""
        return int(self.lib.m3_prior_samples_used(self._h))

    def set_prior_controller(self, kind=None, n=4, indices=None, speeds=None, standoff=None, reach=None):
        """Extension, unsharded point_env planner engines: an ancillary controller ON THE DEVICE (m3_set_prior_controller) --
        the library fills the table of prior samples from the world each rollout starts from, in a kernel ahead of it; nothing
        is uploaded per command.  kind: "go_to" | "push_behind" (or the M3_PRIOR_CONTROLLER_* value); n sequences, one per
        speed factor (default 1 - j / n), the priors of the GLOBAL samples indices (default 0 .. n-1).  kind=None clears
        controller and priors.  Against set_prior_samples the last call wins."""
        if kind is None:
            self._ck(self.lib.m3_set_prior_controller(self._h, None, None))
            return
        pc = L.PriorController()
        self.lib.m3_default_prior_controller(C.byref(pc), int(L.PRIOR_CONTROLLER_KINDS.get(kind, kind)), int(n))
        pc.n = int(n)     # (the defaults clamp n; the setter refuses what is out of range)
        if speeds is not None:
            if len(speeds) != int(n):
                raise ValueError(f"set_prior_controller: {int(n)} sequences but {len(speeds)} speed factors")
            if int(n) <= L.MAX_PRIOR_CONTROLLER_SEQS:
                for j, f in enumerate(speeds):
                    pc.speed[j] = float(f)
        if standoff is not None:
            pc.standoff = float(standoff)
        if reach is not None:
            pc.reach = float(reach)
        idx = list(range(int(n))) if indices is None else [int(i) for i in indices]
        if len(idx) != int(n):
            raise ValueError(f"set_prior_controller: {int(n)} sequences but {len(idx)} indices")
        self._ck(self.lib.m3_set_prior_controller(self._h, C.byref(pc), (C.c_int * max(len(idx), 1))(*idx)))

    def prior_controller(self):
        """the controller as set ({kind, n, speeds, standoff, reach}), or None"""
        pc = L.PriorController()
        self._ck_code(self.lib.m3_get_prior_controller(self._h, C.byref(pc)), "m3_get_prior_controller")
        if pc.kind == 0:
            return None
        return dict(kind=pc.kind, n=pc.n, speeds=[float(pc.speed[j]) for j in range(pc.n)], standoff=float(pc.standoff),
                    reach=float(pc.reach))

    def prior_controller_fill(self):
        """launches the controller alone, for the world currently set or bound (what the next rollout's launch would write)"""
        self._ck(self.lib.m3_prior_controller_fill(self._h))

    def prior_table(self) -> torch.Tensor:
        """zero-copy view [n, T, nu] of the rows of the table of prior samples that are set (read-only by convention; ordered
        on the engine's stream)"""
        p = C.c_void_p()
        n = C.c_int()
        self._ck_code(self.lib.m3_prior_table(self._h, C.byref(p), C.byref(n)), "m3_prior_table")
        return torch.as_tensor(_DevArray(p.value, (max(n.value, 1), self.cfg.T, self.cfg.nu), "<f4", self), device=self.device)[:n.value]

    def set_sample_groups(self, group_of=None, worst=1.0):
        """Extension, unsharded planner engines: SAMPLE GROUPS -- group_of[k] names the group of local sample k (-1: on its own;
        2 .. 16 members per group); after every rollout each group's costs become, in every member, the mean of the group's
        max(1, ceil(worst * size)) largest member costs (worst = 1: the mean; <= 1/16: the maximum), and the update runs on
        those.  That the members of a group carry the same noise rows is the caller's arrangement (groups.tile_noise;
        MPPI.set_sample_groups does it).  group_of=None clears.  See include/m3p2i_hip.h: m3_set_sample_groups."""
        if group_of is None:
            self._ck(self.lib.m3_set_sample_groups(self._h, None, 0, 1.0))
            return
        g = [int(i) for i in (group_of.tolist() if hasattr(group_of, "tolist") else group_of)]
        self._ck(self.lib.m3_set_sample_groups(self._h, (C.c_int * max(len(g), 1))(*g), len(g), float(worst)))

    def sample_groups_set(self):
        """the number of sample groups set (0: none)"""
        return int(self.lib.m3_sample_groups_set(self._h))

    def sample_group(self, k):
        """(group id as given or -1, size, worst_j) of local sample k"""
        g, m, j = C.c_int(), C.c_int(), C.c_int()
        self._ck_code(self.lib.m3_get_sample_group(self._h, int(k), C.byref(g), C.byref(m), C.byref(j)), "m3_get_sample_group")
        return int(g.value), int(m.value), int(j.value)

    def raw_costs(self) -> torch.Tensor:
        """zero-copy view [K_local] of the per-model costs of the last rollout, as they were before the groups' aggregation
        (read-only by convention; ordered on the engine's stream)"""
        p = C.c_void_p()
        self._ck(self.lib.m3_sample_group_raw_costs(self._h, C.byref(p)))
        return torch.as_tensor(_DevArray(p.value, (self.cfg.K_local,), "<f4", self), device=self.device)

    def aggregate_sample_groups(self):
        """launches the aggregation alone, on whatever BUF_TRAJ_COST holds"""
        self._ck(self.lib.m3_aggregate_sample_groups(self._h))

    def _ck_code(self, rc, who):
        # (the getters leave no message behind)
        if rc != 0:
            raise L.M3Error(f"m3p2i_hip error {rc}: {who}")

    def set_point_scene_instance(self, on=-1):
        """-1: the run-time-scene kernels exactly when the scene is not the default (default); 1 / 0 forced (tests, A/B)."""
        self._ck(self.lib.m3_set_point_scene_instance(self._h, int(on)))

    def set_panda_scene(self, scene=None, **overrides):
        """Extension, panda_env: the workspace (a mapping with keys of _lib.PANDA_SCENE_DEFAULTS -- base, table, shelf, obs_half
        as sequences, obs_m, cube_m, mu --, missing keys = the reference's workspace; keyword arguments override single fields;
        nothing at all = the defaults).  Applies from the next command / rollout / step / cost call.
        scenes.panda_scene_from_actors derives the mapping from an actor list."""
        fields = {**(scene or {}), **overrides}
        self.panda_scene_sets = getattr(self, "panda_scene_sets", 0) + 1     # (what a planner keeps its reading of the scene by)
        if not fields:
            self._ck(self.lib.m3_set_panda_scene(self._h, None))
            return
        sc = L.panda_scene_fields(fields)
        self._ck(self.lib.m3_set_panda_scene(self._h, C.byref(sc)))

    def panda_scene(self):
        sc = L.PandaSceneFields()
        self._ck(self.lib.m3_get_panda_scene(self._h, C.byref(sc)))
        return L.panda_scene_dict(sc)

    def set_panda_scene_instance(self, on=-1):
        """-1: the run-time-scene kernels exactly when geometry or friction are not the defaults (default); 1 / 0 forced
        (tests, A/B)."""
        self._ck(self.lib.m3_set_panda_scene_instance(self._h, int(on)))

    def panda_scene_instance_used(self):
        """whether the last rollout or step launched the run-time-scene instance"""
        return self.lib.m3_panda_scene_instance_used(self._h) == 1

    def set_panda_scene_rows(self, rows=None):
        """Extension, sim_only panda_env engines: one workspace per environment -- rows[i] the field overrides of environment i
        over _lib.PANDA_SCENE_DEFAULTS (None: the reference's workspace); len(rows) == K_local.  rows=None clears: the engine
        is back on its single workspace.  Applies from the next step / cost / view refresh; set_panda_scene afterwards clears
        the rows."""
        self._set_rows(_PANDA_ROWS, False, rows)

    def panda_scene_row(self, i):
        """environment i's workspace as set by set_panda_scene_rows (all fields)"""
        return self._get_row(_PANDA_ROWS, False, i)

    def panda_scene_rows_set(self):
        return self.lib.m3_panda_scene_rows_set(self._h) == 1

    def set_panda_rollout_scenes(self, rows=None):
        """Extension, panda_env planner engines: one workspace per SAMPLE of the fused rollout -- rows[i] the field overrides of
        local sample i (global k_offset + i) over _lib.PANDA_SCENE_DEFAULTS (None: the reference's workspace); len(rows) ==
        K_local.  rows=None clears: the engine is back on its single workspace.  Applies from the next rollout / command;
        set_panda_scene afterwards clears the rows.  The reach cost reads the cube of sample 0 as simulated in rows[0] (quirk
        Q8; multi-modal: the orientation of sample K / 2 in its row): scenes.spread_panda_scenes keeps those rows nominal."""
        self._set_rows(_PANDA_ROWS, True, rows)

    def panda_rollout_scene(self, i):
        """local sample i's workspace as set by set_panda_rollout_scenes (all fields)"""
        return self._get_row(_PANDA_ROWS, True, i)

    def panda_rollout_scenes_set(self):
        return self.lib.m3_panda_rollout_scenes_set(self._h) == 1

    def set_panda_cost_weights(self, weights=None):
        """Extension, panda_env: the weights of the task costs (a mapping with keys of _lib.PANDA_COST_WEIGHT_DEFAULTS, missing
        keys = the reference's literal; None = all defaults).  They apply from the next command / rollout / cost call."""
        if weights is None:
            self._ck(self.lib.m3_set_panda_cost_weights(self._h, None))
            return
        unknown = sorted(set(weights) - set(L.PANDA_COST_WEIGHT_DEFAULTS))
        if unknown:
            raise ValueError(f"unknown panda cost weight(s) {unknown}: one of {list(L.PANDA_COST_WEIGHT_DEFAULTS)}")
        w = L.PandaCostWeights(**{**L.PANDA_COST_WEIGHT_DEFAULTS, **{k: float(v) for k, v in weights.items()}})
        self._ck(self.lib.m3_set_panda_cost_weights(self._h, C.byref(w)))

    def panda_cost_weights(self):
        w = L.PandaCostWeights()
        self._ck(self.lib.m3_get_panda_cost_weights(self._h, C.byref(w)))
        return {n: getattr(w, n) for n in L.PANDA_COST_WEIGHT_DEFAULTS}

    def set_panda_weighted_cost_instance(self, on=-1):
        """-1: the weighted kernels exactly when the weights are not the defaults (default); 1 / 0 forced (tests, A/B)."""
        self._ck(self.lib.m3_set_panda_weighted_cost_instance(self._h, int(on)))

    def panda_weighted_cost_instance_used(self):
        """whether the last rollout or cost call launched the weighted kernels"""
        return self.lib.m3_panda_weighted_cost_instance_used(self._h) == 1

    def set_multi_modal(self, mm):
        self._ck(self.lib.m3_set_multi_modal(self._h, int(bool(mm))))

    def set_plan(self, which, values):
        v = np.ascontiguousarray(values, dtype=np.float32)
        assert v.shape == (self.cfg.T, self.cfg.nu)
        self._ck(self.lib.m3_set_plan(self._h, which, v.ctypes.data))

    def set_beta(self, beta):
        self._ck(self.lib.m3_set_beta(self._h, float(beta)))

    def reset(self):
        self._ck(self.lib.m3_reset(self._h))

    def set_action_out(self, tensor):
        """Redirect the returned plan into a caller-owned device tensor (None: library buffer)."""
        self._action_out = tensor
        if tensor is None:
            self._ck(self.lib.m3_set_action_out(self._h, None))
            return
        rows = self.cfg.u_per_command if self.cfg.mode_simple else self.cfg.T
        assert tensor.is_cuda and tensor.dtype == torch.float32 and tensor.is_contiguous()
        assert tuple(tensor.shape) == (rows, self.cfg.nu)
        self._ck(self.lib.m3_set_action_out(self._h, C.c_void_p(tensor.data_ptr())))

    def set_world_point(self, robot, box, dyn_obs):
        w = L.PointWorld()
        for dst, src, n in ((w.robot, robot, 4), (w.box, box, 7), (w.dyn_obs, dyn_obs, 7)):
            for i in range(n):
                dst[i] = float(src[i])
        self._ck(self.lib.m3_set_world_point(self._h, C.byref(w)))

    def set_world_point_raw(self, w18):
        arr = (C.c_float * 18)(*[float(x) for x in w18])
        self._ck(self.lib.m3_set_world_point_raw(self._h, arr))

    def set_world_panda_raw(self, w57):
        """q9 qd9 | cubeA | cubeB | dyn-obs, each pos3 quat4(xyzw) linvel3 angvel3 (include/m3p2i_hip.h)"""
        if len(w57) != 57:
            raise ValueError("set_world_panda_raw: 57 floats (q9 qd9 cubeA13 cubeB13 dyn-obs13), got %d" % len(w57))
        arr = (C.c_float * 57)(*[float(x) for x in w57])
        self._ck(self.lib.m3_set_world_panda_raw(self._h, arr))

    def bind_sim_panda(self, dof_state, root_state, cubeA_actor, cubeB_actor, obs_actor):
        assert dof_state.is_cuda and root_state.is_cuda and dof_state.dtype == torch.float32
        self._bound = (dof_state, root_state)
        self._ck(self.lib.m3_bind_sim_panda(self._h, dof_state.data_ptr(), root_state.data_ptr(),
                                            root_state.shape[-2], cubeA_actor, cubeB_actor, obs_actor))

    def bind_sim_point(self, dof_state, root_state, box_actor, dyn_actor):
        assert dof_state.is_cuda and root_state.is_cuda and dof_state.dtype == torch.float32
        self._bound = (dof_state, root_state)  # keep alive
        self._ck(self.lib.m3_bind_sim_point(self._h, dof_state.data_ptr(), root_state.data_ptr(),
                                            root_state.shape[-2], box_actor, dyn_actor))

    # ---- the hot path ----
    def command(self, sync_host=False):
        """One MPPI iteration.  Returns the device tensor [T, nu] of the filtered plan."""
        if sync_host:
            rows = self.cfg.u_per_command if self.cfg.mode_simple else self.cfg.T
            out = np.zeros((rows, self.cfg.nu), np.float32)
            self._ck(self.lib.m3_command(self._h, out.ctypes.data))
            return out
        self._ck(self.lib.m3_command(self._h, None))
        return self._action_out if self._action_out is not None else self.buffer(L.BUF_ACTION_OUT)

    def rollout(self):
        self._ck(self.lib.m3_rollout(self._h))

    def update(self):
        self._ck(self.lib.m3_update(self._h))

    def update_b(self):
        """shard_mix = 3, between the two exchanges: searches on the mixed tables, local weights and sums."""
        self._ck(self.lib.m3_update_b(self._h))

    def finalize(self):
        self._ck(self.lib.m3_finalize(self._h))

    # ---- device-side exchange of the records (include/m3p2i_hip.h: m3_p2p_*) ----
    def p2p_export(self) -> bytes:
        """This rank's exchange block as an IPC handle (64 bytes) for the other ranks' p2p_connect."""
        buf = C.create_string_buffer(L.IPC_HANDLE_BYTES)
        self._ck(self.lib.m3_p2p_export(self._h, C.cast(buf, C.c_void_p)))
        return buf.raw

    def p2p_connect(self, handles):
        """handles: the p2p_export() of every rank, in rank order (other processes)."""
        blob = b"".join(bytes(x) for x in handles)
        assert len(blob) == L.IPC_HANDLE_BYTES * len(handles)
        buf = C.create_string_buffer(blob, len(blob))
        self._ck(self.lib.m3_p2p_connect(self._h, C.cast(buf, C.c_void_p), len(handles)))

    def p2p_connect_local(self, engines):
        """engines: the HipEngine of every rank, in rank order, all living in this process."""
        arr = (C.c_void_p * len(engines))(*[e._h for e in engines])
        self._p2p_peers = list(engines)     # keep the peers' blocks alive as long as this handle writes into them
        self._ck(self.lib.m3_p2p_connect_local(self._h, arr, len(engines)))

    def p2p_put(self, channel=0):
        """channel 0: M3_BUF_RECORD; 1: M3_BUF_RECORD_B (the second exchange of shard_mix = 3)."""
        self._ck(self.lib.m3_p2p_put_ch(self._h, int(channel)))

    def p2p_wait(self, channel=0):
        self._ck(self.lib.m3_p2p_wait_ch(self._h, int(channel)))

    def p2p_exchange(self, channel=0):
        """put + wait in one launch (one process per GPU; a process driving several handles on one stream uses
        p2p_put / p2p_wait, every put before any wait)."""
        self._ck(self.lib.m3_p2p_exchange(self._h) if channel == 0 else self.lib.m3_p2p_exchange_b(self._h))

    def p2p_status(self):
        """(missing_rank or -1, memory kind: 1 uncached / 2 fine-grained / 3 plain); synchronises the stream."""
        miss, kind = C.c_int(), C.c_int()
        self._ck(self.lib.m3_p2p_status(self._h, C.byref(miss), C.byref(kind)))
        return miss.value, kind.value

    def p2p_set_timeout_ms(self, first_ms=30000, ms=500):
        """How long a wait spins for a missing peer: a channel's first exchange (start-up skew between the ranks) / later ones."""
        self._ck(self.lib.m3_p2p_set_timeout_ms(self._h, int(first_ms), int(ms)))

    def p2p_clear_error(self):
        """Collective re-arm after a wait that gave up: own flags, error word and sequence numbers back to zero (the caller
        holds a barrier before and after: distributed.p2p_recover)."""
        self._ck(self.lib.m3_p2p_clear_error(self._h))

    def p2p_detach(self):
        """This handle stops using the device-side exchange: finalize no longer reads its error word."""
        self._ck(self.lib.m3_p2p_detach(self._h))

    def p2p_set_memory_kind(self, first_kind=1):
        """Where the exchange block's allocation chain starts (1 uncached, 2 fine-grained, 3 plain); before export / connect."""
        self._ck(self.lib.m3_p2p_set_memory_kind(self._h, int(first_kind)))

    def update_finalize(self):
        """update + finalize of an unsharded handle in as few launches as possible."""
        self._ck(self.lib.m3_update_finalize(self._h))

    # ---- views ----
    def _shape(self, which):
        c = self.cfg
        Kl, Kg, T, nu = c.K_local, c.K_global, c.T, c.nu
        return {
            L.BUF_STATES: ((T, Kl, 4), "<f4"), L.BUF_ACTIONS: ((T, Kl, nu), "<f4"),
            L.BUF_COST_HORIZON: ((T, Kl), "<f4"), L.BUF_TRAJ_COST: ((Kl,), "<f4"),
            L.BUF_TRAJ_COST_ALL: ((Kg,), "<f4"), L.BUF_WEIGHTS: ((Kg,), "<f4"),
            L.BUF_WEIGHTS_1: ((Kg // 2,), "<f4"), L.BUF_WEIGHTS_2: ((Kg - Kg // 2,), "<f4"),
            L.BUF_MEAN: ((T, nu), "<f4"), L.BUF_MEAN_1: ((T, nu), "<f4"),
            L.BUF_MEAN_2: ((T, nu), "<f4"), L.BUF_BEST: ((T, nu), "<f4"),
            L.BUF_BEST_1: ((T, nu), "<f4"), L.BUF_BEST_2: ((T, nu), "<f4"),
            L.BUF_ACTION_OUT: ((T, nu), "<f4"), L.BUF_TOP_IDX: ((L.TOPK,), "<i4"),
            L.BUF_TOP_TRAJS: ((L.TOPK, T, 2), "<f4"),
            L.BUF_REDUCE: ((self.lib.m3_reduce_len(self._h),), "<f4"),
            L.BUF_NOISE: ((T, Kl, nu), "<f4"), L.BUF_PENDING_FORCE: ((4, Kl), "<f4"),
            L.BUF_SIM_WORLD: ((28 if c.env_type == L.ENV_POINT else 77, Kl), "<f4"),
            L.BUF_INFO: ((L.INFO_WORDS,), "<i4"),
            L.BUF_NOISE_ALL: ((Kg // Kl, T, Kl, nu), "<f4"),
            L.BUF_COV: ((2, nu), "<f4"),
            L.BUF_RECORD: ((self.lib.m3_record_len(self._h),), "<f4"),
            L.BUF_RECORDS_ALL: ((Kg // Kl, self.lib.m3_record_len(self._h)), "<f4"),
            L.BUF_RECORD_B: ((self.lib.m3_record_b_len(self._h),), "<f4"),
            L.BUF_RECORDS_B_ALL: ((Kg // Kl, self.lib.m3_record_b_len(self._h)), "<f4"),
        }[which]

    def buffer(self, which) -> torch.Tensor:
        """Zero-copy torch view of a library-owned device buffer."""
        if which in self._views:
            return self._views[which]
        p = C.c_void_p()
        n = C.c_longlong()
        self._ck(self.lib.m3_get_buffer(self._h, which, C.byref(p), C.byref(n)))
        shape, typestr = self._shape(which)
        t = torch.as_tensor(_DevArray(p.value, shape, typestr, self), device=self.device)
        self._views[which] = t
        return t

    def info(self) -> L.Info:
        i = L.Info()
        self._ck(self.lib.m3_get_info(self._h, C.byref(i)))
        return i

    def timing(self) -> L.Timing:
        t = L.Timing()
        self._ck(self.lib.m3_get_timing(self._h, C.byref(t)))
        return t

    # reference-layout conveniences ([K, T, c] strided views, no copies)
    @property
    def states(self):
        return self.buffer(L.BUF_STATES).permute(1, 0, 2)

    @property
    def actions(self):
        return self.buffer(L.BUF_ACTIONS).permute(1, 0, 2)

    @property
    def cost_horizon(self):
        return self.buffer(L.BUF_COST_HORIZON).permute(1, 0)

    # ---- step mode ----
    def sim_bind_views(self, dof_state, root_state, rigid_body_state, net_contact_force):
        self._simviews = (dof_state, root_state, rigid_body_state, net_contact_force)
        self._ck(self.lib.m3_sim_bind_views(
            self._h, dof_state.data_ptr(), root_state.data_ptr(), rigid_body_state.data_ptr(),
            net_contact_force.data_ptr(), root_state.shape[1], rigid_body_state.shape[1]))

    def sim_pull_state(self):
        self._ck(self.lib.m3_sim_pull_state(self._h))

    def sim_shift_actor(self, actor, dx, dy, dz=0.0):
        """root position of one actor of every environment += (dx, dy, dz) in the bound view, then the state
        upload -- one launch (update_dyn_obs)."""
        self._ck(self.lib.m3_sim_shift_actor(self._h, int(actor), float(dx), float(dy), float(dz)))

    def sim_push_state(self):
        self._ck(self.lib.m3_sim_push_state(self._h))

    def sim_set_velocity_target(self, u, zero_copy=False):
        """Velocity targets for the next sim_step().  Default: COPIED at this point into an engine-owned tensor (one
        small device copy on the stream) -- Isaac Gym's set_dof_velocity_target_tensor semantics: what the caller does
        with `u` afterwards does not matter.  zero_copy=True (the closed-loop tools, which own their tensors): the
        pointer is handed to the step kernel instead (one launch less per tick); the caller must leave the tensor alone
        until step() -- an in-place torch op in between is detected and refused there, a write by another library
        call (e.g. the planner's action ring being rewritten eight commands later) is not."""
        u = u.to(torch.float32).contiguous()
        assert u.is_cuda and tuple(u.shape) == (self.cfg.K_local, self.cfg.nu), u.shape
        if not zero_copy:
            if getattr(self, "_u_target", None) is None:
                self._u_target = torch.empty(self.cfg.K_local, self.cfg.nu, device=self.device, dtype=torch.float32)
            self._u_target.copy_(u)
            u = self._u_target
        self._pending_u = (u, u._version)

    def sim_apply_body_forces(self, f):
        f = f.to(torch.float32).contiguous()
        assert f.is_cuda
        self._ck(self.lib.m3_sim_apply_body_forces(self._h, f.data_ptr()))

    def sim_step(self):
        pending = getattr(self, "_pending_u", None)
        if pending is None:
            self._ck(self.lib.m3_sim_step(self._h))      # the targets of the last set call stay in force
            return
        u, version = pending
        self._pending_u = None      # (cleared on every path: a failed step must not leave a stale target behind)
        if u._version != version:
            raise RuntimeError("the velocity-target tensor was modified in place between "
                               "set_dof_velocity_target_tensor() and step(): pass a clone")
        self._ck(self.lib.m3_sim_step_with_target(self._h, u.data_ptr()))

    def sim_suction_forces(self, kp_suction):
        """calculate_suction on the device: [K_local, n_bodies, 3] body forces (skill_utils.py:59-94)."""
        nb = self._simviews[2].shape[1]
        f = torch.empty(self.cfg.K_local, nb, 3, device=self.device, dtype=torch.float32)
        self._ck(self.lib.m3_sim_suction_forces(self._h, float(kp_suction), f.data_ptr()))
        return f

    def sim_check_and_apply_suction(self, action, kp_suction, apply=True, want_flags=False, enabled=None):
        """check_suction_condition (+ apply_rigid_body_force_tensors(calculate_suction) where it holds)
        on the device, no host sync (skill_utils.py:36-56).  enabled: optional 1-element int32 device
        tensor that gates the suction (the planner's pull preference).  Returns the per-env condition
        (int32 device tensor) if want_flags."""
        a = action.to(device=self.device, dtype=torch.float32).reshape(self.cfg.K_local, 2).contiguous()
        flags = torch.empty(self.cfg.K_local, device=self.device, dtype=torch.int32) if want_flags else None
        if enabled is not None:
            assert enabled.is_cuda and enabled.dtype == torch.int32 and enabled.numel() == 1
            self._gate = enabled   # keep alive until the kernel ran
        self._ck(self.lib.m3_sim_check_and_apply_suction(
            self._h, a.data_ptr(), float(kp_suction), int(bool(apply)),
            C.c_void_p(flags.data_ptr()) if want_flags else None,
            C.c_void_p(enabled.data_ptr()) if enabled is not None else None))
        return flags

    def cost(self, out=None):
        if out is None:
            out = torch.empty(self.cfg.K_local, device=self.device, dtype=torch.float32)
        self._ck(self.lib.m3_cost(self._h, out.data_ptr()))
        return out


class HipBatch(_CObject):
    """One command() of each of several HipEngines (unsharded handles of one environment per call: point_env or
    panda_env, as the first engine's) in one rollout launch and one update launch per group of handles that run the same
    kernel instance (``m3_batch_command``, include/m3p2i_hip.h).  Each engine's results are bit-identical to its own
    ``command()``, a panda_env engine's automatic kernel form included; the batch holds no planner state, only the device
    workspace of its argument table (allocated here, for up to ``max_handles`` engines per call).
    ``panda_runtime=True`` (``M3_BATCH_PANDA_RUNTIME``) makes room for the larger table entries of panda_env engines with a
    workspace of their own, tuned cost weights or a workspace per sample, which any other batch refuses.
    ``point_runtime=True`` (``M3_BATCH_SECTION_POINT_ROLLOUT_SCENES``, ``m3_batch_create_sections``) makes room for the entries
    of point_env engines with an arena per sample (``set_point_rollout_scenes``), which any other batch refuses.
    ``point_priors=True`` (``M3_BATCH_SECTION_POINT_PRIORS``) makes room for the entries of point_env engines with prior samples
    (``set_prior_samples`` / ``set_prior_controller``; with or without an arena per sample), which any other batch refuses."""

    _ptr, _destroy, _last_error = "_b", "m3_batch_destroy", "m3_batch_last_error"

    def __init__(self, max_handles, device=0, panda_runtime=False, point_runtime=False, point_priors=False):
        if not torch.cuda.is_available():
            raise L.M3Error("HipBatch needs a HIP device (torch.cuda.is_available() is False); there is no CPU fallback")
        self.lib = L.load()
        self.max_handles = int(max_handles)
        self.device = torch.device(f"cuda:{int(device)}")
        self._b = C.c_void_p()
        torch.cuda.set_device(self.device)
        torch.zeros(1, device=self.device)  # make sure the HIP context exists
        if point_runtime or point_priors:
            sections = ((L.BATCH_SECTION_POINT_ROLLOUT_SCENES if point_runtime else 0) | (L.BATCH_SECTION_PANDA_RUNTIME if panda_runtime else 0)
                        | (L.BATCH_SECTION_POINT_PRIORS if point_priors else 0))
            self._ck(self.lib.m3_batch_create_sections(int(device), self.max_handles, sections, C.byref(self._b)))
        elif panda_runtime:
            self._ck(self.lib.m3_batch_create_ex(int(device), self.max_handles, L.BATCH_PANDA_RUNTIME, C.byref(self._b)))
        else:
            self._ck(self.lib.m3_batch_create(int(device), self.max_handles, C.byref(self._b)))
        self._arr = (C.c_void_p * self.max_handles)()

    def command(self, engines, sync_host=False):
        """One MPPI iteration of every engine.  Returns each engine's plan tensor (its set_action_out tensor or the
        library's ACTION_OUT view), or with sync_host=True the plans on the host: an [n, rows, nu] array (a list of
        [rows, nu] arrays when the engines' row counts differ)."""
        engines = list(engines)
        n = len(engines)
        arr = self._arr if n <= self.max_handles else (C.c_void_p * n)()   # (the library refuses n > max_handles)
        for i, e in enumerate(engines):
            arr[i] = e._h.value
        if sync_host:
            rows = [e.cfg.u_per_command if e.cfg.mode_simple else e.cfg.T for e in engines]
            sizes = [r * e.cfg.nu for r, e in zip(rows, engines)]
            out = np.zeros(max(sum(sizes), 1), np.float32)
            self._ck(self.lib.m3_batch_command(self._b, arr, n, out.ctypes.data))
            if len(set(rows)) == 1 and len({e.cfg.nu for e in engines}) == 1:
                return out[:sum(sizes)].reshape(n, rows[0], engines[0].cfg.nu)
            offs = np.cumsum([0] + sizes)
            return [out[offs[i]:offs[i + 1]].reshape(rows[i], engines[i].cfg.nu) for i in range(n)]
        self._ck(self.lib.m3_batch_command(self._b, arr, n, None))
        return [e._action_out if e._action_out is not None else e.buffer(L.BUF_ACTION_OUT) for e in engines]

    def flags(self):
        """The sections the batch was created with (``L.BATCH_SECTION_*`` bits; ``L.BATCH_PANDA_RUNTIME`` is bit 1)."""
        flags = self.lib.m3_batch_flags(self._b)
        if flags < 0:
            self._ck(flags)
        return flags

    def launches(self):
        """(rollout launches, update launches) of the last successful command."""
        r, u = C.c_int(), C.c_int()
        self._ck(self.lib.m3_batch_launches(self._b, C.byref(r), C.byref(u)))
        return r.value, u.value


class HipEpisodes(_CObject):
    """N closed-loop point_env episodes in lockstep (``m3_episodes_*``, include/m3p2i_hip.h): row e of the
    N-env world engine (an ``IsaacGymWrapper(num_envs=N)``'s) is episode e's 1-env world, planned by ``engines[e]``.
    ``specs``: one ``(task, goal, dyn_phase, suction, kp_suction)`` per episode, task a name or M3_TASK_* id, suction one of
    ``L.SUCTION_*``.  Each engine's ``set_action_out`` tensor is read here and must stay the same.  The set owns its
    device state and pinned status words; a tick allocates nothing.
    ``point_runtime=True`` (``M3_EPISODES_ROLLOUT_SCENES``, ``m3_episodes_create_ex``) also takes planners with an arena per
    sample (``set_point_rollout_scenes``), at create and at every tick; hand ``tick`` a ``HipBatch(..., point_runtime=True)``.
    The world's rows step in the world engine's arena either way.
    ``point_priors=True`` (``M3_EPISODES_PRIORS``) also takes planners with prior samples (``set_prior_samples`` /
    ``set_prior_controller``), at create and at every tick; hand ``tick`` a ``HipBatch(..., point_priors=True)``.  A planner's
    controller reads its episode's row of the world every tick, on the device."""

    _ptr, _destroy, _last_error = "_eps", "m3_episodes_destroy", "m3_episodes_last_error"

    def __init__(self, world, engines, specs, max_ticks, trace=False, point_runtime=False, point_priors=False):
        self.lib = L.load()
        self.world, self.engines = world, list(engines)
        self.n, self.max_ticks, self.trace_on = len(self.engines), int(max_ticks), bool(trace)
        arr = (C.c_void_p * max(self.n, 1))(*[e._h.value for e in self.engines])
        sp = (L.EpisodeSpec * max(self.n, 1))()
        for i, (task, goal, phase, suction, kp) in enumerate(specs):
            sp[i].task = L.TASKS[task] if isinstance(task, str) else int(task)
            sp[i].goal[0], sp[i].goal[1] = float(goal[0]), float(goal[1])
            sp[i].dyn_phase, sp[i].suction, sp[i].kp_suction = int(phase), int(suction), float(kp)
        self._eps = C.c_void_p()
        if point_runtime or point_priors:
            flags = (L.EPISODES_ROLLOUT_SCENES if point_runtime else 0) | (L.EPISODES_PRIORS if point_priors else 0)
            self._ck(self.lib.m3_episodes_create_ex(world._h, arr, sp, self.n, self.max_ticks, int(self.trace_on), flags,
                                                    C.byref(self._eps)))
        else:
            self._ck(self.lib.m3_episodes_create(world._h, arr, sp, self.n, self.max_ticks, int(self.trace_on), C.byref(self._eps)))
        self._status = (L.EpisodeStatus * self.n)()

    def tick(self, batch):
        """One tick of every episode: pre kernel, one batched command of the running episodes' planners, post kernel,
        one synchronisation."""
        self._ck(self.lib.m3_episodes_tick(self._eps, batch._b))

    def flags(self):
        """The flags the set was created with (``L.EPISODES_ROLLOUT_SCENES`` / ``L.EPISODES_PRIORS`` bits)."""
        flags = self.lib.m3_episodes_flags(self._eps)
        if flags < 0:
            self._ck(flags)
        return flags

    def begin(self):
        """The pre-command half of a tick whose commands the caller issues itself (a planner's first command)."""
        self._ck(self.lib.m3_episodes_begin(self._eps))

    def end(self):
        self._ck(self.lib.m3_episodes_end(self._eps))

    @property
    def running(self):
        """Episodes not ended as of the last tick (host copy, no synchronisation)."""
        return int(self.lib.m3_episodes_running(self._eps))

    @property
    def ticks_done(self):
        return int(self.lib.m3_episodes_ticks_done(self._eps))

    def status(self, with_trace=False):
        """[dict(done_tick, success, collision_ticks, final_pos)] per episode, and with_trace the trace as a
        [max_ticks, n, 10] float32 array."""
        tr = np.empty((self.max_ticks, self.n, 10), np.float32) if with_trace else None
        self._ck(self.lib.m3_episodes_status(self._eps, self._status, tr.ctypes.data if tr is not None else None))
        st = [dict(done_tick=s.done_tick, success=bool(s.success), collision_ticks=s.collision_ticks,
                   final_pos=(s.final_pos[0], s.final_pos[1])) for s in self._status]
        return (st, tr) if with_trace else st


class HipPandaEpisodes(_CObject):
    """N closed-loop panda_env episodes in lockstep (``m3_panda_episodes_*``, include/m3p2i_hip.h): row e of
    the N-env world engine (an ``IsaacGymWrapper(..., "panda_env", num_envs=N)``'s) is episode e's 1-env world, planned by
    ``engines[e]``.  The task planners stay on the host: a tick is ``observe()`` (the link rows they read, one copy, one
    synchronisation), their decisions, ``act(batch, ended)``.  Each engine's ``set_action_out`` tensor is read here and must
    stay the same.  The set owns its device state, planning views and pinned host copy; a tick allocates nothing.
    ``panda_runtime=True`` (``M3_PANDA_EPISODES_RUNTIME``, ``m3_panda_episodes_create_ex``) also takes a world with a workspace
    of its own or one per environment and planners with a workspace of their own, tuned cost weights or a workspace per
    sample: row e of the world steps in the world's workspace of row e, the planning view of episode e in planner e's; hand
    ``act`` a ``HipBatch(..., panda_runtime=True)``."""

    _ptr, _destroy, _last_error = "_eps", "m3_panda_episodes_destroy", "m3_panda_episodes_last_error"

    def __init__(self, world, engines, max_ticks, settle_ticks=0, trace=False, panda_runtime=False):
        self.lib = L.load()
        self.world, self.engines = world, list(engines)
        self.n, self.max_ticks, self.settle_ticks, self.trace_on = len(self.engines), int(max_ticks), int(settle_ticks), bool(trace)
        arr = (C.c_void_p * max(self.n, 1))(*[e._h.value for e in self.engines])
        self._eps = C.c_void_p()
        if panda_runtime:
            self._ck(self.lib.m3_panda_episodes_create_ex(world._h, arr, self.n, self.max_ticks, self.settle_ticks,
                                                          int(self.trace_on), L.PANDA_EPISODES_RUNTIME, C.byref(self._eps)))
        else:
            self._ck(self.lib.m3_panda_episodes_create(world._h, arr, self.n, self.max_ticks, self.settle_ticks, int(self.trace_on),
                                                       C.byref(self._eps)))
        self._status = (L.PandaEpisodeStatus * self.n)()
        self._ended = (C.c_int * self.n)()
        self._rb = C.POINTER(C.c_float)()
        self.bodies = int(world._simviews[2].shape[1])

    def flags(self):
        """The flags the set was created with (``L.PANDA_EPISODES_RUNTIME`` or 0)."""
        flags = self.lib.m3_panda_episodes_flags(self._eps)
        if flags < 0:
            self._ck(flags)
        return flags

    def observe(self):
        """Pre kernel, one device-to-host copy, one synchronisation.  Returns the planning view's rigid-body rows as an
        [n, bodies, 13] float32 array over the set's pinned memory: valid until the next observe()."""
        self._ck(self.lib.m3_panda_episodes_observe(self._eps, C.byref(self._rb)))
        return np.ctypeslib.as_array(self._rb, shape=(self.n, self.bodies, 13))

    def _flags(self, ended):
        for i in range(self.n):
            self._ended[i] = int(bool(ended[i]))
        return self._ended

    def act(self, batch, ended):
        """ended[e]: episode e's task is done at this tick (the host's check_task_success).  Binds the planners that go on
        to their rows, one batched command, post kernel; no synchronisation."""
        self._ck(self.lib.m3_panda_episodes_act(self._eps, batch._b, self._flags(ended)))

    def act_first(self, sims, ended):
        """Tick 0, after each planner's own first command: no command here; sims[e] is planner e's K-env simulator engine,
        whose kept velocity targets (row 0) become episode e's."""
        arr = (C.c_void_p * self.n)(*[s._h.value for s in sims])
        self._ck(self.lib.m3_panda_episodes_act_first(self._eps, arr, self._flags(ended)))

    @property
    def running(self):
        """Episodes the host has not ended (host mirror, no synchronisation)."""
        return int(self.lib.m3_panda_episodes_running(self._eps))

    @property
    def active(self):
        """Episodes running or still settling."""
        return int(self.lib.m3_panda_episodes_active(self._eps))

    @property
    def ticks_done(self):
        return int(self.lib.m3_panda_episodes_ticks_done(self._eps))

    def status(self, with_trace=False):
        """[dict(phase, done_tick, success, cubeA, cubeB)] per episode (positions as float32 arrays), and with_trace the
        trace as a [max_ticks, n, 132] float32 array (L.PE_TR_* offsets)."""
        tr = np.empty((self.max_ticks, self.n, L.PANDA_EPISODE_TRACE_FLOATS), np.float32) if with_trace else None
        self._ck(self.lib.m3_panda_episodes_status(self._eps, self._status, tr.ctypes.data if tr is not None else None))
        st = [dict(phase=s.phase, done_tick=s.done_tick, success=bool(s.success),
                   cubeA=np.array(s.cubeA[:], np.float32), cubeB=np.array(s.cubeB[:], np.float32)) for s in self._status]
        return (st, tr) if with_trace else st
