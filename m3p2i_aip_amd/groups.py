"""Sample groups (m3_set_sample_groups): the layout of a planner's K samples into groups of M members
that roll the same control sequence out in M models, and the tiling of the noise table that makes the members' controls equal.

The library aggregates each group's costs into one number (the mean of its worst members) ahead of the update; that the members
carry the same noise rows is arranged here.  Host-side helpers: no GPU, no library call.
"""
from __future__ import annotations

import numpy as np

MAX_MEMBERS = 16     # a group is one 16-lane row of the aggregation kernel (csrc/sample_groups.hip)


def special_samples(K, multi_modal):
    """the samples whose controls are no row of the noise table: K - 1 (zero noise / null action); multi-modal: 0 and K / 2
    (the best trajectories)"""
    K = int(K)
    return sorted({K - 1} | ({0, K // 2} if multi_modal else set()))


def grouped_layout(K, M, multi_modal=False):
    """(group_of, model_of) for K samples in groups of M models, as int arrays [K].

    group_of[k]: the group of sample k (the index of its first member) or -1 for a sample on its own; model_of[k]: the model
    0 .. M-1 sample k rolls out in, or -1 for the nominal model.  The special samples are on their own on the nominal model.
    Per half of a multi-modal planner (a group may not have members on both sides of K / 2), else over the whole range: the
    usable samples form G = usable // M groups, member m of group g at base + g + m * G on model m -- so model m's samples are
    one contiguous run, and the first members (whose noise rows the group takes, tile_noise) are the first G rows.  What is
    left over is on its own on the nominal model."""
    K, M = int(K), int(M)
    if not 2 <= M <= MAX_MEMBERS:
        raise ValueError(f"grouped_layout: M = {M} models per group is not in 2 .. {MAX_MEMBERS}")
    if K < 2:
        raise ValueError(f"grouped_layout: K = {K}")
    group_of = np.full(K, -1, dtype=np.int32)
    model_of = np.full(K, -1, dtype=np.int32)
    special = set(special_samples(K, multi_modal))
    halves = [(0, K // 2), (K // 2, K)] if multi_modal else [(0, K)]
    n_groups = 0
    for lo, hi in halves:
        usable = [k for k in range(lo, hi) if k not in special]     # (contiguous: the specials sit at the ends)
        if not usable:
            continue
        base, G = usable[0], len(usable) // M
        for g in range(G):
            for m in range(M):
                k = base + g + m * G
                group_of[k] = base + g
                model_of[k] = m
        n_groups += G
    if n_groups == 0:
        raise ValueError(f"grouped_layout: K = {K} leaves no room for a group of {M}")
    return group_of, model_of


def first_members(group_of):
    """src[k]: the first (smallest) member of sample k's group, k itself for a sample on its own"""
    g = np.asarray(group_of).astype(np.int64).reshape(-1)
    src = np.arange(len(g), dtype=np.int64)
    first = {}
    for k, gid in enumerate(g.tolist()):
        if gid < 0:
            continue
        src[k] = first.setdefault(gid, k)
    return src


def tile_noise(delta, group_of):
    """delta [K, T, nu] (numpy array or torch tensor) with every member's row replaced by its group's first member's row: the
    members of a group then perturb the plan by the same noise, so their controls are equal.  A new array; samples on their
    own keep their rows."""
    src = first_members(group_of)
    if len(src) != len(delta):
        raise ValueError(f"tile_noise: {len(delta)} noise rows for {len(src)} samples")
    if isinstance(delta, np.ndarray):
        return np.ascontiguousarray(delta[src])
    import torch
    return delta[torch.as_tensor(src, device=delta.device)].contiguous()


def aggregate_reference(costs, group_of, worst=1.0):
    """The library's aggregate, emulated in numpy binary32 (the arithmetic of csrc/sample_groups.hpp, bit for bit): per group the
    member costs sorted in descending order of their encodings (-0.0 below +0.0), the j = max(1, ceil(worst * size)) largest
    summed by the fixed pairwise tree SUM16 over a row padded with zeros, one division by j; a NaN member makes the aggregate
    the canonical quiet NaN.  costs [K] float32 -> a new [K] float32 array; samples on their own keep their costs."""
    c = np.array(costs, dtype=np.float32).reshape(-1)
    out = c.copy()
    g = np.asarray(group_of).astype(np.int64).reshape(-1)
    wf = np.float32(worst)
    for gid in np.unique(g[g >= 0]).tolist():
        members = np.nonzero(g == gid)[0]
        out[members] = aggregate_one(c[members], worst_j(wf, len(members)))
    return out


def worst_j(worst, size):
    """j = max(1, ceil(worst * size)): worst as binary32, the product and the ceiling in binary64"""
    return int(min(max(1, int(np.ceil(float(np.float32(worst)) * float(size)))), size))


def aggregate_one(member_costs, j):
    """one group's aggregate (see aggregate_reference)"""
    c = np.asarray(member_costs, dtype=np.float32)
    if np.isnan(c).any():
        return np.uint32(0x7fc00000).view(np.float32)
    bits = c.view(np.int32)
    key = bits ^ ((bits >> 31) & np.int32(0x7fffffff))       # the total order of the encodings
    order = np.argsort(-key.astype(np.int64), kind="stable")
    v = np.zeros(16, dtype=np.float32)
    v[:j] = c[order][:j]
    with np.errstate(invalid="ignore", over="ignore"):
        while len(v) > 1:                                    # ((v0+v1)+(v2+v3)) + ...
            v = (v[0::2] + v[1::2]).astype(np.float32)
        return np.float32(v[0] / np.float32(j))
