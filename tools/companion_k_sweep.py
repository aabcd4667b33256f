"""GPU experiment: up to which workgroup count does the two-wavefront form of the point rollout (dynamics + companion
wavefront, m3_set_point_rollout_form) pay?  Push, T = 30, the Halton-spline noise table (the per-task instance), both forms
on two handles of one process, commands alternating; HIP-event time of the rollout launch.  Prints one JSON line per K and
writes them as a JSON list to OUT (default k_sweep_push.json in the working directory; the committed run is
profiles/companion_wave/k_sweep_push.json).
    python tools/companion_k_sweep.py [K,K,...] [OUT]"""
import json, os, sys
import numpy as np, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from m3p2i_aip_amd.engine import HipEngine, make_config

T = 30
Ks = [int(x) for x in (sys.argv[1] if len(sys.argv) > 1 else "2000,10000,16384,32768,65536").split(",")]
out = []
for K in Ks:
    engs = []
    for form in (0, 1):
        e = HipEngine(make_config(K=K, T=T, nu=2, u_min=[-3, -3], u_max=[3, 3], noise_sigma_diag=[3, 3], seed=1))
        e.set_noise_halton(T // 4, 2, 0.5, "none")
        e.set_objective("push", (-1.0, -1.0))
        e.set_point_rollout_form(form)
        e.enable_timing(True)
        engs.append(e)
    ts = ([], [])
    for it in range(5 + 40):
        for f, e in enumerate(engs):
            e.command()
            torch.cuda.synchronize()
            if it >= 5:
                t = e.timing()
                ts[f].append((t.rollout_ms, t.total_ms))
    rec = dict(K=K, T=T, workgroups=(K + 63) // 64, form_used=[e.point_rollout_form_used() for e in engs])
    for f in (0, 1):
        a = np.array(ts[f])
        rec[f"form{f}_rollout_ms"] = dict(median=float(np.median(a[:, 0])), min=float(a[:, 0].min()), max=float(a[:, 0].max()))
        rec[f"form{f}_command_ms_median"] = float(np.median(a[:, 1]))
    rec["rollout_ratio_form1_over_form0"] = rec["form1_rollout_ms"]["median"] / rec["form0_rollout_ms"]["median"]
    same = all(torch.equal(engs[0].buffer(b), engs[1].buffer(b)) for b in (1, 2, 3))   # actions, per-step costs, trajectory costs
    rec["same_bits"] = bool(same)
    out.append(rec)
    print(json.dumps(rec), flush=True)
    for e in engs:
        e.close()
json.dump(out, open(sys.argv[2] if len(sys.argv) > 2 else "k_sweep_push.json", "w"), indent=1)
