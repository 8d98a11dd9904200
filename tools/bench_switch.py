#!/usr/bin/env python
"""Times of Hamiltonian switching (systems.Switch, nfk_switch.hip) in launches of
whole chunks of steps against the per-step path on one GPU.

    python tools/bench_switch.py [--steps 1000] [--out profiles/switch_bench.json]

Three paths alternate inside one process, window by window:

  one_launch  ``Switch.switch`` over a linear ramp of ``steps`` steps: launches of
              at most ``config.LANGEVIN_STEPS_PER_LAUNCH`` steps, the work of every
              step accumulated in the kernel
  per_step    ``fused_dynamics = False``: per step nfk_philox_fill, the Einstein
              and the target's force kernels, torch elementwise ops and one energy
              evaluation (the zero-step call of the switching kernel, one launch in
              place of the two energy launches the older kernels would need: the
              only part of this path that is not the parent commit's, and it can
              only flatter the baseline)
  langevin    the target's plain ``langevin`` of the same number of steps in
              launches (nfk_langevin.hip): ``vs_langevin`` = one_launch / langevin
              is what the second force and the energy pass of a step cost

Shapes: an Einstein crystal (alpha 600) against LJ-32 (cutoff 1.6, dt 0.002, kT 1)
and against systems.EAM at the Fe shape of tools/bench_eam.py (n = 54, dt 0.005,
the Fe configs' kT), at 500 and 5,000 rows.  Both switching paths are first checked
against each other bit for bit on a short run.  Times are device-event windows
(median, min, max over --windows windows of --iters calls) after warm-up.  Not the
bench.py contract line.
"""
from __future__ import annotations

import argparse
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=1000)
    ap.add_argument("--iters", type=int, default=1, help="calls per window")
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--rows", type=int, nargs="+", default=[500, 5000])
    ap.add_argument("--kinds", nargs="+", default=["lj", "eam"], choices=("lj", "eam"))
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "switch_bench.json"))
    a = ap.parse_args()
    import torch

    import bench_dynamics as bd
    from normalizingflow_amd import config, systems
    dev = torch.device("cuda", 0)
    res = {"tool": "tools/bench_switch.py", "device": torch.cuda.get_device_name(0), "steps": a.steps,
           "iters": a.iters, "windows": a.windows, "steps_per_launch": config.LANGEVIN_STEPS_PER_LAUNCH,
           "switch": {}}
    lam = torch.linspace(0, 1, a.steps + 1)
    for kind in a.kinds:
        target, _ = bd.systems_pair(kind, dev)
        kT = bd.KT_FE if kind == "eam" else 1.0
        lat = bd.fcc32()
        if kind == "eam":  # the bcc lattice that bd.start perturbs
            import numpy as np
            c = np.arange(3)
            corner = np.stack(np.meshgrid(c, c, c, indexing="ij"), -1).reshape(-1, 3).astype(np.float64)
            lat = torch.as_tensor(np.concatenate((corner, corner + 0.5)) * bd.bench_eam().A_FE, dtype=torch.float32)
        crystal = systems.EinsteinCrystal(lat, 3, boxlength=None, alpha=600, device=dev)
        fused, slow = systems.Switch(crystal, target, kT=kT), systems.Switch(crystal, target, kT=kT)
        slow.fused_dynamics = False
        for rows in a.rows:
            x, v, dt = bd.start(kind, rows, dev)
            kw = dict(dt=dt, seed=1, init_pos=x, init_velocity=v)
            short = [sw.switch(lam, nsteps=5, **kw) + (sw.get_velocity(),) for sw in (fused, slow)]
            assert all(torch.equal(p, q) for p, q in zip(*short)), "the two paths differ"
            r = bd.windows({"one_launch": lambda: fused.switch(lam, **kw),
                            "per_step": lambda: slow.switch(lam, **kw),
                            "langevin": lambda: target.langevin(a.steps, kT=kT, **kw)},
                           a.iters, a.windows, ratio=("one_launch", "per_step"))
            r["one_launch_ms_per_step"] = round(r["one_launch"]["median_ms"] / a.steps, 6)
            r["vs_langevin"] = round(r["one_launch"]["median_ms"] / r["langevin"]["median_ms"], 4)
            res["switch"]["%s_rows%d" % (kind, rows)] = r
            print(kind, rows, json.dumps(r), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(json.dumps(res, indent=1) + "\n")
    print(json.dumps(res))
    return 0


if __name__ == "__main__":
    sys.exit(main())
