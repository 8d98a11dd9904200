#!/usr/bin/env python
"""Times of Langevin dynamics in launches of whole chunks of steps
(nfk_langevin.hip) against the per-step path on one GPU.

    python tools/bench_langevin.py [--steps 1000] [--out profiles/langevin/bench_langevin.json]

Two paths alternate inside one process, window by window:

  one_launch  ``langevin(steps)``: launches of at most
              ``config.LANGEVIN_STEPS_PER_LAUNCH`` steps (lifted to ``steps`` with
              --single, to time one launch of that many steps)
  per_step    ``fused_dynamics = False``: nfk_philox_fill, the force kernel and
              torch elementwise ops per step

Two more rows place the generator.  ``nve_one_launch`` is the velocity-Verlet
trajectory of the same number of steps in one launch (nfk_*_trajectory): the
same force loop, registers and barriers without the noise, so
``rng_share`` = 1 - nve / one_launch (both single launches, --single) is what
the thermostat adds inside the kernel.  ``fill_only`` is ``steps`` launches of
nfk_philox_fill ([rows, n, 3] zero-mean normals): at these sizes a fill is a
launch's overhead, which is what the per-step path pays for its noise.

Shapes: LJ-32 (cutoff 1.6, dt 0.002, kT 1) and systems.EAM at the Fe shape of
tools/bench_eam.py (n = 54, dt 0.005, the Fe configs' kT) at 500 and 5,000 rows.
Both paths are first checked against each other bit for bit on a short run.
Times are device-event windows (median, min, max over --windows windows of
--iters calls) after warm-up.  Not the bench.py contract line.
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
    ap.add_argument("--single", action="store_true", help="lift the launch cap: one launch of --steps steps")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "langevin", "bench_langevin.json"))
    a = ap.parse_args()
    import torch

    import bench_dynamics as bd
    from normalizingflow_amd import config, rng
    dev = torch.device("cuda", 0)
    if a.single:
        config.LANGEVIN_STEPS_PER_LAUNCH = a.steps
    res = {"tool": "tools/bench_langevin.py", "device": torch.cuda.get_device_name(0), "steps": a.steps,
           "iters": a.iters, "windows": a.windows, "steps_per_launch": config.LANGEVIN_STEPS_PER_LAUNCH,
           "langevin": {}}
    for kind in a.kinds:
        fused, slow = bd.systems_pair(kind, dev)
        kT = bd.KT_FE if kind == "eam" else 1.0
        for rows in a.rows:
            x, v, dt = bd.start(kind, rows, dev)
            n = x.shape[-2]
            kw = dict(dt=dt, kT=kT, seed=1, init_pos=x, init_velocity=v)
            xa, pa = fused.langevin(5, **kw)
            xb, pb = slow.langevin(5, **kw)
            assert torch.equal(xa, xb) and torch.equal(pa, pb) and torch.equal(
                fused.get_velocity(), slow.get_velocity()), "the two paths differ"
            r = bd.windows({"one_launch": lambda: fused.langevin(a.steps, **kw),
                            "per_step": lambda: slow.langevin(a.steps, **kw),
                            "nve_one_launch": lambda: fused.integration_step(a.steps, dt, x, v, scheme="verlet"),
                            "fill_only": lambda: [rng.philox_normal(1, rows, n, 3, k, zero_mean=True, device=dev)
                                                  for k in range(a.steps)]},
                           a.iters, a.windows, ratio=("one_launch", "per_step"))
            r["one_launch_ms_per_step"] = round(r["one_launch"]["median_ms"] / a.steps, 6)
            r["rng_share"] = round(1 - r["nve_one_launch"]["median_ms"] / r["one_launch"]["median_ms"], 4)
            res["langevin"]["%s_rows%d" % (kind, rows)] = r
            print(kind, rows, json.dumps(r), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(json.dumps(res, indent=1) + "\n")
    print(json.dumps(res))
    return 0


if __name__ == "__main__":
    sys.exit(main())
