#!/usr/bin/env python
"""Times of the fused trajectory launch (nfk_dynamics.hip) against the per-step
path on one GPU.

    python tools/bench_dynamics.py [--out profiles/dynamics/bench_dynamics.json]

Two paths alternate inside one process, window by window:

  fused     one launch per ``integration_step`` (and nfk_hmc_accept per epoch)
  per_step  ``fused_dynamics = False``: ``get_force`` / ``force`` per step plus
            torch elementwise ops -- only calls the code had before the fused
            launch existed, so it is the earlier cost of the same work

Shapes: LJ-32 (cutoff 1.6) and the Einstein crystal 32 x 3 at 500 and 5,000
rows, path_len 12 (the two launches of ``relaxation_step`` on 500 frames with
npoints 10), and one HMC epoch (path_len 12) at 1 and 500 chains.  Warm-up
precedes the timed windows; times are device-event windows (median, min, max
over --windows windows of --iters calls).  Not the bench.py contract line.
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

L32 = 2.92402


def fcc32():
    import torch
    basis = [(0, 0, 0), (.5, .5, 0), (.5, 0, .5), (0, .5, .5)]
    pts = [((i + b[0]) / 2, (j + b[1]) / 2, (k + b[2]) / 2)
           for i in range(2) for j in range(2) for k in range(2) for b in basis]
    return (torch.tensor(pts, dtype=torch.float64) * L32 - L32 / 2 + L32 / 8).float()


def windows(variants, iters, nwin):
    """{name: fn} -> {name: {median_ms, min_ms, max_ms}} per call; the variants
    alternate inside every window round."""
    import torch
    for fn in variants.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in variants}
    for _ in range(nwin):
        for k, fn in variants.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(iters):
                fn()
            e1.record()
            e1.synchronize()
            ms[k].append(e0.elapsed_time(e1) / iters)
    out = {k: {"median_ms": round(statistics.median(v), 5), "min_ms": round(min(v), 5),
               "max_ms": round(max(v), 5)} for k, v in ms.items()}
    out["fused_over_per_step"] = round(out["fused"]["median_ms"] / out["per_step"]["median_ms"], 4)
    return out


def systems_pair(kind, dev):
    from normalizingflow_amd import systems
    pair = []
    for fused in (True, False):
        if kind == "lj":
            sim = systems.LJ(boxlength=L32, cutoff=1.6, device=dev)
        else:
            sim = systems.EinsteinCrystal(fcc32(), 3, boxlength=L32, alpha=600, device=dev)
        sim.fused_dynamics = fused
        pair.append(sim)
    return pair


def start(kind, rows, dev):
    import torch
    g = torch.Generator().manual_seed(rows)
    lat = fcc32()
    if kind == "lj":
        x = lat + 0.03 * torch.randn(rows, 32, 3, generator=g)
        return x.to(dev), torch.randn(rows, 32, 3, generator=g).to(dev), 0.002
    x = lat.flatten() + torch.randn(rows, 96, generator=g) / 600 ** 0.5
    return x.to(dev), torch.randn(rows, 96, generator=g).to(dev), 0.005


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--path-len", type=int, default=12)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "dynamics", "bench_dynamics.json"))
    a = ap.parse_args()
    import torch
    from normalizingflow_amd.hmc import HMC
    dev = torch.device("cuda", 0)
    res = {"tool": "tools/bench_dynamics.py", "device": torch.cuda.get_device_name(0), "iters": a.iters,
           "windows": a.windows, "path_len": a.path_len, "trajectory": {}, "hmc_epoch": {}}
    for kind in ("lj", "einstein"):
        fused, slow = systems_pair(kind, dev)
        for rows in (500, 5000):
            x, v, dt = start(kind, rows, dev)
            xa, _ = fused.integration_step(a.path_len, dt, x, v)
            xb, _ = slow.integration_step(a.path_len, dt, x, v)
            assert torch.equal(xa, xb), "the two paths differ"
            r = windows({"fused": lambda: fused.integration_step(a.path_len, dt, x, v),
                         "per_step": lambda: slow.integration_step(a.path_len, dt, x, v)}, a.iters, a.windows)
            res["trajectory"]["%s_rows%d" % (kind, rows)] = r
            print(kind, rows, json.dumps(r), flush=True)
        for chains in (1, 500):
            x, _, dt = start(kind, chains, dev)
            runs = [HMC(s, path_len=a.path_len, dt=dt) for s in (fused, slow)]
            r = windows({"fused": lambda: runs[0].hmc(1, x, record=False),
                         "per_step": lambda: runs[1].hmc(1, x, record=False)}, a.iters, a.windows)
            r["note"] = "one hmc(1) call: the start potential, one epoch and the closing synchronisation"
            res["hmc_epoch"]["%s_chains%d" % (kind, chains)] = r
            print(kind, "hmc", chains, json.dumps(r), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(json.dumps(res, indent=1) + "\n")
    print(json.dumps(res))
    return 0


if __name__ == "__main__":
    sys.exit(main())
