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

    python tools/bench_dynamics.py --hmc-run [--out profiles/dynamics/bench_hmc_run.json]

times a whole ``hmc(500)`` (path_len 12, records kept, as ``collect_hmc_data``
calls it) for one chain and 500 chains of the same two systems, again two forms
alternating window by window:

  one_launch  ``hmc(500, one_launch=True)``: bulk draws and ONE nfk_*_hmc_run launch
  per_epoch   the default ``hmc(500)``: a trajectory and a Metropolis launch per
              epoch -- the code as it was before the one-launch kernels, the yardstick

    python tools/bench_dynamics.py --kind eam [--hmc-run] [--out profiles/eam_dynamics_bench.json]

is the same pair of measurements for systems.EAM at the Fe shape of
tools/bench_eam.py (n = 54 perturbed bcc 3 x 3 x 3, rc = 0.61 L, 10^4-point
tables): trajectories of 50, 500, 5,000, 6,144, 7,168 and 2^16 rows, one HMC
epoch and, with --hmc-run, ``hmc(500)`` at 1 and 500 chains.  The fused side
times nfk_eam_trajectory at every size: the row cap above which ``EAM`` itself
takes the per-step path (``EAM._FUSED_ROWS_MAX``, set from these numbers) is
lifted here.  Both invocations write into one file: sections the other one
wrote are kept.
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


def windows(variants, iters, nwin, ratio=("fused", "per_step")):
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
    out["%s_over_%s" % ratio] = round(out[ratio[0]]["median_ms"] / out[ratio[1]]["median_ms"], 4)
    return out


def systems_pair(kind, dev):
    from normalizingflow_amd import systems
    pair = []
    for fused in (True, False):
        if kind == "lj":
            sim = systems.LJ(boxlength=L32, cutoff=1.6, device=dev)
        elif kind == "eam":
            tab, L = bench_eam().tables()
            sim = systems.EAM(tab, L, device=dev)
            sim._FUSED_ROWS_MAX = 1 << 62  # time the launch itself at every size: the class routes by this cap
        else:
            sim = systems.EinsteinCrystal(fcc32(), 3, boxlength=L32, alpha=600, device=dev)
        sim.fused_dynamics = fused
        pair.append(sim)
    return pair


def bench_eam():
    """tools/bench_eam.py as a module: the Fe shape's tables and constants."""
    here = os.path.dirname(os.path.abspath(__file__))
    if here not in sys.path:
        sys.path.insert(0, here)
    import bench_eam as m
    return m


KT_FE = 0.00861733326  # the Fe configs' kT: velocities of sd sqrt(kT), beta = 1 / kT
BETA = {"eam": 1 / KT_FE}
ROWS = {"eam": (50, 500, 5000, 6144, 7168, 1 << 16)}  # 6,144 / 7,168: either side of EAM._FUSED_ROWS_MAX


def start(kind, rows, dev):
    import torch
    g = torch.Generator().manual_seed(rows)
    if kind == "eam":
        import numpy as np
        m = bench_eam()
        c = np.arange(3)
        corner = np.stack(np.meshgrid(c, c, c, indexing="ij"), -1).reshape(-1, 3).astype(np.float64)
        lat = torch.as_tensor(np.concatenate((corner, corner + 0.5)) * m.A_FE, dtype=torch.float32)
        x = lat + 0.08 * torch.randn(rows, m.N, 3, generator=g)
        return x.to(dev), (KT_FE ** 0.5 * torch.randn(rows, m.N, 3, generator=g)).to(dev), 0.005
    lat = fcc32()
    if kind == "lj":
        x = lat + 0.03 * torch.randn(rows, 32, 3, generator=g)
        return x.to(dev), torch.randn(rows, 32, 3, generator=g).to(dev), 0.002
    x = lat.flatten() + torch.randn(rows, 96, generator=g) / 600 ** 0.5
    return x.to(dev), torch.randn(rows, 96, generator=g).to(dev), 0.005


def hmc_run_rows(a, dev):
    """hmc(--epochs) in both forms; the two are first checked against each other on
    a short run: same seed, one epoch per launch so that the draws coincide,
    bit-equal records."""
    import torch
    from normalizingflow_amd.hmc import HMC
    res = {"tool": "tools/bench_dynamics.py --hmc-run", "device": torch.cuda.get_device_name(0),
           "iters": a.iters, "windows": a.windows, "path_len": a.path_len, "epochs": a.epochs, "hmc_run": {}}
    for kind in a.kinds:
        sim, _ = systems_pair(kind, dev)
        for chains in (1, 500):
            x, _, dt = start(kind, chains, dev)
            run = HMC(sim, path_len=a.path_len, dt=dt, beta=BETA.get(kind, 1.0))
            torch.manual_seed(0)
            pa = run.hmc(8, x, one_launch=True, draw_bytes=0)[0]  # one epoch per launch: the default's draw order
            torch.manual_seed(0)
            pb = run.hmc(8, x)[0]
            assert torch.equal(pa, pb), "the two forms differ"
            r = windows({"one_launch": lambda: run.hmc(a.epochs, x, one_launch=True),
                         "per_epoch": lambda: run.hmc(a.epochs, x)}, a.iters, a.windows,
                        ratio=("one_launch", "per_epoch"))
            r["note"] = "one hmc(%d) call with records: start potential, draws, epochs, closing synchronisation" % a.epochs
            res["hmc_run"]["%s_chains%d" % (kind, chains)] = r
            print(kind, "hmc(%d)" % a.epochs, chains, json.dumps(r), flush=True)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=None, help="calls per window (10; --hmc-run: 3)")
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--path-len", type=int, default=12)
    ap.add_argument("--hmc-run", action="store_true", help="time hmc(--epochs) in one launch against per epoch")
    ap.add_argument("--epochs", type=int, default=500)
    ap.add_argument("--kind", choices=("eam",), default=None, help="eam: systems.EAM at the Fe shape alone")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    a.kinds = (a.kind,) if a.kind else ("lj", "einstein")
    if a.iters is None:
        a.iters = 3 if a.hmc_run else 10
    if a.out is None and a.kind:
        a.out = os.path.join(REPO, "profiles", "%s_dynamics_bench.json" % a.kind)
    if a.out is None:
        a.out = os.path.join(REPO, "profiles", "dynamics",
                             "bench_hmc_run.json" if a.hmc_run else "bench_dynamics.json")
    import torch
    from normalizingflow_amd.hmc import HMC
    dev = torch.device("cuda", 0)
    if a.hmc_run:
        return save(a, hmc_run_rows(a, dev), "hmc_run")
    res = {"tool": "tools/bench_dynamics.py", "device": torch.cuda.get_device_name(0), "iters": a.iters,
           "windows": a.windows, "path_len": a.path_len, "trajectory": {}, "hmc_epoch": {}}
    for kind in a.kinds:
        fused, slow = systems_pair(kind, dev)
        for rows in ROWS.get(kind, (500, 5000)):
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
            runs = [HMC(s, path_len=a.path_len, dt=dt, beta=BETA.get(kind, 1.0)) for s in (fused, slow)]
            r = windows({"fused": lambda: runs[0].hmc(1, x, record=False),
                         "per_step": lambda: runs[1].hmc(1, x, record=False)}, a.iters, a.windows)
            r["note"] = "one hmc(1) call: the start potential, one epoch and the closing synchronisation"
            res["hmc_epoch"]["%s_chains%d" % (kind, chains)] = r
            print(kind, "hmc", chains, json.dumps(r), flush=True)
    return save(a, res, "trajectory")


def save(a, res, section):
    """Write res; with --kind, into the kind's one file: the other invocation's
    sections stay, each under the settings it was measured with."""
    if a.kind:
        res = {section + "_bench": {k: v for k, v in res.items() if not isinstance(v, dict)},
               **{k: v for k, v in res.items() if isinstance(v, dict)}}
        if os.path.exists(a.out):
            with open(a.out) as f:
                res = {**json.load(f), **res}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(json.dumps(res, indent=1) + "\n")
    print(json.dumps(res))
    return 0


if __name__ == "__main__":
    sys.exit(main())
