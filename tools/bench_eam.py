#!/usr/bin/env python
"""Kernel times of systems.EAM (nfk_eam.hip) on one GPU at the Fe shape.

    python tools/bench_eam.py [--out profiles/eam_bench.json]

n = 54 (bcc 3 x 3 x 3, a = 2.8841, 0.08 of jitter), rc / L = 0.61, synthetic
Finnis-Sinclair-shaped setfl tables of 10^4 points.  Two steps, 2,000 rows (the
reference's fe.py sample count) and 2^16 rows, each a child process under its
own ``timeout``; the parent never opens the GPU and stops at the first step
that fails.  Per step, alternated inside every window round:

  nfk_eam_potential       the energy kernel
  nfk_eam_potential_bwd   the gradient kernel (both of its (j, s) loops)
  torch_path_fwd          the module's fp32 torch path on the same GPU
  torch_path_force        its ``force`` (autograd through the torch path)

Times are device-event windows (median, min, max over --windows windows).
Reported with them: the counted (j, s) terms per second (0 < r <= rc, counted
on the host from the rows), the visited candidates per second, and the shares
of two floors.  The HBM floor is the algorithmic bytes (row read, 4 B or a row
written) over 8.0 TB/s.  The VALU floor is the fp32 lane-instructions the
expressions need -- OPS_* below, counted from nfk_systems_dev.h with a
correctly rounded sqrt and division as ONE instruction each, so the floor is
an ideal the compiled code cannot reach -- over 78.6e12 lane-instructions/s
(256 CUs x 4 SIMDs x 32 lanes x 2.4 GHz).  Not the bench.py contract line.
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

HBM_PEAK = 8.0e12
VALU_PEAK = 256 * 4 * 32 * 2.4e9
A_FE, N = 2.8841, 54
# fp32 lane-instructions per term, without contraction (a cubic is 3 mul + 3 add)
OPS_CANDIDATE = 7    # shift, component, square, r2, the two pre-filters
OPS_COUNTED_FWD = 25  # sqrt, range, lookup index and p (9); f and z cubics (12); 1/r, phi, two sums
OPS_COUNTED_RHO = 16  # the backward's first loop: lookup (9), f's cubic (6), one sum
OPS_COUNTED_FORCE = 42  # lookup (9), z, z', f' (18), 1/r and phi (2), phi' and w (7), three mul + add
STEPS = {"rows_2000": 2000, "rows_65536": 1 << 16}


def tables(npts=10000):
    import numpy as np
    L = 3 * A_FE
    rc = 0.61 * L
    d, c = rc, rc * 3.4 / 3.7
    dr, drho = rc / (npts - 1), 900.0 / (npts - 1)
    r, rho = dr * np.arange(npts), drho * np.arange(npts)
    f = np.where(r < d, (r - d) ** 2 - 0.9 * (r - d) ** 3 / d, 0.0)
    z = np.where(r < c, r * (r - c) ** 2 * (1.2 - 0.6 * r + 0.09 * r * r), 0.0)
    return dict(nrho=npts, drho=drho, nr=npts, dr=dr, rc=rc, F=-1.9 * np.sqrt(rho), f=f, z=z), L


def windows(variants, nwin):
    """{name: (fn, iters)} -> {name: {median_ms, min_ms, max_ms}} per call; the
    variants alternate inside every window round."""
    import torch
    for fn, _ in variants.values():
        for _ in range(2):
            fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in variants}
    for _ in range(nwin):
        for k, (fn, iters) in variants.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(iters):
                fn()
            e1.record()
            e1.synchronize()
            ms[k].append(e0.elapsed_time(e1) / iters)
    return {k: {"median_ms": round(statistics.median(v), 5), "min_ms": round(min(v), 5),
                "max_ms": round(max(v), 5)} for k, v in ms.items()}


def counted_terms_per_row(eam, x):
    """Mean number of (i, j, s) with 0 < r <= rc over the rows of x (fp64 on the device)."""
    import torch
    x = x.double()
    d = x.unsqueeze(-2) - x.unsqueeze(-3)
    L = eam.box
    comp = [d[..., a] - L[a] * torch.round(d[..., a] / L[a]) for a in range(3)]
    total = 0
    for sx in range(-eam.nshift[0], eam.nshift[0] + 1):
        for sy in range(-eam.nshift[1], eam.nshift[1] + 1):
            for sz in range(-eam.nshift[2], eam.nshift[2] + 1):
                r2 = (comp[0] + sx * L[0]) ** 2 + (comp[1] + sy * L[1]) ** 2 + (comp[2] + sz * L[2]) ** 2
                total += int(((r2 > 0) & (r2 <= eam.rc ** 2)).sum())
    return total / x.shape[0]


def step(rows, a):
    import math
    import numpy as np
    import torch
    from normalizingflow_amd import kernels as K_
    from normalizingflow_amd import systems
    dev = torch.device("cuda", 0)
    tab, L = tables()
    eam = systems.EAM(tab, L, device=dev)
    slow = systems.EAM(tab, L, device=dev)
    slow.use_kernels = False
    g = np.arange(3)
    corner = np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3).astype(np.float64)
    lat = torch.as_tensor(np.concatenate((corner, corner + 0.5)) * A_FE, dtype=torch.float32, device=dev)
    torch.manual_seed(0)
    x = lat + 0.08 * torch.randn(rows, N, 3, device=dev)
    x2, gw = x.reshape(rows, 3 * N), torch.ones(rows, device=dev)
    out, gx = torch.empty(rows, device=dev), torch.empty(rows, 3 * N, device=dev)
    kw = eam._kw(dev)
    with torch.no_grad():
        torch.testing.assert_close(eam.potential(x[:256]), slow.potential(x[:256]), rtol=1e-5, atol=2e-3)
    torch.testing.assert_close(eam.force(x[:256]), slow.force(x[:256]), rtol=1e-4, atol=1e-3)
    counted = counted_terms_per_row(eam, x[:256])
    # the shifts one lane walks per axis: nfk_systems_dev.h eam_const
    cand = N * N * math.prod(min(2 * n + 1, int(math.floor(2 * eam.rc * (1 + 1e-5) / b + 2e-4)) + 1)
                             for n, b in zip(eam.nshift, eam.box))
    with torch.no_grad():
        r = windows({"nfk_eam_potential": (lambda: K_.eam_potential(x2, out, n=N, **kw), a.iters),
                     "nfk_eam_potential_bwd": (lambda: K_.eam_potential_bwd(x2, gw, gx, n=N, **kw), a.iters),
                     "torch_path_fwd": (lambda: slow.potential(x), a.torch_iters),
                     "torch_path_force": (lambda: slow.force(x), a.torch_iters)}, a.windows)
    for k, loops, ops, width in (("nfk_eam_potential", 1, OPS_COUNTED_FWD, 3 * N),
                                 ("nfk_eam_potential_bwd", 2, OPS_COUNTED_RHO + OPS_COUNTED_FORCE, 6 * N)):
        sec = r[k]["median_ms"] * 1e-3
        valu_s = rows * (loops * cand * OPS_CANDIDATE + counted * ops) / VALU_PEAK
        hbm_s = rows * (width * 4 + 4) / HBM_PEAK
        r[k].update(counted_terms_per_s=round(rows * counted * loops / sec, 0),
                    visited_terms_per_s=round(rows * cand * loops / sec, 0),
                    valu_floor_ms=round(valu_s * 1e3, 5), share_of_valu_floor=round(valu_s / sec, 4),
                    hbm_floor_ms=round(hbm_s * 1e3, 6), share_of_hbm_floor=round(hbm_s / sec, 5))
    r["kernel_over_torch_fwd"] = round(r["torch_path_fwd"]["median_ms"] / r["nfk_eam_potential"]["median_ms"], 1)
    r["kernel_over_torch_force"] = round(r["torch_path_force"]["median_ms"]
                                         / r["nfk_eam_potential_bwd"]["median_ms"], 1)
    return {"rows": rows, "n": N, "rc_over_L": 0.61, "table_points": 10000, "nshift": list(eam.nshift),
            "counted_terms_per_row": counted, "visited_terms_per_row_per_loop": cand, **r}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50, help="kernel calls per window")
    ap.add_argument("--torch-iters", type=int, default=1, help="torch-path calls per window")
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--timeout", type=int, default=280, help="seconds per step")
    ap.add_argument("--out", default=None)
    ap.add_argument("--only", choices=sorted(STEPS), default=None)
    a = ap.parse_args()
    if a.only:
        print("RESULT " + json.dumps(step(STEPS[a.only], a)))
        return 0
    res = {"tool": "tools/bench_eam.py", "iters": a.iters, "torch_iters": a.torch_iters, "windows": a.windows,
           "ops_per_term": {"candidate": OPS_CANDIDATE, "counted_fwd": OPS_COUNTED_FWD,
                            "counted_bwd": OPS_COUNTED_RHO + OPS_COUNTED_FORCE}}
    for s in STEPS:
        cmd = ["timeout", "-k", "10", str(a.timeout), sys.executable, os.path.abspath(__file__), "--only", s,
               "--iters", str(a.iters), "--torch-iters", str(a.torch_iters), "--windows", str(a.windows)]
        p = subprocess.run(cmd, capture_output=True, text=True)
        line = [ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")]
        if p.returncode != 0 or not line:
            res[s] = {"failed": p.returncode, "stderr": p.stderr[-2000:]}
            print(json.dumps(res))
            return 1  # nothing more is started on the GPU after a failed step
        res[s] = json.loads(line[-1][7:])
    text = json.dumps(res, indent=1)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")
    print(json.dumps(res))
    return 0


if __name__ == "__main__":
    sys.exit(main())
