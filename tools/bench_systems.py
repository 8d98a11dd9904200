#!/usr/bin/env python
"""Kernel and step times of normalizingflow_amd.systems on one GPU.

    python tools/bench_systems.py [--rows 1048576] [--out profiles/systems_bench.json]

Steps (each runs as a child process under its own ``timeout``; the parent
never opens the GPU and stops at the first step that fails):

  einstein  nfk_einstein_logprob (32 x 3) vs the same object on its torch path
            on the GPU vs nfk_normal_logprob at width 96 (the same bytes)
  gmix      nfk_gmix_logprob (20 x 2, M = 2) vs its torch path
  lj        nfk_lj_potential forward and forward + backward (N = 32, cutoff
            1.6) vs the torch path at --torch-rows rows (its [B, N, N, 3]
            temporaries and the autograd copies of them bound the rows)
  step      Einstein.yaml / LJ.yaml's 2-layer NSF_AR log_prob step at 40 rows,
            eager and as a HIP graph replay, with the Einstein prior and with
            the Normal prior

Times are device-event windows (median, min, max over --windows windows of
--iters calls, variants alternated inside one process).  "hbm" figures use the
algorithmic bytes (row read + 4 B written) over the 8.0 TB/s peak.  Not the
bench.py contract line.
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

STEPS = ("einstein", "gmix", "lj", "step")
HBM_PEAK = 8.0e12
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
    return {k: {"median_ms": round(statistics.median(v), 5), "min_ms": round(min(v), 5),
                "max_ms": round(max(v), 5)} for k, v in ms.items()}


def hbm(res, rows, width):
    b = rows * (width * 4 + 4)
    floor_ms = b / HBM_PEAK * 1e3
    res["algorithmic_bytes"] = b
    res["hbm_floor_ms"] = round(floor_ms, 5)
    res["tb_per_s"] = round(b / (res["median_ms"] * 1e-3) / 1e12, 3)
    res["fraction_of_hbm_floor"] = round(floor_ms / res["median_ms"], 3)


def step_einstein(a):
    import torch
    from normalizingflow_amd import kernels as K_, systems
    dev = torch.device("cuda", 0)
    prior = systems.EinsteinCrystal(fcc32(), 3, boxlength=L32, alpha=600, device=dev)
    slow = systems.EinsteinCrystal(fcc32(), 3, boxlength=L32, alpha=600, device=dev)
    slow.use_kernels = False
    x = prior.sample(a.rows)
    out = torch.empty(a.rows, device=dev)
    with torch.no_grad():
        torch.testing.assert_close(prior.log_prob(x), slow.log_prob(x), rtol=1e-5, atol=1e-4)
        r = windows({"nfk_einstein_logprob": lambda: prior._launch(x, out, None, 1, None),
                     "nfk_normal_logprob_w96": lambda: K_.normal_logprob(x, out, scale=0.04, hld=-309.0),
                     "torch_path_same_gpu": lambda: slow.log_prob(x)}, a.iters, a.windows)
    for k in ("nfk_einstein_logprob", "nfk_normal_logprob_w96"):
        hbm(r[k], a.rows, 96)
    return {"rows": a.rows, "natoms": 32, "dim": 3, **r}


def step_gmix(a):
    import torch
    from normalizingflow_amd import systems
    dev = torch.device("cuda", 0)
    mk = lambda: systems.GaussianMixture([[-1, -1], [1, 1]], [0.1, 0.05], 20, 2, device=dev)  # noqa: E731
    prior, slow = mk(), mk()
    slow.use_kernels = False
    x = prior.sample(a.rows)
    out = torch.empty(a.rows, device=dev)
    with torch.no_grad():
        torch.testing.assert_close(prior.log_prob(x), slow.log_prob(x), rtol=1e-5, atol=1e-4)
        r = windows({"nfk_gmix_logprob": lambda: prior._launch(x, out, None, 1, None),
                     "torch_path_same_gpu": lambda: slow.log_prob(x)}, a.iters, a.windows)
    hbm(r["nfk_gmix_logprob"], a.rows, 40)
    r["note"] = "168 MB of rows at 2^20: resident in the 256 MiB Infinity Cache across calls"
    return {"rows": a.rows, "npart": 20, "dim": 2, "ncenters": 2, **r}


def step_lj(a):
    import torch
    from normalizingflow_amd import kernels as K_, systems
    dev = torch.device("cuda", 0)
    lj = systems.LJ(boxlength=L32, cutoff=1.6, device=dev)
    slow = systems.LJ(boxlength=L32, cutoff=1.6, device=dev)
    slow.use_kernels = False
    lat = fcc32().to(dev)

    def positions(rows):
        p = lat + 0.05 * torch.randn(rows, 32, 3, device=dev)
        return p - L32 * torch.floor(p / L32 + 0.5)

    x = positions(a.rows)
    xs = positions(a.torch_rows)
    x2, g = x.reshape(a.rows, 96), torch.ones(a.rows, device=dev)
    out, gx = torch.empty(a.rows, device=dev), torch.empty(a.rows, 96, device=dev)
    kw = lj._kw()
    with torch.no_grad():
        torch.testing.assert_close(lj.potential(xs), slow.potential(xs), rtol=1e-5, atol=2e-3)

    def torch_fwd_bwd():
        xr = xs.detach().requires_grad_()
        slow.potential(xr).sum().backward()

    with torch.no_grad():
        r = windows({"nfk_lj_potential": lambda: K_.lj_potential(x2, out, n=32, dim=3, **kw),
                     "nfk_lj_potential_bwd": lambda: K_.lj_potential_bwd(x2, g, gx, n=32, dim=3, **kw),
                     "torch_path_fwd_same_gpu": lambda: slow.potential(xs)}, a.iters, a.windows)
    r.update(windows({"torch_path_fwd_bwd_same_gpu": torch_fwd_bwd}, max(1, a.iters // 4), a.windows))
    for k in ("nfk_lj_potential", "nfk_lj_potential_bwd"):
        width = 96 if k == "nfk_lj_potential" else 192
        hbm(r[k], a.rows, width)
        r[k]["pair_evaluations_per_s"] = round(a.rows * 1024 / (r[k]["median_ms"] * 1e-3), 0)
    for k in ("torch_path_fwd_same_gpu", "torch_path_fwd_bwd_same_gpu"):
        r[k]["rows"] = a.torch_rows
        r[k]["median_ms_scaled_to_rows"] = round(r[k]["median_ms"] * a.rows / a.torch_rows, 3)
    return {"rows": a.rows, "n": 32, "dim": 3, "cutoff": 1.6, **r}


def step_step(a):
    import torch
    import nf.flows as nff
    import nf.models as nfm
    from normalizingflow_amd import systems
    from normalizingflow_amd.graphs import GraphedLogProb
    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    flows = [nff.NSF_AR(dim=96, K=32, B=L32 / 2, hidden_dim=354) for _ in range(2)]
    ein = systems.EinsteinCrystal(fcc32(), 3, alpha=1000, device=dev)
    normal = torch.distributions.MultivariateNormal(torch.zeros(96, device=dev), torch.eye(96, device=dev))
    m_e = nfm.NormalizingFlowModel(ein, flows).to(dev)
    m_n = nfm.NormalizingFlowModel(normal, flows).to(dev)
    x = ein.sample(40)
    g_e, g_n = GraphedLogProb(m_e, x), GraphedLogProb(m_n, x)
    r = windows({"einstein_prior_eager": lambda: m_e.log_prob(x), "einstein_prior_graph": lambda: g_e(None),
                 "normal_prior_eager": lambda: m_n.log_prob(x), "normal_prior_graph": lambda: g_n(None)},
                a.iters * 5, a.windows)
    return {"rows": 40, "flow": "2 x NSF_AR(96, K=32, hidden 354)", **r}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1 << 20)
    ap.add_argument("--torch-rows", type=int, default=1 << 17, help="rows of the LJ torch path")
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--timeout", type=int, default=240, help="seconds per step")
    ap.add_argument("--out", default=None)
    ap.add_argument("--only", choices=STEPS, default=None)
    a = ap.parse_args()
    if a.only:
        print("RESULT " + json.dumps(globals()["step_" + a.only](a)))
        return 0
    res = {"tool": "tools/bench_systems.py", "rows": a.rows, "iters": a.iters, "windows": a.windows}
    for s in STEPS:
        cmd = ["timeout", "-k", "10", str(a.timeout), sys.executable, os.path.abspath(__file__), "--only", s,
               "--rows", str(a.rows), "--torch-rows", str(a.torch_rows), "--iters", str(a.iters),
               "--windows", str(a.windows)]
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
