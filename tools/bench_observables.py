#!/usr/bin/env python
"""Times of observables.pair_histogram (nfk_pair_hist.hip) on one GPU.

    python tools/bench_observables.py [--out profiles/pair_hist_bench.json]

Shapes: LJ, n = 32 (fcc 2 x 2 x 2 at rho = 0.8, 0.08 of jitter) at 2,000, 2^16 and
2^20 rows; Fe, n = 54 (bcc 3 x 3 x 3, a = 2.8841, 0.08 of jitter) at 2,000 and
2^16 rows; 100 bins up to half the box.  Each shape is a child process under
its own ``timeout``; the parent never opens the GPU and stops at the first step
that fails.  Per step, alternated inside every window round:

  kernel              pair_histogram on the kernel, unit weights (both launches
                      and the workspace allocation: the public call)
  kernel_weighted     the same with one fp64 weight per row
  torch_path          the module's chunked torch restatement on the same GPU
  torch_path_weighted the same with weights
  cdist_histc         torch.cdist + torch.histc over the [B, n, n] distances,
                      where that temporary stays below --cdist-bytes: what a user
                      writes today.  It applies no minimum image and no weights,
                      and counts every pair twice; it is here as a time only.

Times are device-event windows (median, min, max over --windows windows).  With
them: pairs per second and the share of a VALU floor, the fp32 lane-instructions
one pair needs (OPS_PAIR, counted from the kernel's expressions with sqrt as ONE
instruction) over 78.6e12 lane-instructions/s (256 CUs x 4 SIMDs x 32 lanes x
2.4 GHz).  Not the bench.py contract line.
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

VALU_PEAK = 256 * 4 * 32 * 2.4e9
# 3 subtractions, 3 x (mul, rint, mul, sub), 3 mul + 2 add, sqrt, compare, mul, cvt, compare
OPS_PAIR = 25
NBINS = 100
STEPS = {"lj_2000": ("lj", 2000), "lj_65536": ("lj", 1 << 16), "lj_1048576": ("lj", 1 << 20),
         "fe_2000": ("fe", 2000), "fe_65536": ("fe", 1 << 16)}


def lattice(kind):
    import numpy as np
    if kind == "lj":
        cells, a = 2, (4 / 0.8) ** (1 / 3)
        basis = np.array([[0, 0, 0], [0.5, 0.5, 0], [0.5, 0, 0.5], [0, 0.5, 0.5]])
    else:
        cells, a = 3, 2.8841
        basis = np.array([[0, 0, 0], [0.5, 0.5, 0.5]])
    g = np.arange(cells)
    corner = np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3).astype(np.float64)
    return np.concatenate([corner + b for b in basis]) * a, cells * a


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


def step(kind, rows, a):
    import torch
    from normalizingflow_amd import observables as O
    dev = torch.device("cuda", 0)
    sites, L = lattice(kind)
    n = len(sites)
    torch.manual_seed(0)
    x = torch.as_tensor(sites, dtype=torch.float32, device=dev) + 0.08 * torch.randn(rows, n, 3, device=dev)
    w = torch.rand(rows, dtype=torch.float64, device=dev) + 0.5
    r_max = 0.5 * L

    def kernel(weights=None):
        return O.pair_histogram(x, L, r_max, NBINS, weights=weights)[0]

    def torch_path(weights=None):
        O.use_kernels = False
        try:
            return O.pair_histogram(x, L, r_max, NBINS, weights=weights)[0]
        finally:
            O.use_kernels = True

    def cdist_histc():
        return torch.histc(torch.cdist(x, x), bins=NBINS, min=0.0, max=r_max)

    # fp32 distances on both paths: a pair within an ulp of an edge may sit one bin apart
    hk, ht = kernel(), torch_path()
    pairs = rows * n * (n - 1) // 2
    assert float((hk - ht).abs().sum()) <= 1e-4 * pairs and 0 < float(hk.sum()) <= pairs, (hk.sum(), ht.sum())
    assert torch.equal(hk, kernel())
    torch.testing.assert_close(kernel(w), torch_path(w), rtol=1e-3, atol=1e-4 * pairs)
    variants = {"kernel": (kernel, a.iters), "kernel_weighted": (lambda: kernel(w), a.iters),
                "torch_path": (torch_path, a.torch_iters), "torch_path_weighted": (lambda: torch_path(w), a.torch_iters)}
    if rows * n * n * 4 <= a.cdist_bytes:
        variants["cdist_histc"] = (cdist_histc, a.torch_iters)
    r = windows(variants, a.windows)
    for k in ("kernel", "kernel_weighted"):
        sec = r[k]["median_ms"] * 1e-3
        r[k].update(pairs_per_s=round(pairs / sec, 0), share_of_valu_floor=round(pairs * OPS_PAIR / VALU_PEAK / sec, 4))
    r["kernel_over_torch_path"] = round(r["torch_path"]["median_ms"] / r["kernel"]["median_ms"], 1)
    r["kernel_over_torch_path_weighted"] = round(r["torch_path_weighted"]["median_ms"]
                                                 / r["kernel_weighted"]["median_ms"], 1)
    if "cdist_histc" in r:
        r["kernel_over_cdist_histc"] = round(r["cdist_histc"]["median_ms"] / r["kernel"]["median_ms"], 1)
    return {"system": kind, "rows": rows, "n": n, "nbins": NBINS, "box": round(L, 6), "pairs": pairs,
            "pairs_in_range": int(hk.sum()), **r}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20, help="kernel calls per window")
    ap.add_argument("--torch-iters", type=int, default=1, help="torch-path calls per window")
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--timeout", type=int, default=200, help="seconds per step")
    ap.add_argument("--cdist-bytes", type=int, default=1 << 30, help="largest [B, n, n] fp32 temporary to time")
    ap.add_argument("--out", default=None)
    ap.add_argument("--only", choices=sorted(STEPS), default=None)
    a = ap.parse_args()
    if a.only:
        print("RESULT " + json.dumps(step(*STEPS[a.only], a)))
        return 0
    res = {"tool": "tools/bench_observables.py", "iters": a.iters, "torch_iters": a.torch_iters,
           "windows": a.windows, "ops_per_pair": OPS_PAIR}
    for s in STEPS:
        cmd = ["timeout", "-k", "10", str(a.timeout), sys.executable, os.path.abspath(__file__), "--only", s,
               "--iters", str(a.iters), "--torch-iters", str(a.torch_iters), "--windows", str(a.windows),
               "--cdist-bytes", str(a.cdist_bytes)]
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
