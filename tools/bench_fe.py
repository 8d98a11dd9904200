#!/usr/bin/env python
"""Times of the free-energy estimator (nfk_bar.hip, normalizingflow_amd/bar.py)
on one GPU against the two host forms it replaces.

    python tools/bench_fe.py [--out profiles/fe/bench_fe.json]
    python tools/bench_fe.py --mbar [--out profiles/fe/bench_mbar.json]
    python tools/bench_fe.py --metropolize [--out profiles/metropolize_bench.json]

Three forms of the same work alternate inside one process, window by window:

  kernel  ``bar.bar_solve`` / ``bar.bootstrap`` / ``app.fe_estimates`` on fp32
          device tensors: every problem of a call in one nfk_bar launch
  torch   the same calls with ``bar.use_kernels = False``: the fp64 torch
          iteration on the same GPU, one host sync per iteration
  numpy   the work values (or Q) copied to the host, then an fp64 NumPy loop of
          the same iteration; the copy is inside the timed call

Shapes: one solve at n_f = n_r = 500, 2^16 and 2^20; a 200-replica bootstrap at
500 and 2^16; ``fe_estimates`` from a device Q of 2^16 rows.  Work values are
Crooks-consistent Gaussians (dF 37.5, s 2).  Every timed call ends in a device
synchronise and is timed by the host clock (the host forms have no other
clock); the kernel's device-event time is recorded next to it.  Warm-up
precedes the timed windows; median, min and max over --windows windows.  Not
the bench.py contract line.

``--mbar`` times the multistate solver (nfk_mbar.hip, normalizingflow_amd/
mbar.py) instead, by the same method and in the same three forms: one solve and
a 200-replica stratified bootstrap of 500 + 500 samples at K = 2 (the work
values above as two states) and of 4,096 samples of K = 8 states (512 each,
harmonic wells with offsets of 40 per state: N K is the kernel's LDS cap).

``--metropolize`` times ``reweight.metropolis_chain`` alone (nfk_metropolize.hip)
on synthetic energies whose acceptance rate is about 0.05, 0.5 and 1.0 (a
strictly decreasing e: the most rounds per block the kernel can take), at
(chains, proposals) = (1, 2000), (10, 2000), (200, 2000) and (1, 2^20), in three
forms: the kernel; the torch restatement on the same GPU (``use_kernels =
False``); and the reference's per-frame loop on CPU tensors with the energies
precomputed.  The last two are serial in the steps and are timed on at most
2^14 steps (the loop on one chain); the result file holds those times and
their linear scaling to the whole shape, named as such.  Default output:
profiles/metropolize_bench.json.
"""
from __future__ import annotations

import argparse
import json
import math
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)


def numpy_bar(w_f, w_r, delta=0.0, max_iter=1000, rtol=1e-5):
    """The iteration of normalizingflow_amd/bar.py in NumPy fp64: (DeltaF, iterations)."""
    import numpy as np
    n_f, n_r = w_f.size, w_r.size
    M = math.log(n_f / n_r)

    def g(a):
        return -(np.maximum(a, 0.0) + np.log1p(np.exp(-np.abs(a))))

    def lse(t):
        m = t.max()
        return math.log(np.exp(t - m).sum()) + m

    for k in range(max_iter):
        new = (lse(g((M - w_r) - delta) - w_r) - math.log(n_r)) - (lse(g((M + w_f) - delta)) - math.log(n_f))
        stop = new != new or (k > 0 and abs((new - delta) / new) < rtol)
        delta = new
        if stop:
            break
    return delta, k + 1


def numpy_mbar(u, n_k, max_iter=1000, rtol=1e-8):
    """The iteration of normalizingflow_amd/mbar.py in NumPy fp64: (f, iterations)."""
    import numpy as np
    n = np.asarray(n_k, dtype=np.float64)
    logn = np.log(n)

    def weights(f):
        a = (logn + f)[None, :] - u
        e = np.exp(a - a.max(axis=1, keepdims=True))
        return e / e.sum(axis=1, keepdims=True)

    f = np.zeros(len(n))
    for k in range(max_iter):
        W = weights(f)
        S, G = W.sum(axis=0), W.T @ W
        f_sc = f - np.log(S / n)
        f_sc = f_sc - f_sc[0]
        new, H = f_sc, (np.diag(S) - G)[1:, 1:]
        try:
            np.linalg.cholesky(H)
            f_nr = np.concatenate((f[:1], f[1:] - np.linalg.solve(H, (S - n)[1:])))
            if np.all(np.isfinite(f_nr)):
                g_sc, g_nr = weights(f_sc).sum(axis=0) - n, weights(f_nr).sum(axis=0) - n
                if np.dot(g_nr, g_nr) < np.dot(g_sc, g_sc):
                    new = f_nr
        except np.linalg.LinAlgError:
            pass
        stop = np.any(np.isnan(new)) or np.max(np.abs(new - f)) < rtol * np.max(np.abs(new))
        f = new
        if stop:
            break
    return f, k + 1


def timed(variants, nwin, budget_s):
    """{name: fn} -> {name: {median_ms, min_ms, max_ms, calls}}: the variants
    alternate inside every window; a window holds as many calls of a variant as
    fit ``budget_s`` (at least one), fixed after the warm-up."""
    import torch
    calls = {}
    for k, fn in variants.items():
        fn()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        calls[k] = max(1, min(50, int(budget_s / max(time.perf_counter() - t0, 1e-6))))
    ms = {k: [] for k in variants}
    for _ in range(nwin):
        for k, fn in variants.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(calls[k]):
                fn()
                torch.cuda.synchronize()
            ms[k].append((time.perf_counter() - t0) * 1e3 / calls[k])
    return {k: {"median_ms": round(statistics.median(v), 4), "min_ms": round(min(v), 4),
                "max_ms": round(max(v), 4), "calls": calls[k]} for k, v in ms.items()}


def device_ms(fn, reps=5):
    import torch
    fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        out.append(e0.elapsed_time(e1))
    return round(statistics.median(out), 4)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--budget", type=float, default=0.2, help="seconds of calls per variant and window")
    ap.add_argument("--nboot", type=int, default=200)
    ap.add_argument("--mbar", action="store_true", help="time the multistate solver instead")
    ap.add_argument("--metropolize", action="store_true", help="time the Metropolis chain instead")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.out is None and a.metropolize:
        a.out = os.path.join(REPO, "profiles", "metropolize_bench.json")
    if a.out is None:
        a.out = os.path.join(REPO, "profiles", "fe", "bench_mbar.json" if a.mbar else "bench_fe.json")
    import numpy as np
    import torch
    from normalizingflow_amd import app
    from normalizingflow_amd import bar as B
    if not torch.cuda.is_available():
        raise SystemExit("tools/bench_fe.py needs a HIP device")
    dev = torch.device("cuda", 0)
    if a.metropolize:
        return main_metropolize(a, dev)

    def torch_path(fn):
        def run():
            B.use_kernels = False
            try:
                return fn()
            finally:
                B.use_kernels = True
        return run

    def work(n, seed):
        g = torch.Generator().manual_seed(seed)
        w_f = 37.5 + 2.0 + 2.0 * torch.randn(n, generator=g)
        w_r = -37.5 + 2.0 + 2.0 * torch.randn(n, generator=g)
        return w_f.to(dev), w_r.to(dev)

    from normalizingflow_amd import kernels as K_
    if a.mbar:
        return main_mbar(a, dev, work)
    res = {"tool": "tools/bench_fe.py", "device": torch.cuda.get_device_name(0), "windows": a.windows,
           "budget_s": a.budget, "stage_cap": None, "solve": {}, "bootstrap": {}, "fe_estimates": {}}
    res["stage_cap"] = K_.bar_stage_cap()

    for n in (500, 1 << 16, 1 << 20):
        w_f, w_r = work(n, n)
        out, iters = B.bar_solve(w_f, w_r)
        ref, ref_iters = numpy_bar(w_f.cpu().double().numpy(), w_r.cpu().double().numpy())
        t_out, t_iters = torch_path(lambda: B.bar_solve(w_f, w_r))()
        r = timed({"kernel": lambda: B.bar_solve(w_f, w_r),
                   "torch": torch_path(lambda: B.bar_solve(w_f, w_r)),
                   "numpy": lambda: numpy_bar(w_f.cpu().double().numpy(), w_r.cpu().double().numpy())},
                  a.windows, a.budget)
        r["kernel_device_ms"] = device_ms(lambda: B.bar_solve(w_f, w_r))
        r["iterations"] = {"kernel": int(iters[0]), "torch": int(t_iters[0]), "numpy": ref_iters}
        r["kernel_minus_numpy"] = float(out[0, 0]) - ref
        r["torch_minus_numpy"] = float(t_out[0, 0]) - ref
        res["solve"]["n%d" % n] = r
        print("solve", n, json.dumps(r), flush=True)

    for n in (500, 1 << 16):
        w_f, w_r = work(n, n + 1)

        def host_boot():
            f, r_ = w_f.cpu().double().numpy(), w_r.cpu().double().numpy()
            rng = np.random.default_rng(0)
            return [numpy_bar(f[rng.integers(n, size=n)], r_[rng.integers(n, size=n)])[0] for _ in range(a.nboot)]

        gen = torch.Generator(dev).manual_seed(0)
        r = timed({"kernel": lambda: B.bootstrap(w_f, w_r, a.nboot, generator=gen),
                   "torch": torch_path(lambda: B.bootstrap(w_f, w_r, a.nboot, generator=gen)),
                   "numpy": host_boot}, a.windows, a.budget)
        r["kernel_device_ms"] = device_ms(lambda: B.bootstrap(w_f, w_r, a.nboot, generator=gen))
        r["nboot"] = a.nboot
        r["form"] = "staged" if 2 * n <= res["stage_cap"] else "streamed"
        res["bootstrap"]["n%d" % n] = r
        print("bootstrap", n, json.dumps(r), flush=True)

    n = 1 << 16
    w_f, w_r = work(n, 7)
    g = torch.Generator().manual_seed(8)
    q00 = (-150.0 + 5.0 * torch.randn(n, generator=g)).to(dev)
    q11 = (-180.0 + 5.0 * torch.randn(n, generator=g)).to(dev)
    Q = torch.stack((torch.stack((q00, q00 - w_f), 1), torch.stack((q11 - w_r, q11), 1))).contiguous()
    cfg = app.get_cfg_defaults()
    cfg.dataset.nparticles, cfg.dataset.kT = 32, 2.0

    def host_fe():
        q = Q.cpu().numpy()
        s0, s1 = q[1][:, 0].min(), q[1][:, 1].min()
        q = q - np.array([s0, s1], dtype=q.dtype)
        f, r_ = (q[0][:, 0] - q[0][:, 1]).astype(np.float64), (-q[1][:, 0] + q[1][:, 1]).astype(np.float64)
        off = float(s0 - s1)
        lme = [math.log(np.exp(w - w.max()).mean()) + w.max() for w in (f, r_)]
        return tuple((off + v) / 32 * 2.0 for v in (numpy_bar(f, r_)[0], -lme[1], lme[0]))

    ours = [float(v) for v in app.fe_estimates(cfg, Q)]
    host = host_fe()
    r = timed({"kernel": lambda: app.fe_estimates(cfg, Q), "torch": torch_path(lambda: app.fe_estimates(cfg, Q)),
               "numpy": host_fe}, a.windows, a.budget)
    r["kernel_device_ms"] = device_ms(lambda: app.fe_estimates(cfg, Q))
    r["kernel_minus_numpy"] = [o - h for o, h in zip(ours, host)]
    res["fe_estimates"]["rows%d" % n] = r
    print("fe_estimates", n, json.dumps(r), flush=True)

    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(json.dumps(res, indent=1) + "\n")
    print(json.dumps(res))
    return 0


def main_mbar(a, dev, work):
    import numpy as np
    import torch
    from normalizingflow_amd import kernels as K_
    from normalizingflow_amd import mbar as M

    def torch_path(fn):
        def run():
            M.use_kernels = False
            try:
                return fn()
            finally:
                M.use_kernels = True
        return run

    def two_states(n):
        w_f, w_r = work(n, n)
        u = torch.zeros(2 * n, 2, device=dev)
        u[:n, 1] = w_f
        u[n:, 0] = w_r
        return u, [n, n]

    def wells(K, n):
        g = torch.Generator().manual_seed(K * n)
        mu, sig = torch.linspace(0.0, 2.0, K), torch.linspace(1.0, 0.5, K)
        x = (mu.repeat_interleave(n) + sig.repeat_interleave(n) * torch.randn(K * n, generator=g)).double()
        u = 0.5 * ((x[:, None] - mu[None, :].double()) / sig[None, :].double()) ** 2 + 40.0 * torch.arange(K)
        return u.float().to(dev), [n] * K

    res = {"tool": "tools/bench_fe.py --mbar", "device": torch.cuda.get_device_name(0), "windows": a.windows,
           "budget_s": a.budget, "stage_cap": K_.mbar_stage_cap(), "solve": {}, "bootstrap": {}}
    for name, (u, n_k) in (("k2_n500", two_states(500)), ("k8_n4096", wells(8, 512))):
        K, N = len(n_k), sum(n_k)
        form = "staged" if N * K <= res["stage_cap"] else "streamed"
        f, iters, _ = M.mbar_solve(u, n_k)
        ref, ref_iters = numpy_mbar(u.cpu().double().numpy(), n_k)
        t_f, t_iters, _ = torch_path(lambda: M.mbar_solve(u, n_k))()
        r = timed({"kernel": lambda: M.mbar_solve(u, n_k), "torch": torch_path(lambda: M.mbar_solve(u, n_k)),
                   "numpy": lambda: numpy_mbar(u.cpu().double().numpy(), n_k)}, a.windows, a.budget)
        r["kernel_device_ms"] = device_ms(lambda: M.mbar_solve(u, n_k))
        r["iterations"] = {"kernel": int(iters[0]), "torch": int(t_iters[0]), "numpy": ref_iters}
        r["kernel_minus_numpy"] = float((f[0].cpu() - torch.from_numpy(ref)).abs().max())
        r["torch_minus_numpy"] = float((t_f[0].cpu() - torch.from_numpy(ref)).abs().max())
        r["K"], r["N"], r["form"] = K, N, form
        res["solve"][name] = r
        print("solve", name, json.dumps(r), flush=True)

        def host_boot():
            h = u.cpu().double().numpy()
            rng = np.random.default_rng(0)
            offs = np.concatenate(([0], np.cumsum(n_k)[:-1]))
            return [numpy_mbar(h[np.concatenate([o + rng.integers(n, size=n) for o, n in zip(offs, n_k)])], n_k)[0]
                    for _ in range(a.nboot)]

        gen = torch.Generator(dev).manual_seed(0)
        r = timed({"kernel": lambda: M.bootstrap(u, n_k, a.nboot, generator=gen),
                   "torch": torch_path(lambda: M.bootstrap(u, n_k, a.nboot, generator=gen)),
                   "numpy": host_boot}, a.windows, a.budget)
        r["kernel_device_ms"] = device_ms(lambda: M.bootstrap(u, n_k, a.nboot, generator=gen))
        r["nboot"], r["K"], r["N"], r["form"] = a.nboot, K, N, form
        res["bootstrap"][name] = r
        print("bootstrap", name, json.dumps(r), flush=True)

    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(json.dumps(res, indent=1) + "\n")
    print(json.dumps(res))
    return 0


def reference_chain(e, r):
    """The per-frame loop of applications/src/utils.py:86-99 on CPU tensors, with
    the energies precomputed (its energy call per frame is not part of this
    measurement): one 0-d tensor operation and one host comparison per step."""
    import torch
    energy, n = e[0], 0
    for i in range(len(e)):
        if r[i] < torch.exp(energy - e[i]):
            energy = e[i]
            n += 1
    return n


def main_metropolize(a, dev):
    import torch
    from normalizingflow_amd import reweight as R

    PREFIX = 1 << 14  # the torch path and the reference loop are timed on at most this many steps

    def torch_path(fn):
        def run():
            R.use_kernels = False
            try:
                return fn()
            finally:
                R.use_kernels = True
        return run

    def energies(C, N, rate, seed):
        """fp32 energies whose energy-only chain accepts at about ``rate``:
        i.i.d. N(0, s^2) accepts at 2 Phi(-s / sqrt 2) once stationary (s 0.954:
        0.5, s 2.772: 0.05); strictly decreasing accepts every step."""
        g = torch.Generator().manual_seed(seed)
        if rate == 1.0:
            e = -(torch.arange(N, dtype=torch.float32) / 64.0).expand(C, N).contiguous()
        else:
            e = {0.5: 0.954, 0.05: 2.772}[rate] * torch.randn(C, N, generator=g)
        return e, torch.rand(C, N, generator=g)

    res = {"tool": "tools/bench_fe.py --metropolize", "device": torch.cuda.get_device_name(0), "windows": a.windows,
           "budget_s": a.budget, "prefix_steps": PREFIX, "shapes": {}}
    for C, N in ((1, 2000), (10, 2000), (200, 2000), (1, 1 << 20)):
        for rate in (0.05, 0.5, 1.0):
            e, r = energies(C, N, rate, C + N)
            de, dr = e.to(dev), r.to(dev)
            n = min(N, PREFIX)
            pe, pr = de[:, :n].contiguous(), dr[:, :n].contiguous()
            ce, cr = e[0, :n].contiguous(), r[0, :n].contiguous()
            state, accepted, naccept, _ = R.metropolis_chain(de, dr)
            t = timed({"kernel": lambda: R.metropolis_chain(de, dr),
                       "torch": torch_path(lambda: R.metropolis_chain(pe, pr)),
                       "reference_loop": lambda: reference_chain(ce, cr)}, a.windows, a.budget)
            row = {"C": C, "N": N, "target_rate": rate, "acceptance": round(float(naccept.double().mean()) / N, 4),
                   "kernel": t["kernel"], "kernel_device_ms": device_ms(lambda: R.metropolis_chain(de, dr)),
                   # the torch path on the first `steps` steps of all C chains; the reference loop on the
                   # first `steps` steps of ONE chain.  Both are serial in the steps, the loop in the chains
                   # too: the *_scaled_ms entries are the medians times N / steps (and times C)
                   "torch": dict(t["torch"], steps=n), "reference_loop": dict(t["reference_loop"], steps=n, chains=1)}
            row["torch_scaled_ms"] = round(t["torch"]["median_ms"] * N / n, 3)
            row["reference_loop_scaled_ms"] = round(t["reference_loop"]["median_ms"] * N / n * C, 3)
            row["kernel_over_torch"] = round(row["torch_scaled_ms"] / t["kernel"]["median_ms"], 1)
            row["kernel_over_reference_loop"] = round(row["reference_loop_scaled_ms"] / t["kernel"]["median_ms"], 1)
            res["shapes"]["c%d_n%d_rate%g" % (C, N, rate)] = row
            print("metropolize", C, N, rate, json.dumps(row), flush=True)

    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(json.dumps(res, indent=1) + "\n")
    print(json.dumps(res))
    return 0


if __name__ == "__main__":
    sys.exit(main())
