"""Generate the ``mbar_*`` golden vectors of the multistate solver
(normalizingflow_amd/mbar.py, nfk_mbar.hip) with an independent fp64 NumPy
statement of its algorithm, pinned by two outside references:

    python tests/golden/make_mbar_golden.py

``mbar_k2_<case>.npz`` -- the K = 2 view of the work values of
``fe_bar_<case>.npz``: ``u[:n_f] = (0, w_f)``, ``u[n_f:] = (w_r, 0)``, N_k =
(n_f, n_r).  The energies are not stored again (``meta["source"]`` names the
fixture; tests/test_mbar_cpu.py rebuilds u).  The MBAR fixed point of two
states is the BAR root, so the expected f_1 is that fixture's ``root_64``,
which the reference's bar.py produced; the generator asserts that the NumPy
solver, run to relative tolerance 1e-13, lands within the tolerance below.

``mbar_k<K>_wells.npz``, K = 3, 5, 8 -- harmonic wells: state k has centre
2 k / (K - 1), width 1 - 0.5 k / (K - 1) and offset 40 k, N_k = 100 + 29 ((3 k +
1) mod 7) samples drawn from its own Gaussian, ``u`` [N, K] cast to fp32.  The
expected f (``f_bfgs``) is a SciPy BFGS minimum of the convex MBAR objective
in fp64, started at the offsets; ``bfgs_err`` = ||H_r^{-1} g_r||_inf there is
its own first-order distance from the root, asserted below 1e-9.

Every case records the solver's fp64 iterate history ``hist_64`` [iters, K]
from f = 0 at relative tolerance 1e-8, ``iters_64``, the Gram matrix
``gram_64`` at the last iterate, the root ``f_root`` (tolerance 1e-13) and

    kappa = max over iterates of ||H_r^{-1}||_inf max_k N_k

taken over the iterates at which the Newton candidate was valid and chosen:
where the self-consistent candidate is chosen H_r^{-1} does not enter the
iterate (from f = 0 with offsets of 40 per state it is of order e^40, and no
figure derived from it would bound anything), and the self-consistent map does
not amplify.  ``picks`` holds the choices (1 = Newton).

Asserted per case, so that no knife-edge decides a count or a choice: at the
stop the relative change is below rtol / 2 and the one before it is above
2 rtol; at every iteration the two candidates' gradient norms differ by more
than 1e-3 relative (or the candidates themselves coincide to a few ulps, as
they do at the last iterate of the one-sample case, where the choice changes
nothing).  The wells are redrawn until they meet both (``SEEDS``).  The K = 2
work values are given and so is the tolerance: ``n500_d37`` stops at a relative
change of 9.73e-9, inside the factor 2, and is kept on a measured ground
instead: reordering its samples moves that figure by 4e-16, a 10^-6th of its
distance from the tolerance.

Tolerance of the tests: tol = 64 N 2^-53 max(1, max|f|) max(1, kappa).
"""
from __future__ import annotations

import io
import json
import os
import sys
import zipfile

import numpy as np
from scipy.optimize import minimize
from scipy.special import logsumexp

HERE = os.path.dirname(os.path.abspath(__file__))
sys.dont_write_bytecode = True
sys.path.insert(0, os.path.dirname(HERE))

import golden_io as gio  # noqa: E402

RTOL = 1.0e-8


def _save(name, meta, arrays):
    """np.savez_compressed's layout with fixed entry timestamps."""
    out = {"meta": np.array(json.dumps(meta, sort_keys=True))}
    out.update({k: np.asarray(v) for k, v in arrays.items()})
    path = os.path.join(HERE, name + ".npz")
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as z:
        for k, v in out.items():
            buf = io.BytesIO()
            np.lib.format.write_array(buf, v, allow_pickle=False)
            info = zipfile.ZipInfo(k + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o644 << 16
            z.writestr(info, buf.getvalue())
    print("wrote", path, os.path.getsize(path), "bytes")


def weights(u, n, f):
    a = (np.log(n) + f)[None, :] - u
    e = np.exp(a - a.max(axis=1, keepdims=True))
    return e / e.sum(axis=1, keepdims=True)


def grad_norm(u, n, f):
    g = weights(u, n, f).sum(axis=0) - n
    return float(np.dot(g, g))


def solve(u, n, rtol, max_iter=1000):
    """The adaptive iteration: (history, relative changes, picks, kappa, norm ratios)."""
    K = len(n)
    f = np.zeros(K)
    hist, rcs, picks, kappas, ratios = [], [], [], [], []
    for _ in range(max_iter):
        W = weights(u, n, f)
        S, G = W.sum(axis=0), W.T @ W
        f_sc = f - np.log(S / n)
        f_sc = f_sc - f_sc[0]
        H = (np.diag(S) - G)[1:, 1:]
        valid = bool(np.all(np.isfinite(H)))
        if valid:
            try:
                np.linalg.cholesky(H)
                f_nr = np.concatenate((f[:1], f[1:] - np.linalg.solve(H, (S - n)[1:])))
                valid = bool(np.all(np.isfinite(f_nr)))
            except np.linalg.LinAlgError:
                valid = False
        n_sc = grad_norm(u, n, f_sc)
        take = False
        if valid:
            n_nr = grad_norm(u, n, f_nr)
            take = n_nr < n_sc
            # two candidates that coincide to a few ulps give the same iterate whichever is taken
            same = np.max(np.abs(f_nr - f_sc)) <= 8 * 2.0 ** -53 * max(1.0, np.max(np.abs(f_sc)))
            ratios.append(1.0 if same else abs(n_nr - n_sc) / max(n_nr, n_sc))
        new = f_nr if take else f_sc
        if take:
            kappas.append(float(np.abs(np.linalg.inv(H)).sum(axis=1).max() * n.max()))
        picks.append(int(take))
        rcs.append(float(np.max(np.abs(new - f))) / float(np.max(np.abs(new))))
        hist.append(new)
        f = new
        if rcs[-1] < rtol:
            break
    return np.array(hist), rcs, picks, max(kappas) if kappas else 0.0, ratios


def tol_of(N, f, kappa):
    return 64 * N * 2.0 ** -53 * max(1.0, float(np.abs(f).max())) * max(1.0, kappa)


def arrays_of(u32, n_k, given=False):
    u = u32.astype(np.float64)
    n = np.asarray(n_k, dtype=np.float64)
    hist, rcs, picks, kappa, ratios = solve(u, n, RTOL)
    edge = not (rcs[-1] < RTOL / 2 and (len(rcs) < 2 or rcs[-2] > 2 * RTOL))
    assert given or not edge, "knife-edge stop: %r" % (rcs[-2:],)
    if edge:
        # The work values and the tolerance are both given, so a case cannot be redrawn.  It is
        # kept if summation order cannot move its count: with the samples reversed and in three
        # random orders the last two relative changes move by less than a thousandth of their
        # distance from the tolerance.
        moved = 0.0
        for order in [np.arange(len(u))[::-1]] + [np.random.default_rng(s).permutation(len(u)) for s in (1, 2, 3)]:
            other = solve(u[order], n, RTOL)[1]
            assert len(other) == len(rcs)
            moved = max(moved, abs(other[-1] - rcs[-1]), abs(other[-2] - rcs[-2]))
        margin = min(RTOL - rcs[-1], rcs[-2] - RTOL)
        print("  stop within a factor 2 of rtol: rc %r, margin %.3g, moved by order %.3g" % (rcs[-2:], margin, moved))
        assert margin > 1000 * moved, "knife-edge stop: %r" % (rcs[-2:],)
    assert all(r > 1e-3 for r in ratios), "knife-edge choice: %r" % (ratios,)
    root = solve(u, n, 1.0e-13)[0][-1]
    W = weights(u, n, hist[-1])
    print("  iters %d picks %s kappa %.3g tol %.3g |last - root| %.3g" % (
        len(hist), "".join("SN"[p] for p in picks), kappa, tol_of(len(u), hist[-1], kappa),
        np.abs(hist[-1] - root).max()))
    return dict(n_k=np.asarray(n_k, dtype=np.int64), hist_64=hist, iters_64=np.int32(len(hist)),
                picks=np.asarray(picks, dtype=np.int32), gram_64=W.T @ W, kappa=np.float64(kappa), f_root=root)


def case_k2(name):
    meta, d, _ = gio.load(name)
    w_f, w_r = d["w_f"].numpy(), d["w_r"].numpy()
    n_f, n_r = w_f.size, w_r.size
    u = np.zeros((n_f + n_r, 2), dtype=np.float32)
    u[:n_f, 1] = w_f
    u[n_f:, 0] = w_r
    print("mbar_k2_" + name[len("fe_bar_"):])
    arr = arrays_of(u, (n_f, n_r), given=True)
    root_64 = float(d["root_64"])
    err = abs(arr["f_root"][1] - root_64)
    tol = tol_of(n_f + n_r, arr["f_root"], float(arr["kappa"]))
    print("  |f_root - BAR root_64| %.3g" % err)
    assert err <= tol, (err, tol)
    arr["root_64"] = np.float64(root_64)
    arr["bar_root_err"] = np.float64(abs(float(d["bar_64"]) - root_64))
    _save("mbar_k2_" + name[len("fe_bar_"):], dict(kind="mbar", K=2, source=name, rtol=RTOL, numpy=np.__version__),
          arr)


def case_wells(K, seed):
    rng = np.random.default_rng(seed)
    mu, sig = np.linspace(0.0, 2.0, K), np.linspace(1.0, 0.5, K)
    n_k = [100 + 29 * ((3 * k + 1) % 7) for k in range(K)]
    x = np.concatenate([rng.normal(mu[k], sig[k], n_k[k]) for k in range(K)])
    u32 = (0.5 * ((x[:, None] - mu[None, :]) / sig[None, :]) ** 2 + 40.0 * np.arange(K)[None, :]).astype(np.float32)
    print("mbar_k%d_wells" % K, n_k)
    arr = arrays_of(u32, n_k)
    u, n = u32.astype(np.float64), np.asarray(n_k, dtype=np.float64)

    def full(fr):
        return np.concatenate(([0.0], fr))

    def obj(fr):
        return logsumexp((np.log(n) + full(fr))[None, :] - u, axis=1).sum() - (n * full(fr)).sum()

    def grad(fr):
        return (weights(u, n, full(fr)).sum(axis=0) - n)[1:]

    r = minimize(obj, 40.0 * np.arange(1, K), jac=grad, method="BFGS", options=dict(gtol=1e-9))
    for _ in range(3):  # BFGS stalls on precision loss; a restart from its result rebuilds the metric
        if np.abs(grad(r.x)).max() >= 1e-9:
            r = minimize(obj, r.x, jac=grad, method="BFGS", options=dict(gtol=1e-9))
    W = weights(u, n, full(r.x))
    H = (np.diag(W.sum(axis=0)) - W.T @ W)[1:, 1:]
    bfgs_err = float(np.abs(np.linalg.solve(H, grad(r.x))).max())
    print("  BFGS: |grad| %.3g, own error %.3g, |f_root - f_bfgs| %.3g" % (
        np.abs(grad(r.x)).max(), bfgs_err, np.abs(arr["f_root"][1:] - r.x).max()))
    assert bfgs_err < 1e-9 and np.abs(grad(r.x)).max() < 1e-6
    assert np.abs(arr["f_root"][1:] - r.x).max() <= tol_of(len(u), arr["f_root"], float(arr["kappa"])) + 2 * bfgs_err
    arr.update(u=u32, f_bfgs=full(r.x), bfgs_err=np.float64(bfgs_err))
    _save("mbar_k%d_wells" % K, dict(kind="mbar", K=K, seed=seed, rtol=RTOL, numpy=np.__version__), arr)


def main():
    for name in gio.names("fe_bar_"):
        case_k2(name)
    for K in (3, 5, 8):
        case_wells(K, SEEDS[K])


# the first seeds from 1 upwards at which a case meets the asserted conditions
SEEDS = {3: 1, 5: 1, 8: 10}

if __name__ == "__main__":
    main()
