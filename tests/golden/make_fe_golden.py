"""Generate the ``fe_*`` golden vectors from the REFERENCE's BAR estimator
(applications/src/bar.py).

Run in the build container (where /root/reference exists):

    python tests/golden/make_fe_golden.py

The reference's bar.py is imported from the reference tree, nothing of it is
altered and no bytecode is written.  Outputs, in golden_io.load's format and
arrays only (the archives are written with fixed timestamps, so a second run
reproduces them byte for byte):

``tests/golden/fe_bar_<case>.npz`` -- fp32 work values ``w_f`` / ``w_r``, drawn
as Crooks-consistent Gaussians w_F ~ N(dF + s^2/2, s), w_R ~ N(-dF + s^2/2, s);
the reference's ``BAR(w_f, w_r)`` on the fp32 arrays as run here (``bar_ref``;
the NumPy version, whose promotion rules decide that run's precision, is in
``meta``) and on the arrays cast to fp64 (``bar_64``); the fp64 iterate history
``hist_64`` (every iterate up to the stop) and its length ``iters_64``; the
root converged with relative_tolerance 1e-13 (``root_64``); and the fp64
``lme_f_64`` / ``lme_r_64`` = log mean exp(w).

The generator asserts, per case: in the fp64 run the relative change at the
stopping iteration is below rtol / 2 and the one before it is above 2 rtol (no
knife-edge decides an iteration count); every exponent |a| the iteration meets
stays below 600 (the reference's overflow-prone form is finite); successive
differences of ``hist_64`` shrink by a factor of at most 0.5 per step.

``tests/golden/fe_q_lj.npz`` -- a [2, 64, 2] fp32 ``Q`` with the magnitudes of a
Lennard-Jones run (log q ~ -150 +- 5, -U/kT ~ -180 +- 5), ``nparticles`` and
``kT`` in ``meta``, and ``bar`` / ``md`` / ``nf``: the arithmetic of test.py:55-68
redone with NumPy on the reference's ``BAR`` (test.py itself needs private
packages and is not imported).  Q is shifted in fp32 as the reference shifts
it, the work values are formed in fp32, and everything from there on is fp64.
"""
from __future__ import annotations

import io
import json
import os
import sys
import zipfile

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
REF = "/root/reference"

sys.dont_write_bytecode = True
sys.path[:] = [p for p in sys.path if os.path.abspath(p or ".") not in (REPO, HERE)]
sys.path.insert(0, REF + "/applications")

import numpy as np  # noqa: E402

from src import bar as rbar  # noqa: E402

assert os.path.realpath(rbar.__file__).startswith(REF), rbar.__file__

RTOL = 1.0e-5


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


def _history(w_f, w_r, rtol, max_iter=1000):
    """The loop of the reference's BAR (bar.py:60-68) over its BARzero, keeping
    every iterate, every relative change and the largest exponent met."""
    M = np.log(float(w_f.size) / float(w_r.size))
    delta, hist, rcs, amax = 0.0, [], [], 0.0
    for it in range(max_iter):
        amax = max(amax, float(np.abs(M + w_f - delta).max()), float(np.abs(M - w_r - delta).max()))
        old = delta
        delta = -rbar.BARzero(w_f, w_r, delta) + delta
        hist.append(delta)
        rcs.append(abs((delta - old) / delta))
        if it > 0 and rcs[-1] < rtol:
            break
    return np.array(hist, dtype=np.float64), rcs, amax


def _lme(w):
    return float(np.log(np.mean(np.exp(w))))


def bar_arrays(w_f, w_r):
    """The recorded results of one pair of fp32 work vectors, with the
    generator's conditions asserted."""
    assert w_f.dtype == np.float32 and w_r.dtype == np.float32
    f64, r64 = w_f.astype(np.float64), w_r.astype(np.float64)
    hist, rcs, amax = _history(f64, r64, RTOL)
    bar_64 = float(rbar.BAR(f64, r64))
    assert bar_64 == hist[-1], "the recorded history is not the reference's own loop"
    assert rcs[-1] < RTOL / 2 and rcs[-2] > 2 * RTOL, "knife-edge stop: rc %r" % (rcs[-2:],)
    assert amax < 600.0, "exponent %g" % amax
    steps = np.abs(np.diff(np.concatenate(([0.0], hist))))
    assert all(b <= 0.5 * a for a, b in zip(steps[:-1], steps[1:])), "contraction above 0.5: %r" % (steps,)
    root = float(rbar.BAR(f64, r64, relative_tolerance=1.0e-13))
    return dict(w_f=w_f, w_r=w_r, bar_ref=np.float64(rbar.BAR(w_f, w_r)), bar_64=np.float64(bar_64),
                hist_64=hist, iters_64=np.int32(len(hist)), root_64=np.float64(root),
                lme_f_64=np.float64(_lme(f64)), lme_r_64=np.float64(_lme(r64)))


def crooks(n_f, n_r, dF, s, seed):
    rng = np.random.default_rng(seed)
    w_f = rng.normal(dF + 0.5 * s * s, s, n_f).astype(np.float32)
    w_r = rng.normal(-dF + 0.5 * s * s, s, n_r).astype(np.float32)
    return w_f, w_r


def case_bar(name, n_f, n_r, dF, s, seed):
    w_f, w_r = crooks(n_f, n_r, dF, s, seed)
    _save("fe_bar_" + name, dict(kind="bar", n_f=n_f, n_r=n_r, dF=dF, s=s, seed=seed, rtol=RTOL,
                                 numpy=np.__version__), bar_arrays(w_f, w_r))


def case_single(name, w_f, w_r):
    w_f, w_r = np.array([w_f], dtype=np.float32), np.array([w_r], dtype=np.float32)
    _save("fe_bar_" + name, dict(kind="bar", n_f=1, n_r=1, dF=None, s=None, seed=None, rtol=RTOL,
                                 numpy=np.__version__), bar_arrays(w_f, w_r))


def q_arrays(n, seed):
    rng = np.random.default_rng(seed)
    dF, s = 30.0, 2.0
    w_f, w_r = rng.normal(dF + 0.5 * s * s, s, n), rng.normal(-dF + 0.5 * s * s, s, n)
    Q = np.empty((2, n, 2))
    Q[0, :, 0] = rng.normal(-150.0, 5.0, n)  # log q of the flow's samples
    Q[0, :, 1] = Q[0, :, 0] - w_f            # their -U/kT
    Q[1, :, 1] = rng.normal(-180.0, 5.0, n)  # -U/kT of the target's samples
    Q[1, :, 0] = Q[1, :, 1] - w_r            # their log q
    return Q.astype(np.float32)


def case_q(name, n, nparticles, kT, seed):
    Q0 = q_arrays(n, seed)
    Q = Q0.copy()
    # test.py:55-60, in Q's dtype
    to_subtract_0, to_subtract_1 = Q[1][:, 0].min(), Q[1][:, 1].min()
    Q[0][:, 0] -= to_subtract_0
    Q[0][:, 1] -= to_subtract_1
    Q[1][:, 1] -= to_subtract_1
    Q[1][:, 0] -= to_subtract_0
    w_f, w_r = Q[0][:, 0] - Q[0][:, 1], -Q[1][:, 0] + Q[1][:, 1]
    res = bar_arrays(w_f, w_r)
    off = np.float64(to_subtract_0 - to_subtract_1)
    # test.py:66-68 in fp64
    bar = (off + res["bar_64"]) / nparticles * kT
    md = off / nparticles * kT - res["lme_r_64"] / nparticles * kT
    nf = -(-off / nparticles * kT - res["lme_f_64"] / nparticles * kT)
    _save(name, dict(kind="q", n=n, nparticles=nparticles, kT=kT, seed=seed, rtol=RTOL, numpy=np.__version__),
          dict(Q=Q0, bar=np.float64(bar), md=np.float64(md), nf=np.float64(nf), delta_64=res["bar_64"],
               w_f=w_f, w_r=w_r))


def main():
    case_bar("n500_d37", 500, 400, 37.5, 2.0, SEEDS["n500_d37"])
    case_bar("n500_dm3", 500, 400, -3.0, 1.0, SEEDS["n500_dm3"])
    case_bar("n37_d07", 37, 29, 0.7, 0.5, SEEDS["n37_d07"])
    case_bar("n4096_d120", 4096, 3277, 120.0, 4.0, SEEDS["n4096_d120"])
    case_bar("n500_d300", 500, 400, 300.0, 6.0, SEEDS["n500_d300"])
    case_single("n1", 3.0, -2.5)
    case_q("fe_q_lj", 64, 32, 2.0, SEEDS["q_lj"])


# the first seeds from 1 upwards at which a case meets the asserted conditions
SEEDS = {"n500_d37": 1, "n500_dm3": 1, "n37_d07": 1, "n4096_d120": 1, "n500_d300": 3, "q_lj": 1}

if __name__ == "__main__":
    main()
