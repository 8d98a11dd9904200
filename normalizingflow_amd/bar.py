"""The Bennett acceptance ratio of the applications layer
(applications/src/bar.py) and its bootstrap.

* ``logsum`` / ``BARzero`` / ``BAR`` -- the reference's names and signatures.
* ``bar_solve`` -- the batched form: P independent solves, problem p on the
  rows ``w_f[idx_f[p]]`` / ``w_r[idx_r[p]]``; returns ``out [P, 3]`` (DeltaF,
  log mean exp(w_f), log mean exp(w_r)) in fp64 and ``iters [P]`` in int32.
* ``bootstrap`` -- ``nboot`` solves over resampled work values.

One iteration maps D to
``D' = [LSE_i(g(M - wr_i - D) - wr_i) - log n_r] - [LSE_i g(M + wf_i - D) - log n_f]``
with ``M = log(n_f / n_r)``, ``g(a) = -log(1 + e^a)`` and a max-shifted
log-sum-exp, from ``DeltaF``; after iteration k (0-based) the loop stops when
``k > 0`` and ``|(D' - D) / D'| < relative_tolerance``, or at
``maximum_iterations``.

HIP fp32 tensors take the nfk_bar kernel: every problem of a call in one
launch, no host sync (``use_kernels = False`` forces the torch path).  NumPy
arrays, CPU tensors and other dtypes take an fp64 torch restatement of the same
iteration, which synchronises once per iteration on a device.

Both paths differ from the reference's text in two ways: ``g`` is evaluated as
``-(max(a, 0) + log1p(exp(-|a|)))``, finite for every finite a (the reference's
form shifts by min(a, 0) and overflows for |a| >~ 709), and a NaN iterate ends
the loop at once and is returned (the reference spins to maximum_iterations
and returns the same NaN).  ``bootstrap`` gives the errors of these estimates;
the multistate estimate of test.py:61-63 and its asymptotic error are mbar.py's.
"""
from __future__ import annotations

import math

import numpy as np
import torch

from . import kernels as K_

__all__ = ["logsum", "BARzero", "BAR", "bar_solve", "bootstrap"]

use_kernels = True


def _g(a):
    return -(a.clamp_min(0.0) + torch.log1p(torch.exp(-a.abs())))


def _lse(t):
    """Max-shifted log-sum-exp over the last dimension."""
    m = t.amax(dim=-1)
    return torch.log(torch.exp(t - m.unsqueeze(-1)).sum(dim=-1)) + m


def _tensor64(a):
    """A NumPy array or tensor as an fp64 tensor; (tensor, was it NumPy / CPU)."""
    if torch.is_tensor(a):
        return a.detach().double(), not a.is_cuda
    return torch.from_numpy(np.asarray(a, dtype=np.float64)), True


def _iterate(wf, wr, delta):
    """One BAR iteration of every row: wf [P, n_f], wr [P, n_r], delta [P] -> [P]."""
    n_f, n_r = wf.shape[-1], wr.shape[-1]
    M = math.log(n_f / n_r)
    d = delta.unsqueeze(-1)
    log_numer = _lse(_g((M + wf) - d)) - math.log(n_f)
    log_denom = _lse(_g((M - wr) - d) - wr) - math.log(n_r)
    return log_denom - log_numer


def logsum(a_n):
    """bar.py:3-14: log sum exp(a_n), shifted by the maximum."""
    t, host = _tensor64(a_n)
    out = _lse(t.reshape(-1))
    return float(out) if host else out


def BARzero(w_F, w_R, DeltaF):
    """bar.py:16-58: the function whose root is the BAR estimate,
    ``DeltaF - (log_denom - log_numer)``."""
    wf, host = _tensor64(w_F)
    wr, _ = _tensor64(w_R)
    d = torch.as_tensor(DeltaF, dtype=torch.float64, device=wf.device).reshape(1)
    out = (d - _iterate(wf.reshape(1, -1), wr.reshape(1, -1).to(wf.device), d))[0]
    return float(out) if host else out


def _solve_torch(wf, wr, delta0, maximum_iterations, relative_tolerance):
    P = wf.shape[0]
    dev = wf.device
    delta = torch.full((P,), float(delta0), dtype=torch.float64, device=dev)
    iters = torch.zeros(P, dtype=torch.int32, device=dev)
    done = torch.zeros(P, dtype=torch.bool, device=dev)
    for k in range(maximum_iterations):
        new = _iterate(wf, wr, delta)
        stop = torch.isnan(new)
        if k > 0:
            stop = stop | (((new - delta) / new).abs() < relative_tolerance)
        delta = torch.where(done, delta, new)
        iters = torch.where(done, iters, torch.full_like(iters, k + 1))
        done = done | stop
        if bool(done.all()):  # the one host sync of an iteration
            break
    out = torch.stack((delta, _lse(wf) - math.log(wf.shape[-1]), _lse(wr) - math.log(wr.shape[-1])), dim=1)
    return out, iters


def _rows(w64, idx, P):
    if idx is None:
        return w64.reshape(1, -1).expand(P, -1)
    return w64[idx.long()]


def bar_solve(w_f, w_r, *, idx_f=None, idx_r=None, delta0=0.0, maximum_iterations=1000,
              relative_tolerance=1.0e-5):
    """P independent BAR solves: problem p works on ``w_f[idx_f[p]]`` and
    ``w_r[idx_r[p]]`` (``idx_f`` [P, n_f] and ``idx_r`` [P, n_r] integer rows;
    both None: one problem on the vectors as they are).  Returns ``(out, iters)``:
    ``out`` [P, 3] fp64 holds DeltaF, log mean exp(w_f) and log mean exp(w_r) of
    every problem, ``iters`` [P] int32 the iterations done.  Index values must
    lie inside the vectors; on the device they are not checked."""
    if maximum_iterations < 1:
        raise ValueError("maximum_iterations must be at least 1")
    if not relative_tolerance >= 0:
        raise ValueError("relative_tolerance must be a number >= 0")
    P = 1
    for ix in (idx_f, idx_r):
        if ix is not None:
            if not torch.is_tensor(ix) or ix.dim() != 2 or ix.dtype.is_floating_point:
                raise ValueError("index rows must be a 2-D integer tensor")
            P = ix.shape[0]
    if idx_f is not None and idx_r is not None and idx_f.shape[0] != idx_r.shape[0]:
        raise ValueError("idx_f and idx_r hold different numbers of problems")
    on_kernel = (use_kernels and torch.is_tensor(w_f) and torch.is_tensor(w_r) and w_f.is_cuda and w_r.is_cuda
                 and w_f.dtype == torch.float32 and w_r.dtype == torch.float32)
    if on_kernel:
        wf, wr = w_f.detach().reshape(-1).contiguous(), w_r.detach().reshape(-1).contiguous()
        if (idx_f is None) != (idx_r is None):  # a single problem with one side plain
            if idx_f is None:
                idx_f = torch.arange(wf.numel(), dtype=torch.int32, device=wf.device).reshape(1, -1).expand(P, -1)
            else:
                idx_r = torch.arange(wr.numel(), dtype=torch.int32, device=wr.device).reshape(1, -1).expand(P, -1)
        if idx_f is not None:
            idx_f = idx_f.to(device=wf.device, dtype=torch.int32).contiguous()
            idx_r = idx_r.to(device=wf.device, dtype=torch.int32).contiguous()
        out = torch.empty(P, 3, dtype=torch.float64, device=wf.device)
        iters = torch.empty(P, dtype=torch.int32, device=wf.device)
        K_.bar(wf, wr, out, iters, idx_f=idx_f, idx_r=idx_r, delta0=delta0,
               max_iterations=maximum_iterations, rtol=relative_tolerance)
        return out, iters
    wf, _ = _tensor64(w_f)
    wr, _ = _tensor64(w_r)
    wf, wr = wf.reshape(-1), wr.reshape(-1).to(wf.device)
    if wf.numel() < 1 or wr.numel() < 1:
        raise ValueError("w_f and w_r must hold at least one work value each")
    rows_f = _rows(wf, None if idx_f is None else idx_f.to(wf.device), P)
    rows_r = _rows(wr, None if idx_r is None else idx_r.to(wf.device), P)
    return _solve_torch(rows_f, rows_r, delta0, maximum_iterations, relative_tolerance)


def BAR(w_F, w_R, DeltaF=0.0, maximum_iterations=1000, relative_tolerance=1.0e-5):
    """bar.py:60-68.  A Python float for NumPy arrays and CPU tensors, as the
    reference returns; a 0-d fp64 device tensor (no sync) for device tensors."""
    out, _ = bar_solve(w_F, w_R, delta0=DeltaF, maximum_iterations=maximum_iterations,
                       relative_tolerance=relative_tolerance)
    return out[0, 0] if out.is_cuda else float(out[0, 0])


def bootstrap(w_f, w_r, nboot, *, generator=None, chunk_bytes=1 << 28, **solver_kw):
    """``nboot`` BAR solves over work values resampled with replacement:
    ``out`` [nboot, 3] as ``bar_solve`` returns it.  The int32 index rows come
    from ``torch.randint`` on the work values' device through ``generator``;
    problems are solved in chunks whose two index matrices together stay within
    ``chunk_bytes``, and a chunk draws all of its ``idx_f`` first, then all of
    its ``idx_r``."""
    wf = w_f if torch.is_tensor(w_f) else torch.from_numpy(np.asarray(w_f))
    wr = w_r if torch.is_tensor(w_r) else torch.from_numpy(np.asarray(w_r))
    wf, wr = wf.detach().reshape(-1), wr.detach().reshape(-1)
    n_f, n_r = wf.numel(), wr.numel()
    per = max(1, int(chunk_bytes) // (4 * (n_f + n_r)))
    outs = []
    for p0 in range(0, nboot, per):
        c = min(per, nboot - p0)
        idx_f = torch.randint(n_f, (c, n_f), dtype=torch.int32, device=wf.device, generator=generator)
        idx_r = torch.randint(n_r, (c, n_r), dtype=torch.int32, device=wf.device, generator=generator)
        outs.append(bar_solve(wf, wr, idx_f=idx_f, idx_r=idx_r, **solver_kw)[0])
    return torch.cat(outs, dim=0)
