"""Multistate free energies: the MBAR self-consistent equations behind the
``emus`` estimate of test.py:61-63 and the FastMBAR driver of test.py:74-88.

The reference calls a private ``MBAR`` class and FastMBAR; neither is copied.
Both solve, for K states with N_k samples each (N samples in all, reduced
energies ``u[n, k]`` of every sample in every state),

    f_i = -log sum_n exp(-u_ni) / sum_k N_k exp(f_k - u_nk)        (gauge f_0 = 0)

whose solution is the minimum of a convex function with gradient ``g = S - N``
and Hessian ``H = diag(S) - G``, where ``W_nk = N_k exp(f_k - u_nk) / sum_j N_j
exp(f_j - u_nj)`` lies in [0, 1], ``S_k = sum_n W_nk`` and ``G = W^T W``.  For
two states the fixed point is exactly the BAR root.

* ``mbar_solve`` -- P independent solves, problem p on the rows ``u[idx[p]]``:
  ``(f [P, K] fp64, iters [P] int32, gram [P, K, K] fp64)``, gram = G at f.
* ``mbar_covariance`` / ``mbar_std`` -- the asymptotic covariance of f from
  ``gram`` and the standard deviation of a difference f_j - f_i.
* ``bootstrap`` -- ``nboot`` solves over samples resampled within each state.
* ``MBAR`` -- the call shape of test.py:61-62: ``MBAR(-Q).norm_const(niter)``.

One iteration at f forms two candidates from S and G: the self-consistent step
``f_sc = f - log(S / N)``, re-gauged, and the Newton step ``f_nr = f - H_r^{-1}
g_r`` on states 1..K-1 (Cholesky; a pivot that is not positive or a non-finite
entry makes it invalid).  It evaluates ``|S - N|^2`` at both and takes Newton
iff it is valid and its norm is strictly smaller, so a NaN falls to the
self-consistent step.  The loop stops when ``max_i |f'_i - f_i| <
relative_tolerance * max_i |f'_i|`` (from the first iteration on) or at
``maximum_iterations``; a NaN iterate ends it at once and is returned.  The
plain self-consistent iteration alone contracts at 0.93 to 0.996 on the
committed work-value sets and stops far from the root at any practical cap.

HIP fp32 ``u`` with ``kernels.mbar_supported(K)`` (2 <= K <= 8) takes the
nfk_mbar kernel: every problem of a call in one launch, no host sync
(``use_kernels = False`` forces the torch path).  NumPy arrays, CPU tensors,
other dtypes and other K take an fp64 torch restatement of the same algorithm,
which synchronises once per iteration on a device.

Every ``N_k`` must be at least 1: states without samples are not built, and
``ValueError`` is raised for them.
"""
from __future__ import annotations

import math

import numpy as np
import torch

from . import kernels as K_

__all__ = ["mbar_solve", "mbar_covariance", "mbar_std", "bootstrap", "MBAR"]

use_kernels = True


def _counts(n_k):
    try:
        counts = [int(n) for n in n_k]
    except TypeError:
        raise ValueError("n_k must be a sequence of ints") from None
    if any(c != n for c, n in zip(counts, n_k)):
        raise ValueError("n_k must hold whole numbers")
    if len(counts) < 2:
        raise ValueError("MBAR needs at least 2 states, got %d" % len(counts))
    if min(counts) < 1:
        raise ValueError("every N_k must be at least 1 (states without samples are not built), got %s" % (counts,))
    return counts


def _weights(u, c):
    """W [P, N, K] from u [P, N, K] and c = log N_k + f_k [P, K]."""
    a = c.unsqueeze(1) - u
    e = torch.exp(a - a.amax(dim=-1, keepdim=True))
    return e / e.sum(dim=-1, keepdim=True)


def _sums(u, c):
    W = _weights(u, c)
    G = torch.matmul(W.transpose(1, 2), W)  # a threaded GEMM need not give G_jk and G_kj the same bits
    return W.sum(dim=1), 0.5 * (G + G.transpose(1, 2))


def _host_vector(values, dev):
    """A short host list as an fp64 tensor on ``dev`` without a host sync."""
    return torch.tensor(values, dtype=torch.float64).to(dev, non_blocking=True)


def _solve_torch(u, counts, f0, maximum_iterations, relative_tolerance, trace=None):
    """u [P, N, K] fp64 -> (f [P, K], iters [P], gram [P, K, K]).  ``trace``, a
    list, receives per iteration (Newton taken [P] and still iterating, H_r
    [P, K-1, K-1]): what the tests derive their tolerance from."""
    P, _, K = u.shape
    dev = u.device
    n = _host_vector(counts, dev)
    logn = _host_vector([math.log(c) for c in counts], dev)
    f = (f0 - f0[0]).expand(P, K).clone()
    iters = torch.zeros(P, dtype=torch.int32, device=dev)
    done = torch.zeros(P, dtype=torch.bool, device=dev)
    for k in range(maximum_iterations):
        S, G = _sums(u, logn + f)
        f_sc = f - torch.log(S / n)
        f_sc = f_sc - f_sc[:, :1]
        H = torch.diag_embed(S[:, 1:]) - G[:, 1:, 1:]
        L, info = torch.linalg.cholesky_ex(torch.nan_to_num(H, nan=-1.0, posinf=-1.0, neginf=-1.0))
        step = torch.cholesky_solve((S - n)[:, 1:].unsqueeze(-1), L).squeeze(-1)
        f_nr = torch.cat((f[:, :1], f[:, 1:] - step), dim=1)
        valid = (info == 0) & torch.isfinite(H).all(dim=(1, 2)) & torch.isfinite(f_nr).all(dim=1)
        f_nr = torch.where(valid.unsqueeze(1), f_nr, f_sc)
        n_sc = (_weights(u, logn + f_sc).sum(dim=1) - n).square().sum(dim=1)
        n_nr = (_weights(u, logn + f_nr).sum(dim=1) - n).square().sum(dim=1)
        take = valid & (n_nr < n_sc)
        new = torch.where(take.unsqueeze(1), f_nr, f_sc)
        if trace is not None:
            trace.append((take & ~done, H))
        stop = torch.isnan(new).any(dim=1) | ((new - f).abs().amax(dim=1) < relative_tolerance * new.abs().amax(dim=1))
        f = torch.where(done.unsqueeze(1), f, new)
        iters = torch.where(done, iters, torch.full_like(iters, k + 1))
        done = done | stop
        if bool(done.all()):  # the one host sync of an iteration
            break
    return f, iters, _sums(u, logn + f)[1]


def mbar_solve(u, n_k, *, idx=None, f0=None, maximum_iterations=1000, relative_tolerance=1.0e-8):
    """P independent MBAR solves.  ``u`` [N, K] holds the reduced energy of
    every sample in every state (``(-Q).reshape(-1, K)`` as it is), ``n_k`` the
    K sample counts as host ints (each at least 1).  Problem p works on the rows
    ``u[idx[p]]`` (``idx`` [P, sum n_k] integer rows; None: one problem on u as
    it is, which then has sum n_k rows).  ``f0`` [K] is the start (default
    zeros).  Returns ``(f, iters, gram)``: ``f`` [P, K] fp64 with f[:, 0] = 0,
    ``iters`` [P] int32, ``gram`` [P, K, K] fp64, the Gram matrix W^T W of the
    weights at f.  Index values must lie inside u; on the device they are not
    checked."""
    counts = _counts(n_k)
    K, N = len(counts), sum(counts)
    if maximum_iterations < 1:
        raise ValueError("maximum_iterations must be at least 1")
    if not relative_tolerance >= 0:
        raise ValueError("relative_tolerance must be a number >= 0")
    ut = u if torch.is_tensor(u) else torch.from_numpy(np.asarray(u))
    ut = ut.detach()
    if ut.dim() != 2 or ut.shape[1] != K:
        raise ValueError("u must be [N, K] with K = len(n_k) = %d, got %s" % (K, tuple(ut.shape)))
    P = 1
    if idx is not None:
        if not torch.is_tensor(idx) or idx.dim() != 2 or idx.dtype.is_floating_point:
            raise ValueError("index rows must be a 2-D integer tensor")
        P = idx.shape[0]
        if idx.shape[1] != N or P < 1:
            raise ValueError("idx must be [P, sum n_k = %d], got %s" % (N, tuple(idx.shape)))
    elif ut.shape[0] != N:
        raise ValueError("the n_k sum to %d but u holds %d samples" % (N, ut.shape[0]))
    if f0 is not None:
        f0 = torch.as_tensor(f0, dtype=torch.float64).reshape(-1)
        if f0.numel() != K:
            raise ValueError("f0 must hold K = %d values" % K)
    if use_kernels and ut.is_cuda and ut.dtype == torch.float32 and K_.mbar_supported(K):
        if ut.stride(1) != 1:
            ut = ut.contiguous()
        if idx is not None:
            idx = idx.to(device=ut.device, dtype=torch.int32).contiguous()
        f = torch.empty(P, K, dtype=torch.float64, device=ut.device)
        iters = torch.empty(P, dtype=torch.int32, device=ut.device)
        gram = torch.empty(P, K, K, dtype=torch.float64, device=ut.device)
        K_.mbar(ut, counts, f, iters, gram, idx=idx, f0=None if f0 is None else f0.tolist(),
                max_iterations=maximum_iterations, rtol=relative_tolerance)
        return f, iters, gram
    u64 = ut.double()
    rows = u64.unsqueeze(0) if idx is None else u64[idx.to(u64.device).long()]
    start = torch.zeros(K, dtype=torch.float64) if f0 is None else f0
    return _solve_torch(rows, counts, start.to(u64.device), maximum_iterations, relative_tolerance)


def mbar_covariance(gram, n_k):
    """The asymptotic covariance of f, ``Theta = (G_w^{-1} - diag(N_k) +
    1 1^T / N)^{-1}`` with ``G_w = gram / (N_i N_j)``: the K x K form of
    ``W_w^T (I - W_w diag(N) W_w^T)^+ W_w`` for the normalised weights
    ``W_w = W / N_k``.  fp64 on gram's device, batched over leading dimensions,
    without a host sync."""
    counts = _counts(n_k)
    g = torch.as_tensor(gram).double()
    if g.shape[-1] != len(counts) or g.shape[-2] != len(counts):
        raise ValueError("gram must be [..., K, K] with K = len(n_k)")
    n = _host_vector(counts, g.device)
    gw = g / (n.unsqueeze(-1) * n.unsqueeze(-2))
    # inv_ex: no error check, so no host sync; a singular matrix gives inf / NaN entries
    inner = torch.linalg.inv_ex(gw).inverse - torch.diag(n) + 1.0 / float(sum(counts))
    return torch.linalg.inv_ex(inner).inverse


def mbar_std(gram, n_k, i, j):
    """The asymptotic standard deviation of f_j - f_i:
    ``sqrt(Theta_ii + Theta_jj - 2 Theta_ij)``."""
    t = mbar_covariance(gram, n_k)
    return torch.sqrt(t[..., i, i] + t[..., j, j] - 2.0 * t[..., i, j])


def bootstrap(u, n_k, nboot, *, generator=None, chunk_bytes=1 << 28, **solver_kw):
    """``nboot`` MBAR solves over samples resampled with replacement inside
    each state: the rows of u are the K states' blocks in order (n_k[0] rows of
    state 0's samples, then n_k[1] of state 1's, ...), and the positions of a
    block draw from that block.  Returns ``(f, iters, gram)`` as ``mbar_solve``
    does, with nboot problems.  The int32 index rows come from ``torch.randint``
    on u's device through ``generator``; problems are solved in chunks whose
    index matrix stays within ``chunk_bytes``, and a chunk draws its blocks in
    state order."""
    counts = _counts(n_k)
    ut = u if torch.is_tensor(u) else torch.from_numpy(np.asarray(u))
    N = sum(counts)
    if ut.dim() != 2 or ut.shape[0] != N:
        raise ValueError("the n_k sum to %d but u is %s" % (N, tuple(ut.shape)))
    per = max(1, int(chunk_bytes) // (4 * N))
    outs = []
    for p0 in range(0, nboot, per):
        c = min(per, nboot - p0)
        blocks, o = [], 0
        for n in counts:
            blocks.append(torch.randint(n, (c, n), dtype=torch.int32, device=ut.device, generator=generator) + o)
            o += n
        outs.append(mbar_solve(ut, counts, idx=torch.cat(blocks, dim=1), **solver_kw))
    return tuple(torch.cat(t, dim=0) for t in zip(*outs))


class MBAR:
    """The call shape of test.py:61-62.  ``neg_Q`` [K, N, K] holds, for the N
    samples drawn from each of K states, minus their log density in every
    state (``-Q``), so ``neg_Q.reshape(-1, K)`` is u and every N_k is N.
    ``norm_const(niter)`` returns the normalising constants ``c_i = exp(-f_i)``
    with c_0 = 1 as a [K] fp64 tensor on neg_Q's device; ``niter`` caps the
    iterations.  The private class's ``norm_const_err`` has no public
    definition and is not restated: ``mbar_covariance`` gives the asymptotic
    error of f."""

    def __init__(self, neg_Q):
        q = neg_Q if torch.is_tensor(neg_Q) else torch.from_numpy(np.asarray(neg_Q))
        if q.dim() != 3 or q.shape[0] != q.shape[2]:
            raise ValueError("neg_Q must be [K, N, K], got %s" % (tuple(q.shape),))
        self.u = q.detach().reshape(-1, q.shape[2])
        self.n_k = [q.shape[1]] * q.shape[0]
        self.f = self.iters = self.gram = None

    def norm_const(self, niter=40):
        f, self.iters, self.gram = mbar_solve(self.u, self.n_k, maximum_iterations=niter)
        self.f = f[0]
        return torch.exp(-self.f)
