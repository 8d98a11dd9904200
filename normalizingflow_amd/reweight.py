"""Importance weights of a Boltzmann-generator flow and the Metropolis chain
that turns its samples into samples of the target
(applications/src/utils.py:82-99).

* ``metropolis_chain`` -- C independent chains over N proposals each.  Step i
  proposes sample i; in the input's dtype and in this order

      d = e_cur - e[i];   with log_q: d = (d + lq_cur) - log_q[i]
      accept iff r[i] < exp(d)                    (a NaN rejects)

  and on acceptance ``(e_cur, lq_cur, idx_cur)`` become ``(e[i], log_q[i],
  base + i)``.  Without ``carry`` a chain starts at proposal 0, so step 0
  compares proposal 0 with itself, as the reference's loop does.  With
  ``log_q`` this is the independence sampler, whose stationary distribution is
  the target ``exp(-e)``; without it the test is the reference's, on the
  energy alone, which samples the target only if the proposals are uniform.
* ``log_weights`` -- ``log w = -e - log_q``; ``ess`` -- the Kish effective
  sample size of such weights; ``reweighted_mean`` -- the self-normalised
  importance average.  Plain torch, any device.

HIP fp32 tensors take the nfk_metropolize kernel: every chain of a call in one
launch, no host sync, capturable in a graph (``use_kernels = False`` forces the
torch path).  CPU tensors and other dtypes take a torch restatement of the same
arithmetic, vectorised over the chains and looping over the N steps.
"""
from __future__ import annotations

import torch

from . import kernels as K_

__all__ = ["metropolis_chain", "log_weights", "ess", "reweighted_mean"]

use_kernels = True


def _chain_torch(e, r, lq, start, base):
    """The chain in torch: e, r, lq [C, N]; start None or (e_cur, lq_cur, idx_cur)."""
    C, N = e.shape
    if start is None:
        ec = e[:, 0].clone()
        qc = None if lq is None else lq[:, 0].clone()
        ic = torch.full((C,), base, dtype=torch.int32, device=e.device)
    else:
        ec, qc, ic = start
    state = torch.empty(C, N, dtype=torch.int32, device=e.device)
    accepted = torch.empty(C, N, dtype=torch.bool, device=e.device)
    for i in range(N):
        d = ec - e[:, i]
        if lq is not None:
            d = (d + qc) - lq[:, i]
        a = r[:, i] < torch.exp(d)
        ec = torch.where(a, e[:, i], ec)
        if lq is not None:
            qc = torch.where(a, lq[:, i], qc)
        ic = torch.where(a, torch.full_like(ic, base + i), ic)
        state[:, i] = ic
        accepted[:, i] = a
    return state, accepted, accepted.sum(dim=1, dtype=torch.int32), (ec, qc, ic)


def _unit_rows(t):
    """t [C, N] as the kernel reads it: unit column stride, rows that do not overlap."""
    C, N = t.shape
    if (N > 1 and t.stride(1) != 1) or (C > 1 and t.stride(0) < N):
        return t.contiguous()
    return t


def metropolis_chain(e, r, log_q=None, *, carry=None, base=0):
    """C Metropolis chains over the N proposals of their rows: ``e`` (reduced
    energies U/kT), ``r`` (uniforms in [0, 1)) and ``log_q`` (log proposal
    densities, optional) are [C, N], or [N] for one chain.  Returns ``(state,
    accepted, naccept, carry)``: ``state`` int32, the index (``base`` + position
    in the row) of the chain's state after every step; ``accepted`` bool;
    ``naccept`` int32 per chain ([C], or 0-d for [N] input); ``carry`` the final
    ``(e_cur, lq_cur, idx_cur)`` (``lq_cur`` None without ``log_q``), which a
    later call takes as ``carry=`` to continue the chain on the next batch, with
    ``base`` the number of proposals seen so far.  ``base + N`` must fit int32."""
    one = e.dim() == 1
    if e.dim() not in (1, 2):
        raise ValueError("e must be [C, N] or [N], got %s" % (tuple(e.shape),))
    if r.shape != e.shape or (log_q is not None and log_q.shape != e.shape):
        raise ValueError("e, r and log_q must have one shape, got %s, %s%s" % (
            tuple(e.shape), tuple(r.shape), "" if log_q is None else ", %s" % (tuple(log_q.shape),)))
    base = int(base)
    e2, r2 = (t.detach().unsqueeze(0) if one else t.detach() for t in (e, r))
    q2 = None if log_q is None else (log_q.detach().unsqueeze(0) if one else log_q.detach())
    C, N = e2.shape
    if base < 0 or base + N > 2 ** 31 - 1:
        raise ValueError("base must be >= 0 and base + N fit int32 (base %d, N %d)" % (base, N))
    r2 = r2.to(device=e2.device, dtype=e2.dtype)
    if q2 is not None:
        q2 = q2.to(device=e2.device, dtype=e2.dtype)
    start = None
    if carry is not None:
        ec, qc, ic = carry
        if (qc is None) != (q2 is None):
            raise ValueError("the carry holds lq_cur exactly when log_q is given")
        # copies: the caller's carry is left as it is
        start = (ec.detach().reshape(-1).to(device=e2.device, dtype=e2.dtype, copy=True),
                 None if qc is None else qc.detach().reshape(-1).to(device=e2.device, dtype=e2.dtype, copy=True),
                 ic.detach().reshape(-1).to(device=e2.device, dtype=torch.int32, copy=True))
        if any(t is not None and t.numel() != C for t in start):
            raise ValueError("the carry must hold one state per chain (%d)" % C)
    if N == 0:
        if start is None:
            raise ValueError("a chain without carry needs at least one proposal")
        state = torch.empty(C, 0, dtype=torch.int32, device=e2.device)
        accepted = torch.empty(C, 0, dtype=torch.bool, device=e2.device)
        naccept, out = torch.zeros(C, dtype=torch.int32, device=e2.device), start
    elif use_kernels and e2.is_cuda and e2.dtype == torch.float32:
        dev = e2.device
        state = torch.empty(C, N, dtype=torch.int32, device=dev)
        acc8 = torch.empty(C, N, dtype=torch.uint8, device=dev)
        naccept = torch.zeros(C, dtype=torch.int32, device=dev)
        if start is None:
            out = (torch.empty(C, dtype=torch.float32, device=dev),
                   None if q2 is None else torch.empty(C, dtype=torch.float32, device=dev),
                   torch.empty(C, dtype=torch.int32, device=dev))
        else:
            out = start
        K_.metropolize(_unit_rows(e2), _unit_rows(r2), lq=None if q2 is None else _unit_rows(q2), state=state,
                       accepted=acc8, naccept=naccept, e_cur=out[0], lq_cur=out[1], idx_cur=out[2],
                       carry_in=start is not None, base=base)
        accepted = acc8.view(torch.bool)
    else:
        state, accepted, naccept, out = _chain_torch(e2, r2, q2, start, base)
    if one:
        return state[0], accepted[0], naccept[0], tuple(None if t is None else t[0] for t in out)
    return state, accepted, naccept, out


def log_weights(log_q, e):
    """``log w = -e - log_q``: the log importance weights of samples drawn with
    log density ``log_q`` for the target ``exp(-e)``, unnormalised."""
    return -e - log_q


def ess(logw):
    """The Kish effective sample size ``(sum w)^2 / sum w^2 = exp(2 LSE(logw) -
    LSE(2 logw))`` over the last dimension, in fp64: N for equal weights, 1 when
    one weight dominates."""
    lw = logw.detach().double()
    return torch.exp(2.0 * torch.logsumexp(lw, dim=-1) - torch.logsumexp(2.0 * lw, dim=-1))


def reweighted_mean(values, logw):
    """The self-normalised importance average ``sum_n w_n values_n / sum_n w_n``
    in fp64, ``w = exp(logw)`` over the last dimension of ``logw`` [..., N];
    ``values`` is [..., N] or [..., N, W] (a [..., W] average per row)."""
    w = torch.softmax(logw.detach().double(), dim=-1)
    v = values.detach().double()
    if v.dim() == w.dim():
        return (w * v).sum(dim=-1)
    if v.dim() == w.dim() + 1:
        return (w.unsqueeze(-1) * v).sum(dim=-2)
    raise ValueError("values must be [..., N] or [..., N, W] for logw [..., N], got %s and %s" % (
        tuple(values.shape), tuple(logw.shape)))
