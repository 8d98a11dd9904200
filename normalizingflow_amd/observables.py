"""Structure of a batch of configurations: the pair-distance histogram, the
radial distribution function g(r) and the running coordination number (the
reference has no counterpart; its drivers stop at ``plot_Q``).

* ``pair_histogram`` -- ``hist[k] = sum_b w_b * #{i < j : floor(r_ij * nbins /
  r_max) == k, r_ij < r_max}`` over a batch ``x`` [..., n, dim] with optional
  per-configuration ``weights``.  The pair vector is formed in x's dtype; with a
  box every component takes the minimum image ``d - L * rint(d * (1 / L))``, so
  positions need not lie in the box or within one box length of each other;
  ``r = sqrt(sum d^2)``.  Pairs at or beyond ``r_max`` land in no bin, and so do
  pairs whose r is NaN or infinite (the comparison is false; nothing is raised).
* ``rdf`` -- ``g[k] = hist[k] / (W * n (n - 1) / 2 * V_shell[k] / V)`` with
  ``W = sum w``: 1 for an ideal gas.  ``weights`` or ``log_weights`` (the log
  importance weights of ``reweight.log_weights``, self-normalised in fp64) give
  the reweighted g(r) of a flow's samples.
* ``coordination`` -- the mean number of neighbours within every bin edge.

HIP fp32 tensors of a supported shape (``kernels.pair_hist_supported``: n <=
256, dim 2 or 3, nbins <= 1024) take the nfk_pair_hist kernel: no [B, n, n]
temporary, integer counts per row, weights applied in fp64, fixed-order sums --
bitwise reproducible, exact integers for unit weights -- no host sync,
capturable on one stream.  Everything else (CPU, fp64, other shapes,
``use_kernels = False``) takes a torch restatement of the same definition in
the input's dtype, accumulated in fp64 and chunked over rows.
"""
from __future__ import annotations

import math

import torch

from . import kernels as K_

__all__ = ["pair_histogram", "rdf", "coordination"]

use_kernels = True
_CHUNK_ELEMS = 1 << 22  # pairs per chunk of the torch path


def _box_lengths(box, dim):
    """None, or the ``dim`` box lengths as floats."""
    if box is None:
        return None
    if torch.is_tensor(box):
        box = box.tolist()
    L = [float(box)] * dim if not isinstance(box, (tuple, list)) else [float(v) for v in box]
    if len(L) != dim:
        raise ValueError("box must be None, a scalar or %d lengths, got %r" % (dim, box))
    if not all(v > 0 and math.isfinite(v) for v in L):
        raise ValueError("box lengths must be positive, got %r" % (L,))
    return L


def _hist_torch(flat, L, r_max, nbins, w):
    """The restatement: flat [B, n, dim], w None or fp64 [B]; fp64 [nbins]."""
    B, n, dim = flat.shape
    dt, dev = flat.dtype, flat.device
    hist = torch.zeros(nbins, dtype=torch.float64, device=dev)
    if B == 0 or n < 2:
        return hist
    iu = torch.triu_indices(n, n, 1, device=dev)
    npair = iu.shape[1]
    rmax_t = torch.tensor(r_max, dtype=dt, device=dev)
    scale = torch.tensor(nbins / r_max, dtype=dt, device=dev)
    if L is not None:
        Lt = torch.tensor(L, dtype=dt, device=dev)
        iL = torch.tensor([1.0 / v for v in L], dtype=dt, device=dev)
    rows = max(1, _CHUNK_ELEMS // npair)  # row chunks: nothing grows with B * n * n
    for s in range(0, B, rows):
        pos = flat[s:s + rows]
        d = pos[:, iu[0]] - pos[:, iu[1]]
        if L is not None:
            d = d - Lt * torch.round(d * iL)
        r2 = d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]
        if dim == 3:
            r2 = r2 + d[..., 2] * d[..., 2]
        r = torch.sqrt(r2)
        inside = r < rmax_t  # false for a NaN
        bins = torch.where(inside, r * scale, torch.zeros_like(r)).long()
        inside = inside & (bins < nbins)
        if w is None:
            hist += torch.bincount(bins[inside], minlength=nbins).double()
        else:
            hist += torch.bincount(bins[inside], weights=w[s:s + rows, None].expand(-1, npair)[inside],
                                   minlength=nbins)
    return hist


def pair_histogram(x, box, r_max, nbins, weights=None):
    """The weighted pair-distance histogram of ``x`` [..., n, dim] (dim 2 or 3).
    ``box``: None (no wrap), a scalar (cubic) or ``dim`` lengths (orthorhombic);
    with a box ``r_max`` may not exceed half the shortest length.  ``weights``:
    None (1 for every configuration) or one weight per configuration, shape
    ``x.shape[:-2]``; they multiply a configuration's integer counts in fp64.
    Returns ``(hist, edges)``, fp64 [nbins] and [nbins + 1] on x's device."""
    if x.dim() < 2 or x.shape[-1] not in (2, 3):
        raise ValueError("x must be [..., n, dim] with dim 2 or 3, got %s" % (tuple(x.shape),))
    n, dim = x.shape[-2], x.shape[-1]
    nbins = int(nbins)
    r_max = float(r_max)
    if nbins < 1:
        raise ValueError("nbins must be at least 1, got %d" % nbins)
    if not (r_max > 0 and math.isfinite(r_max)):
        raise ValueError("r_max must be a number > 0, got %r" % r_max)
    L = _box_lengths(box, dim)
    if L is not None and r_max > 0.5 * min(L):
        raise ValueError("r_max %g exceeds half the shortest box length %g: beyond it one image per pair "
                         "is not enough" % (r_max, min(L)))
    flat = x.detach().reshape(-1, n, dim)
    B = flat.shape[0]
    w = None
    if weights is not None:
        w = weights.detach().reshape(-1).to(device=flat.device, dtype=torch.float64)
        if w.numel() != B:
            raise ValueError("weights must hold one value per configuration (%d), got shape %s"
                             % (B, tuple(weights.shape)))
    edges = torch.linspace(0.0, r_max, nbins + 1, dtype=torch.float64, device=flat.device)
    if use_kernels and flat.is_cuda and flat.dtype == torch.float32 and K_.pair_hist_supported(n, dim, nbins):
        rows = x.detach().reshape(B, n * dim)  # stays a view of a column slice of a wider tensor
        if (n * dim > 1 and rows.stride(1) != 1) or (B > 1 and rows.stride(0) < n * dim):
            rows = rows.contiguous()
        hist = torch.empty(nbins, dtype=torch.float64, device=flat.device)
        ws = torch.empty(K_.pair_hist_workspace_elems(B, nbins), dtype=torch.float64, device=flat.device)
        K_.pair_hist(rows, hist, ws if B > 0 else None, n=n, dim=dim,
                     box=(0.0, 0.0, 0.0) if L is None else (L + [L[0]])[:3], r_max=r_max,
                     weights=None if w is None else w.contiguous())
        return hist, edges
    return _hist_torch(flat, L, r_max, nbins, w), edges


def _shells(edges, dim):
    """The volume (area in 2-D) between consecutive edges."""
    if dim == 3:
        return 4.0 / 3.0 * math.pi * (edges[1:] ** 3 - edges[:-1] ** 3)
    return math.pi * (edges[1:] ** 2 - edges[:-1] ** 2)


def rdf(x, box, r_max=None, nbins=100, weights=None, log_weights=None):
    """The radial distribution function of ``x`` [..., n, dim] in a periodic box:
    ``(r, g)``, fp64 [nbins] each, r the bin centres and

        g[k] = hist[k] / (W * n (n - 1) / 2 * V_shell[k] / V),   W = sum w,

    with ``V_shell`` the volume of the shell between the bin's edges (the
    annulus area in 2-D) and ``V`` the box volume (area), so an ideal gas gives 1.
    ``r_max=None`` means half the shortest box length.  ``log_weights`` are
    self-normalised in fp64 (softmax over all configurations, as
    ``reweight.reweighted_mean`` does); ``weights`` are taken as they are; giving
    both is an error.  Without a box there is no ideal-gas normalisation:
    ``rdf`` raises, and ``pair_histogram`` is the call to make."""
    if weights is not None and log_weights is not None:
        raise ValueError("give weights or log_weights, not both")
    if box is None:
        raise ValueError("rdf needs a box for its ideal-gas normalisation; use pair_histogram without one")
    if x.dim() < 2 or x.shape[-1] not in (2, 3):
        raise ValueError("x must be [..., n, dim] with dim 2 or 3, got %s" % (tuple(x.shape),))
    n, dim = x.shape[-2], x.shape[-1]
    L = _box_lengths(box, dim)
    if r_max is None:
        r_max = 0.5 * min(L)
    B = x.numel() // max(n * dim, 1)
    if log_weights is not None:
        weights = torch.softmax(log_weights.detach().double().reshape(-1), dim=0)
    hist, edges = pair_histogram(x, L, r_max, nbins, weights=weights)
    W = float(B) if weights is None else weights.detach().double().sum().to(hist.device)
    V = math.prod(L)
    ideal = W * (n * (n - 1) / 2.0) * _shells(edges, dim) / V
    return 0.5 * (edges[1:] + edges[:-1]), hist / ideal


def coordination(r, g, n, box, dim=3):
    """The running coordination number at every bin edge, fp64 [nbins + 1]:
    ``N(r_k) = rho * sum_{m < k} g[m] V_shell[m]`` over the shells ``rdf`` divides
    by, with ``rho = (n - 1) / V`` the density of the other particles, which makes
    N exactly the mean number of neighbours within r (``(n - 1) V_sphere / V``
    for an ideal gas).  ``r`` are rdf's bin centres (uniform bins from 0), ``box``
    a scalar or ``dim`` lengths."""
    L = _box_lengths(box, len(box) if isinstance(box, (tuple, list)) else dim)
    if L is None:
        raise ValueError("coordination needs a box")
    r = r.detach().double()
    g = g.detach().double().to(r.device)
    edges = torch.cat((r - r[0], (r[-1] + r[0]).reshape(1)))
    rho = (n - 1) / math.prod(L)
    zero = torch.zeros(1, dtype=torch.float64, device=r.device)
    return torch.cat((zero, rho * torch.cumsum(g * _shells(edges, len(L)), dim=0)))
