"""Hand-written backward row kernels called directly through
normalizingflow_amd.kernels against fp64 autograd of the CPU reference
(rowkern.py): affine_coupling_bwd, planar_bwd, radial_bwd_scalars +
radial_bwd_apply, actnorm_bwd, maf_bwd and trig_features_bwd.

Shapes as in test_gpu_row_kernels.py (rowkern.SHAPES; the width -> W / column
block table is in rowkern.py).  For the backward they add what the layer tests
at dim 6 never ran: W = 1 (64 rows per wave), W = 64 with up to 256 trips,
the ragged last wave (batch 67), 1, 2, 5 and 256 column blocks of
k_colsum_part, two unequal chunks (batch 259 = 130 + 129 rows), the second
block of k_colsum_final and the second trip of the 256-thread loops (257 and
up), and batch 0.

Cotangents: both present over all shapes and in the strided layout (widths 5,
64, 100; every operand a view of its own NaN-filled buffer, g_in
accumulating); gz null and gld null at two shapes each, the reference
dropping the loss term.

Tolerances: row outputs (gx, g_s, g_t, gparams) element by element at
test_gpu_parity's Z_RTOL / Z_ATOL; batch-summed parameter gradients by
test_gpu_grad's rel_close at GRAD_TOL.  A case falls back to the on-par rule
only where the fp32 CPU reference itself misses (rowkern.check_rows /
check_sums print a FALLBACK line); on the MI355X run of this module no
backward case did.
"""
import pytest
import torch

import rowkern as rk
from normalizingflow_amd import kernels as K
from rowkern import GRID_STRIDE, NAN, NLS, NULLS, SHAPES, STRIDED, Layout, both_refs, check_rows, check_sums, ids, rnd
from test_gpu_parity import Z_ATOL, Z_RTOL
from test_gpu_row_kernels import maf_inputs, maf_range_params, maf_ranges, radial_params

pytestmark = pytest.mark.gpu

# (shape, strided layout, which cotangents are present)
CASES = ([pytest.param(s, False, "both", id=ids(s)) for s in SHAPES]
         + [pytest.param(s, True, "both", id=ids(s) + "-strided") for s in STRIDED]
         + [pytest.param(s, False, n, id=ids(s) + "-" + n) for s in NULLS for n in ("no_gz", "no_gld")])
EMPTY = (0, 5)


def cotangents(nulls, zshape, ldshape, seed=7):
    gz = None if nulls == "no_gz" else rnd(seed, *zshape)
    gld = None if nulls == "no_gld" else rnd(seed + 1, *ldshape)
    return gz, gld


def nanvec(n, dev):
    return torch.full((n,), NAN, device=dev)


def rows(what, ours, r64, r32):
    check_rows(what, ours, r64, r32, Z_RTOL, Z_ATOL)


# ---------------------------------------------------------------------------- affine coupling
def affine_bwd_case(shape, strided, nulls, inverse, dev, with_gt=True):
    B, n = shape
    x, s, t = rnd(1, B, n), rnd(2, B, n, scale=0.5), rnd(3, B, n)
    gz, gld = cotangents(nulls, (B, n), (B,))
    (_, _, g64), (_, _, g32) = both_refs(rk.ref_affine, dict(x=x, s=s, t=t), ("x", "s", "t"), gz, gld,
                                         inverse=inverse)
    accumulate = strided  # g_in accumulates in the strided layout, is written otherwise
    L = Layout(dev, strided)
    xd = L.inp(x)
    sd, td = L.pair(s, t)
    gzd = L.inp(gz) if gz is not None else None
    start = rnd(5, B, n)
    gin = L.inp(start) if accumulate else L.out(B, n)
    gsd, gtd = L.pair((B, n), (B, n)) if with_gt else (L.out(B, n), None)
    K.affine_coupling_bwd(xd, sd, td, gzd, None if gld is None else gld.to(dev), gin, gsd, gtd,
                          accumulate=accumulate, inverse=inverse)
    L.pads_intact()
    base = start if accumulate else torch.zeros(B, n)
    rows("g_in", gin, base.double() + g64["x"], base + g32["x"])
    rows("g_s", gsd, g64["s"], g32["s"])
    if with_gt:
        rows("g_t", gtd, g64["t"], g32["t"])


@pytest.mark.parametrize("inverse", [False, True], ids=["fwd", "inv"])
@pytest.mark.parametrize("shape,strided,nulls", CASES)
def test_affine_coupling_bwd(shape, strided, nulls, inverse, hip_device):
    affine_bwd_case(shape, strided, nulls, inverse, hip_device)


@pytest.mark.parametrize("strided", [False, True], ids=["write", "strided-acc"])
def test_affine_coupling_bwd_null_gt(strided, hip_device):
    """The forward direction allows g_t null (it is g_out itself)."""
    affine_bwd_case((67, 5), strided, "both", False, hip_device, with_gt=False)


# ---------------------------------------------------------------------------- planar
def planar_bwd_case(x, w, u, b, nl, strided, nulls, dev):
    B, D = x.shape
    gz, gld = cotangents(nulls, (B, D), (B,))
    (_, _, g64), (_, _, g32) = both_refs(rk.ref_planar, dict(x=x, w=w, u=u, b=b), ("x", "w", "u", "b"), gz, gld,
                                         nl=nl)
    L = Layout(dev, strided)
    xd = L.inp(x)
    gzd = L.inp(gz) if gz is not None else None
    gxd = L.out(B, D)
    gw, gu, gb = nanvec(D, dev), nanvec(D, dev), nanvec(1, dev)
    K.planar_bwd(xd, w.to(dev), u.to(dev), b.to(dev), gzd, None if gld is None else gld.to(dev), gxd, gw, gu, gb,
                 nonlinearity=K.PLANAR_NL[nl])
    L.pads_intact()
    rows("gx", gxd, g64["x"], g32["x"])
    check_sums("gw", gw, g64["w"], g32["w"])
    check_sums("gu", gu, g64["u"], g32["u"])
    check_sums("gb", gb, g64["b"], g32["b"])


@pytest.mark.parametrize("nl", NLS)
@pytest.mark.parametrize("shape,strided,nulls", CASES)
def test_planar_bwd(shape, strided, nulls, nl, hip_device):
    B, D = shape
    w, u, b = rk.planar_params(D, 11, nl)
    planar_bwd_case(rnd(14, B, D), w, u, b, nl, strided, nulls, hip_device)


@pytest.mark.parametrize("nl", ["leaky_relu", "elu"])
@pytest.mark.parametrize("dim", [5, 64, 257])
def test_planar_bwd_negative_s(dim, nl, hip_device):
    """w.u = -3: rows of both signs of s; the backward multiplies by sign(s).  No row is excluded."""
    x, w, u, b = rk.planar_negative_s_inputs(67, dim, nl, 21)
    planar_bwd_case(x, w, u, b, nl, False, "both", hip_device)
    planar_bwd_case(x, w, u, b, nl, False, "no_gz", hip_device)


@pytest.mark.parametrize("nl", ["leaky_relu", "elu"])
def test_planar_bwd_lin_zero_row(nl, hip_device):
    """A row of exact zeros with b = 0: lin == 0."""
    w, u, b = rk.planar_params(5, 31, nl, negative_s=True, bias=0.0)
    x = rnd(34, 67, 5)
    x[7] = 0.0
    planar_bwd_case(x, w, u, b, nl, False, "both", hip_device)


# ---------------------------------------------------------------------------- radial
def radial_bwd_case(shape, strided, nulls, dev):
    B, D = shape
    x = rnd(41, B, D)
    x0, la, be = radial_params(D, 42)
    gz, gld = cotangents(nulls, (B, D), (1,))
    (_, _, g64), (_, _, g32) = both_refs(rk.ref_radial, dict(x=x, x0=x0, la=la, be=be), ("x", "x0", "la", "be"),
                                         gz, gld)
    L = Layout(dev, strided)
    xd = L.inp(x)
    gzd = L.inp(gz) if gz is not None else None
    gxd = L.out(B, D)
    x0d, lad, bed = x0.to(dev), la.to(dev), be.to(dev)
    sumsq = torch.empty(1, dtype=torch.float64, device=dev)
    K.radial_sumsq(xd, x0d, torch.empty(K.radial_workspace_elems(), dtype=torch.float64, device=dev), sumsq)
    ws = K.flows_bwd_workspace(B, D, dev)
    scal, gx0 = nanvec(4, dev), nanvec(D, dev)
    K.radial_bwd_scalars(xd, x0d, lad, bed, sumsq, gzd, None if gld is None else gld.to(dev), scal, ws)
    K.radial_bwd_apply(xd, x0d, gzd, scal, gxd, gx0, ws)
    L.pads_intact()
    rows("gx", gxd, g64["x"], g32["x"])
    check_sums("gx0", gx0, g64["x0"], g32["x0"])
    check_sums("g_log_alpha", scal[1:2], g64["la"], g32["la"])
    check_sums("g_beta", scal[2:3], g64["be"], g32["be"])


@pytest.mark.parametrize("shape,strided,nulls", CASES)
def test_radial_bwd(shape, strided, nulls, hip_device):
    radial_bwd_case(shape, strided, nulls, hip_device)


# ---------------------------------------------------------------------------- actnorm
def actnorm_bwd_case(shape, strided, nulls, inverse, dev):
    B, D = shape
    x, mu, ls = rnd(51, B, D), rnd(52, D), rnd(53, D, scale=0.3)
    gz, gld = cotangents(nulls, (B, D), (1,))  # the log|det| is one scalar
    (_, _, g64), (_, _, g32) = both_refs(rk.ref_actnorm, dict(x=x, mu=mu, ls=ls), ("x", "mu", "ls"), gz, gld,
                                         inverse=inverse)
    L = Layout(dev, strided)
    xd, gzd, gxd = L.inp(x), L.inp(gz), L.out(B, D)
    gmu, gls = nanvec(D, dev), nanvec(D, dev)
    K.actnorm_bwd(xd, mu.to(dev), ls.to(dev), gzd, None if gld is None else gld.reshape(1).to(dev), gxd, gmu, gls,
                  inverse=inverse)
    L.pads_intact()
    rows("gx", gxd, g64["x"], g32["x"])
    check_sums("gmu", gmu, g64["mu"], g32["mu"])
    check_sums("gls", gls, g64["ls"], g32["ls"])


@pytest.mark.parametrize("inverse", [False, True], ids=["fwd", "inv"])
@pytest.mark.parametrize("shape,strided,nulls", [c for c in CASES if c.values[2] != "no_gz"])  # gz is not nullable
def test_actnorm_bwd(shape, strided, nulls, inverse, hip_device):
    actnorm_bwd_case(shape, strided, nulls, inverse, hip_device)


# ---------------------------------------------------------------------------- MAF
def maf_bwd_case(shape, c0, c1, inverse, strided, nulls, dev):
    B, dim = shape
    x, init, P = maf_inputs(B, dim)
    prm = maf_range_params(P, c0, c1)
    out_cols = rk.maf_out_cols(dim, c0, c1, inverse)
    in_cols = rk.maf_out_cols(dim, c0, c1, not inverse)  # forward reads x[:, i], the inverse x[:, dim-1-i]
    gout, gld = cotangents(nulls, (B, dim), (B,))
    inputs = dict(x=x, init=init, prm=prm if prm is not None else torch.zeros(B, 0))
    (_, _, g64), (_, _, g32) = both_refs(rk.ref_maf, inputs, ("x", "init", "prm"),
                                         None if gout is None else gout[:, out_cols], gld, c0=c0, c1=c1,
                                         inverse=inverse)
    L = Layout(dev, strided)
    xd = L.inp(x)
    pd = L.inp(prm) if prm is not None else None
    god = L.inp(gout) if gout is not None else None
    gxd = L.out(B, dim)
    gpd = L.out(B, prm.shape[1]) if prm is not None else None
    ginit = nanvec(2, dev)
    K.maf_bwd(xd, init.to(dev), pd, god, None if gld is None else gld.to(dev), c0, c1, gxd, gpd, ginit,
              inverse=inverse)
    L.pads_intact()
    rest = [c for c in range(dim) if c not in in_cols]
    rows("gx", gxd[:, in_cols], g64["x"][:, in_cols], g32["x"][:, in_cols])
    assert bool(torch.isnan(gxd[:, rest]).all()), "a gx column outside the range was written"
    if prm is not None:
        rows("gparams", gpd, g64["prm"], g32["prm"])
    if c0 == 0:
        check_sums("ginit", ginit, g64["init"], g32["init"])
    else:
        assert bool(torch.isnan(ginit).all()), "ginit is written only when c0 == 0"


@pytest.mark.parametrize("inverse", [False, True], ids=["fwd", "inv"])
@pytest.mark.parametrize("shape,strided,nulls", CASES)
def test_maf_bwd(shape, strided, nulls, inverse, hip_device):
    maf_bwd_case(shape, 0, shape[1], inverse, strided, nulls, hip_device)


@pytest.mark.parametrize("inverse", [False, True], ids=["fwd", "inv"])
@pytest.mark.parametrize("dim,cr", [pytest.param(d, r, id="d%d-%d:%d" % (d, r[0], r[1]))
                                    for d in (1, 2, 6, 65) for r in maf_ranges(d)])
def test_maf_bwd_column_ranges(dim, cr, inverse, hip_device):
    maf_bwd_case((67, dim), cr[0], cr[1], inverse, False, "both", hip_device)
    maf_bwd_case((67, dim), cr[0], cr[1], inverse, True, "no_gld", hip_device)


# ---------------------------------------------------------------------------- trig features
def trig_bwd_case(shape, strided, dev):
    B, n = shape
    x, gf, start = rnd(71, B, n, scale=2.0), rnd(72, B, 2 * n), rnd(73, B, n)
    (_, _, g64), (_, _, g32) = both_refs(rk.ref_trig, dict(x=x), ("x",), gf, None, bnd=3.0)
    L = Layout(dev, strided)
    xd, gfd, gxd = L.inp(x), L.inp(gf), L.inp(start)  # the kernel accumulates into gx
    K.trig_features_bwd(xd, gfd, gxd, 3.0)
    L.pads_intact()
    rows("gx", gxd, start.double() + g64["x"], start + g32["x"])


@pytest.mark.parametrize("shape,strided", [pytest.param(s, False, id=ids(s)) for s in SHAPES]
                         + [pytest.param(s, True, id=ids(s) + "-strided") for s in STRIDED])
def test_trig_features_bwd(shape, strided, hip_device):
    trig_bwd_case(shape, strided, hip_device)


def test_trig_features_bwd_grid_stride(hip_device):
    """batch * n above the 16,384-block cap of k_trig_bwd."""
    trig_bwd_case(GRID_STRIDE, False, hip_device)


# ---------------------------------------------------------------------------- empty batch
def test_empty_batch_backward(hip_device):
    """Batch 0 (null row pointers) succeeds; the parameter gradients are what
    autograd gives for an empty sum: zero, but for ActNorm's batch-independent log|det| term."""
    for nl in NLS:
        w, u, b = rk.planar_params(EMPTY[1], 11, nl)
        planar_bwd_case(rnd(14, *EMPTY), w, u, b, nl, False, "both", hip_device)
    for inverse in (False, True):
        actnorm_bwd_case(EMPTY, False, "both", inverse, hip_device)
        maf_bwd_case(EMPTY, 0, EMPTY[1], inverse, False, "both", hip_device)
        affine_bwd_case(EMPTY, False, "both", inverse, hip_device)
    torch.cuda.synchronize(hip_device)
