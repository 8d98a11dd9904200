"""Forward row kernels called directly through normalizingflow_amd.kernels
(not through the layer classes) against the fp64 CPU reference of rowkern.py:
affine_coupling, planar, radial_sumsq + radial_apply, actnorm, maf,
trig_features and normal_logprob, both directions where there is an inverse.

Shapes (rowkern.SHAPES): every width of WIDTHS at batch 67 (3 at the two
widest), every batch of BATCHES at widths 1, 5, 64, 65 and 257.  The widths
put every lane-group instance W of k_affine / k_planar / k_normal_lp to work
once exactly full and once ragged, with one and with several trips of the
``c += W`` loop (table in rowkern.py); batch 67 leaves the last wave ragged
for every W.  normal_logprob also runs every multiple of 4 up to 256, which
puts dim / 4 on each W of the float4 kernel (4 -> 1, 8 -> 2, 12-16 -> 4,
20-32 -> 8, 36-64 -> 16, 68-128 -> 32, 132-256 -> 64), and each of those
widths again as an unaligned view, which takes the scalar kernel at a
multiple-of-4 width.

Layouts: contiguous with logdet_mode WRITE; at widths 5, 64, 100 each matrix
operand a view of its own NaN-filled buffer with its own row stride
(rowkern.Layout) with logdet_mode ACC; logdet_mode NONE at two more shapes.

Tolerances: test_gpu_parity's Z_*, LD_*, LP_* against fp64, every element.
Cases where the fp32 CPU reference itself misses them fall back to the on-par
rule (rowkern.check_rows) and print a FALLBACK line with both errors.  On an
MI355X one case needs it: Radial's log|det| at 16,384 columns
(test_radial[b3-d16384], ld_scalar and logdet), where (dim - 1) log(1 + bh h)
multiplies one fp32 rounding by 16,383: the fp32 reference is 7.63e-4 off
fp64 and the kernel's value is the same 7.63e-4 off.  Planar at its cap of
16,384 columns (64 KiB of dynamic LDS next to the static reduction scratch)
launches and passes directly.
"""
import math

import pytest
import torch

import rowkern as rk
from normalizingflow_amd import _lib, kernels as K
from normalizingflow_amd.kernels import MODE_ACC, MODE_NONE, MODE_WRITE
from rowkern import (GRID_STRIDE, NAN, NLS, NULLS, SHAPES, STRIDED, WIDTHS, Layout, both_refs, check_rows, ids,
                     ld_operand, rnd, uni)
from test_gpu_parity import LD_ATOL, LD_RTOL, LP_ATOL, LP_RTOL, Z_ATOL, Z_RTOL

pytestmark = pytest.mark.gpu

CASES = ([pytest.param(s, False, MODE_WRITE, id=ids(s)) for s in SHAPES]
         + [pytest.param(s, True, MODE_ACC, id=ids(s) + "-strided-acc") for s in STRIDED]
         + [pytest.param(s, False, MODE_NONE, id=ids(s) + "-none") for s in NULLS])
LAYOUT_CASES = ([pytest.param(s, False, id=ids(s)) for s in SHAPES]
                + [pytest.param(s, True, id=ids(s) + "-strided") for s in STRIDED])


def check_ld(ldd, start, ld64, ld32):
    if ldd is not None:
        check_rows("logdet", ldd, start.double() + ld64, start + ld32, LD_RTOL, LD_ATOL)


def test_widths_cover_every_lane_group():
    """Every W instance runs once exactly full (dim == W) and once ragged."""
    for w in (1, 2, 4, 8, 16, 32, 64):
        assert w in WIDTHS
        assert w <= 2 or any(rk.lanes_for(d) == w and d < w for d in WIDTHS)  # W = 1, 2 have one width each
    assert {rk.lanes_for(d // 4) for d in range(4, 257, 4)} == {1, 2, 4, 8, 16, 32, 64}


# ---------------------------------------------------------------------------- affine coupling
@pytest.mark.parametrize("inverse", [False, True], ids=["fwd", "inv"])
@pytest.mark.parametrize("shape,strided,mode", CASES)
def test_affine_coupling(shape, strided, mode, inverse, hip_device):
    B, n = shape
    x, s, t = rnd(1, B, n), rnd(2, B, n, scale=0.5), rnd(3, B, n)
    (z64, ld64, _), (z32, ld32, _) = both_refs(rk.ref_affine, dict(x=x, s=s, t=t), inverse=inverse)
    L = Layout(hip_device, strided)
    xd = L.inp(x)
    sd, td = L.pair(s, t)
    zd = L.out(B, n)
    ldd, start = ld_operand(mode, B, hip_device)
    K.affine_coupling(xd, sd, td, zd, logdet=ldd, logdet_mode=mode, inverse=inverse)
    L.pads_intact()
    check_rows("z", zd, z64, z32, Z_RTOL, Z_ATOL)
    check_ld(ldd, start, ld64, ld32)


@pytest.mark.parametrize("inverse", [False, True], ids=["fwd", "inv"])
def test_affine_coupling_unequal_st_strides(inverse, hip_device):
    """s and t with unequal row strides: the wrapper copies them."""
    B, n = 67, 5
    x, s, t = rnd(1, B, n), rnd(2, B, n, scale=0.5), rnd(3, B, n)
    (z64, ld64, _), (z32, ld32, _) = both_refs(rk.ref_affine, dict(x=x, s=s, t=t), inverse=inverse)
    L = Layout(hip_device, True)
    xd, sd, td, zd = L.inp(x), L.inp(s), L.inp(t), L.out(B, n)
    assert sd.stride(0) != td.stride(0)
    ldd, start = ld_operand(MODE_WRITE, B, hip_device)
    K.affine_coupling(xd, sd, td, zd, logdet=ldd, logdet_mode=MODE_WRITE, inverse=inverse)
    L.pads_intact()
    check_rows("z", zd, z64, z32, Z_RTOL, Z_ATOL)
    check_ld(ldd, start, ld64, ld32)


# ---------------------------------------------------------------------------- planar
def run_planar(x, w, u, b, nl, strided, mode, dev):
    B, D = x.shape
    (z64, ld64, _), (z32, ld32, _) = both_refs(rk.ref_planar, dict(x=x, w=w, u=u, b=b), nl=nl)
    L = Layout(dev, strided)
    xd, zd = L.inp(x), L.out(B, D)
    ldd, start = ld_operand(mode, B, dev)
    ld_out = torch.full((B,), NAN, device=dev)
    K.planar(xd, w.to(dev), u.to(dev), b.to(dev), zd, logdet=ldd, logdet_mode=mode, ld_out=ld_out,
             nonlinearity=K.PLANAR_NL[nl])
    L.pads_intact()
    check_rows("z", zd, z64, z32, Z_RTOL, Z_ATOL)
    check_rows("ld_out", ld_out, ld64, ld32, LD_RTOL, LD_ATOL)  # written under every mode
    check_ld(ldd, start, ld64, ld32)


@pytest.mark.parametrize("nl", NLS)
@pytest.mark.parametrize("shape,strided,mode", CASES)
def test_planar(shape, strided, mode, nl, hip_device):
    B, D = shape
    w, u, b = rk.planar_params(D, 11, nl)
    run_planar(rnd(14, B, D), w, u, b, nl, strided, mode, hip_device)


@pytest.mark.parametrize("nl", ["leaky_relu", "elu"])
@pytest.mark.parametrize("dim", [5, 64, 257])
def test_planar_negative_s(dim, nl, hip_device):
    """w.u = -3: rows of both signs of s = 1 + h'(lin) w.u, none excluded."""
    x, w, u, b = rk.planar_negative_s_inputs(67, dim, nl, 21)
    run_planar(x, w, u, b, nl, False, MODE_WRITE, hip_device)


@pytest.mark.parametrize("nl", ["leaky_relu", "elu"])
def test_planar_lin_zero_row(nl, hip_device):
    """A row of exact zeros with b = 0: lin == 0, where h' takes neither mask."""
    w, u, b = rk.planar_params(5, 31, nl, negative_s=True, bias=0.0)
    x = rnd(34, 67, 5)
    x[7] = 0.0
    run_planar(x, w, u, b, nl, False, MODE_WRITE, hip_device)


def test_planar_dim_cap(hip_device):
    """The entry point refuses widths above its cap of 16,384 (SHAPES runs the cap itself)."""
    x = torch.zeros(3, 16385, device=hip_device)
    v = torch.zeros(16385, device=hip_device)
    with pytest.raises(ValueError, match="bad sizes"):
        K.planar(x, v, v, torch.zeros(1, device=hip_device), torch.empty_like(x))


# ---------------------------------------------------------------------------- radial
def radial_params(dim, seed):
    return uni(seed, dim, 1.0 / math.sqrt(dim)), uni(seed + 1, 1, 1.0), uni(seed + 2, 1, 1.0)


def radial_case(shape, strided, mode, dev):
    B, D = shape
    x = rnd(41, B, D)
    x0, la, be = radial_params(D, 42)
    (z64, ld64, _), (z32, ld32, _) = both_refs(rk.ref_radial, dict(x=x, x0=x0, la=la, be=be))
    L = Layout(dev, strided)
    xd, zd = L.inp(x), L.out(B, D)
    ws = torch.empty(K.radial_workspace_elems(), dtype=torch.float64, device=dev)
    sumsq = torch.full((1,), NAN, dtype=torch.float64, device=dev)
    K.radial_sumsq(xd, x0.to(dev), ws, sumsq)
    want = ((x.double() - x0.double()) ** 2).sum()
    assert abs(float(sumsq) - float(want)) <= Z_RTOL * float(want)
    ldd, start = ld_operand(mode, B, dev)
    ld_scalar = torch.full((1,), NAN, device=dev)
    K.radial_apply(xd, x0.to(dev), la.to(dev), be.to(dev), sumsq, zd, ld_scalar, logdet=ldd, logdet_mode=mode)
    L.pads_intact()
    check_rows("z", zd, z64, z32, Z_RTOL, Z_ATOL)
    check_rows("ld_scalar", ld_scalar, ld64, ld32, LD_RTOL, LD_ATOL)  # written under every mode
    if ldd is not None:
        check_ld(ldd, start, ld64.expand(B), ld32.expand(B))


@pytest.mark.parametrize("shape,strided,mode", CASES)
def test_radial(shape, strided, mode, hip_device):
    radial_case(shape, strided, mode, hip_device)


def test_radial_apply_grid_stride(hip_device):
    """batch * dim above the 16,384-block cap of k_radial_apply: second trip of its loop."""
    radial_case(GRID_STRIDE, False, MODE_WRITE, hip_device)


# ---------------------------------------------------------------------------- actnorm
@pytest.mark.parametrize("inverse", [False, True], ids=["fwd", "inv"])
@pytest.mark.parametrize("shape,strided,mode", CASES)
def test_actnorm(shape, strided, mode, inverse, hip_device):
    B, D = shape
    dev = hip_device
    x, mu, ls = rnd(51, B, D), rnd(52, D), rnd(53, D, scale=0.3)
    (z64, ld64, _), (z32, ld32, _) = both_refs(rk.ref_actnorm, dict(x=x, mu=mu, ls=ls), inverse=inverse)
    L = Layout(dev, strided)
    xd, zd = L.inp(x), L.out(B, D)
    ldd, start = ld_operand(mode, B, dev)
    ld_scalar = torch.full((1,), NAN, device=dev)
    K.actnorm(xd, mu.to(dev), ls.to(dev), zd, logdet=ldd, logdet_mode=mode, ld_scalar=ld_scalar, inverse=inverse)
    L.pads_intact()
    check_rows("z", zd, z64, z32, Z_RTOL, Z_ATOL)
    check_rows("ld_scalar", ld_scalar, ld64.reshape(1), ld32.reshape(1), LD_RTOL, LD_ATOL)
    if ldd is not None:
        check_ld(ldd, start, ld64.expand(B), ld32.expand(B))


# ---------------------------------------------------------------------------- MAF
def maf_inputs(B, dim, seed=61):
    init = uni(seed, 2, math.sqrt(0.5))
    P = rnd(seed + 1, B, 2 * max(dim - 1, 1))  # (mu, alpha) of the columns 1 .. dim-1
    P[:, 1::2] *= 0.3
    return rnd(seed + 2, B, dim), init, P


def maf_range_params(P, c0, c1):
    """The columns of [max(c0, 1), c1), as the wrapper takes them (None when there are none)."""
    p0 = max(c0, 1)
    return P[:, 2 * (p0 - 1):2 * (c1 - 1)] if c1 > p0 else None


def maf_case(shape, c0, c1, inverse, strided, mode, dev):
    B, dim = shape
    x, init, P = maf_inputs(B, dim)
    prm = maf_range_params(P, c0, c1)
    inputs = dict(x=x, init=init, prm=prm if prm is not None else torch.zeros(B, 0))
    (z64, ld64, _), (z32, ld32, _) = both_refs(rk.ref_maf, inputs, c0=c0, c1=c1, inverse=inverse)
    L = Layout(dev, strided)
    xd, zd = L.inp(x), L.out(B, dim)
    pd = L.inp(prm) if prm is not None else None
    ldd, start = ld_operand(mode, B, dev)
    K.maf(xd, init.to(dev), pd, zd, c0, c1, logdet=ldd, logdet_mode=mode, inverse=inverse)
    L.pads_intact()
    cols = rk.maf_out_cols(dim, c0, c1, inverse)
    rest = [c for c in range(dim) if c not in cols]
    check_rows("z", zd[:, cols], z64, z32, Z_RTOL, Z_ATOL)
    assert bool(torch.isnan(zd[:, rest]).all()), "a column outside the range was written"
    if c0 == c1 and ldd is not None:  # an empty range launches nothing
        assert bool(torch.isnan(ldd).all()) if mode == MODE_WRITE else torch.equal(ldd.cpu(), start)
    else:
        check_ld(ldd, start, ld64, ld32)


@pytest.mark.parametrize("inverse", [False, True], ids=["fwd", "inv"])
@pytest.mark.parametrize("shape,strided,mode", CASES)
def test_maf(shape, strided, mode, inverse, hip_device):
    maf_case(shape, 0, shape[1], inverse, strided, mode, hip_device)


def maf_ranges(dim):
    rs = [(0, dim), (0, 1), (1, dim), (2, 5), (dim - 1, dim)]
    return sorted({(a, b) for a, b in rs if 0 <= a <= b <= dim})


MAF_RANGES = [pytest.param(d, r, id="d%d-%d:%d" % (d, r[0], r[1])) for d in (1, 2, 6, 65) for r in maf_ranges(d)]


@pytest.mark.parametrize("inverse", [False, True], ids=["fwd", "inv"])
@pytest.mark.parametrize("dim,cr", MAF_RANGES)
def test_maf_column_ranges(dim, cr, inverse, hip_device):
    maf_case((67, dim), cr[0], cr[1], inverse, False, MODE_WRITE, hip_device)
    maf_case((67, dim), cr[0], cr[1], inverse, True, MODE_ACC, hip_device)


@pytest.mark.parametrize("dim", [6, 65])
def test_maf_inverse_assembled_from_ranges(dim, hip_device):
    """Consecutive ranges with MODE_ACC equal the one-shot reference."""
    B, dev = 67, hip_device
    x, init, P = maf_inputs(B, dim)
    (z64, ld64, _), (z32, ld32, _) = both_refs(rk.ref_maf, dict(x=x, init=init, prm=P), c0=0, c1=dim, inverse=True)
    xd, Pd = x.to(dev), P.to(dev)
    zd = torch.full((B, dim), NAN, device=dev)
    ldd = torch.zeros(B, device=dev)
    for c0, c1 in ((0, 1), (1, 2), (2, 5), (5, dim)):
        K.maf(xd, init.to(dev), maf_range_params(Pd, c0, c1), zd, c0, c1, logdet=ldd, logdet_mode=MODE_ACC,
              inverse=True)
    check_rows("z", zd, z64, z32, Z_RTOL, Z_ATOL)
    check_rows("logdet", ldd, ld64, ld32, LD_RTOL, LD_ATOL)


# ---------------------------------------------------------------------------- trig features
def trig_case(shape, strided, dev):
    B, n = shape
    x = rnd(71, B, n, scale=2.0)
    (f64, _, _), (f32, _, _) = both_refs(rk.ref_trig, dict(x=x), bnd=3.0)
    L = Layout(dev, strided)
    xd, fd = L.inp(x), L.out(B, 2 * n)
    K.trig_features(xd, fd, 3.0)
    L.pads_intact()
    check_rows("feat", fd, f64, f32, Z_RTOL, Z_ATOL)


@pytest.mark.parametrize("shape,strided", LAYOUT_CASES)
def test_trig_features(shape, strided, hip_device):
    trig_case(shape, strided, hip_device)


def test_trig_features_grid_stride(hip_device):
    trig_case(GRID_STRIDE, False, hip_device)


# ---------------------------------------------------------------------------- normal_logprob
VAR = 1.7


def normal_consts(dim):
    if dim <= 1000:
        return K.iso_normal_consts(VAR, dim)
    scale = torch.tensor(VAR, dtype=torch.float32).sqrt()  # the Cholesky diagonal of var * I
    return float(scale), float(scale.expand(dim).log().sum())


def unaligned(z, dev, odd_stride=False):
    """z as a view that the float4 kernel cannot take: pointer 4 bytes past a
    16-byte boundary (stride a multiple of 4), or an odd row stride."""
    B, D = z.shape
    if odd_stride:
        buf = torch.full((B, D + 1 + (D % 2)), NAN, device=dev)
        assert buf.stride(0) % 2 == 1
        v = buf[:, :D]
    else:
        buf = torch.full((B, D + 4 + (-D) % 4), NAN, device=dev)
        assert buf.stride(0) % 4 == 0
        v = buf[:, 1:1 + D]
    v.copy_(z)
    return v


NORMAL_SHAPES = SHAPES + [(67, d) for d in range(4, 257, 4) if (67, d) not in SHAPES]


@pytest.mark.parametrize("shape", NORMAL_SHAPES, ids=ids)
def test_normal_logprob(shape, hip_device):
    B, D = shape
    dev = hip_device
    z, ld = rnd(81, B, D), rnd(82, B)
    scale, hld = normal_consts(D)
    zc = z.to(dev)
    views = [("contiguous", zc), ("unaligned", unaligned(z, dev)), ("odd stride", unaligned(z, dev, True))]
    assert zc.data_ptr() % 16 == 0 and views[1][1].data_ptr() % 16 == 4
    for sign, logdet in ((1, None), (1, ld), (-1, ld)):
        r64 = rk.ref_normal(z.double(), VAR, logdet, sign)
        r32 = rk.ref_normal(z, VAR, logdet, sign)
        got = {}
        for name, zv in views:
            out = torch.full((B,), NAN, device=dev)
            status = torch.zeros(1, dtype=torch.int32, device=dev)
            K.normal_logprob(zv, out, scale=scale, hld=hld, logdet=None if logdet is None else logdet.to(dev),
                             sign=sign, status=status)
            check_rows("log_prob (%s, sign %d)" % (name, sign), out, r64, r32, LP_RTOL, LP_ATOL)
            assert int(status) == 0, "status touched without a NaN"
            got[name] = out.cpu()
        # scalar kernel against float4 kernel (where dim % 4 == 0) on the same numbers
        for name in ("unaligned", "odd stride"):
            torch.testing.assert_close(got[name], got["contiguous"], rtol=LP_RTOL, atol=LP_ATOL)


@pytest.mark.parametrize("dim", [5, 8, 64, 100, 256])
def test_normal_logprob_nan_row(dim, hip_device):
    """A NaN in one row: that row's output is NaN, NFK_ST_NAN_Z is set, and the
    other rows are bitwise what they are without it -- on both kernels."""
    B, dev = 67, hip_device
    z = rnd(83, B, dim)
    bad = z.clone()
    bad[40, dim // 2] = NAN
    scale, hld = normal_consts(dim)
    keep = torch.arange(B) != 40
    for make in (lambda t: t.to(dev), lambda t: unaligned(t, dev)):
        outs = []
        for src in (z, bad):
            out = torch.full((B,), NAN, device=dev)
            status = torch.zeros(1, dtype=torch.int32, device=dev)
            K.normal_logprob(make(src), out, scale=scale, hld=hld, status=status)
            outs.append((out.cpu(), int(status)))
        (clean, st0), (dirty, st1) = outs
        assert st0 == 0 and st1 == _lib.ST_NAN_Z
        assert bool(torch.isnan(dirty[40])) and bool(torch.isfinite(clean).all())
        assert torch.equal(dirty[keep], clean[keep])


# ---------------------------------------------------------------------------- empty batch
def test_empty_batch_forward(hip_device):
    """Batch 0 succeeds and returns empty outputs (tensors of no rows have a null pointer)."""
    dev, D = hip_device, 5
    x = torch.empty(0, D, device=dev)
    z = torch.empty(0, D, device=dev)
    ld = torch.empty(0, device=dev)
    assert x.data_ptr() == 0
    w, u, b = (t.to(dev) for t in rk.planar_params(D, 11, "tanh"))
    K.planar(x, w, u, b, z, logdet=ld, logdet_mode=MODE_WRITE, ld_out=torch.empty(0, device=dev))
    K.affine_coupling(x, x, x, z, logdet=ld, logdet_mode=MODE_ACC)
    K.affine_coupling(x, x, x, z, logdet=ld, logdet_mode=MODE_ACC, inverse=True)
    K.maf(x, torch.zeros(2, device=dev), torch.empty(0, 2 * (D - 1), device=dev), z, 0, D, logdet=ld,
          logdet_mode=MODE_WRITE)
    ls = rnd(53, D, scale=0.3)
    ld_scalar = torch.full((1,), NAN, device=dev)
    K.actnorm(x, torch.zeros(D, device=dev), ls.to(dev), z, logdet=ld, logdet_mode=MODE_WRITE, ld_scalar=ld_scalar)
    check_rows("ld_scalar", ld_scalar, ls.double().sum().reshape(1), ls.sum().reshape(1), LD_RTOL, LD_ATOL)
    torch.cuda.synchronize(dev)
    assert z.shape == (0, D) and ld.shape == (0,)
