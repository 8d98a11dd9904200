"""GPU: the weight-stream RealNVP kernels (csrc/nfk_wide_rnvp.hip) called
directly -- K_.wlin_pack, K_.WideRnvpPack, K_.wide_rnvp, K_.WideRnvpChain,
K_.wide_rnvp_chain and the C entries with a workspace of the test's own --
on packs built from the test's own fp32 tensors (widernvp.make_layer), at
every row-tile count, split-K plan, width edge and calling convention.

Two rules (widernvp.py):

* masters -- rows X[:64] (the fused GEMM + tanh stages, MT 4) and X[:128]
  (split-K, MT 8) of every shape and direction -- against the fp64 CPU
  reference: max and p99 error within 2 x the fp32 CPU reference's own, for z
  and for log|det|, no additive floor;
* every other run bitwise equal, pass by pass, to the same rows of the master
  of its group (passes of <= 64 rows: the 64-row master; 65 ... 128: the
  128-row master).  A row's result does not depend on its batch: MFMA columns
  are independent, k_wl_gemm_act splits k over its waves by KB only and adds
  them in wave order, wl_plan's KS / KC depend on N and KB only, and
  k_wl_act / k_wl_rows add the splits in order.

The stage plans (widernvp.plan_table; test_wide_rnvp_split_cpu.py asserts
what each shape is there for).  A plan with KS = 1 needs N >= 8208 and
hidden-by-hidden weights of 270 MB each: left out on purpose.

    half hidden stage    N     K  NT nblk  KB  KS  KC last | fused: KW waves last
       4     16    L1   16     4   1    1   1   1   1    1 |         1     1    1
       4     16    L2   16    16   1    1   1   1   1    1 |         1     1    1
       4     16    L3    4    16   1    1   1   1   1    1 |
      20    300    L1  300    20  19    3   1   1   1    1 |         1     1    1
      20    300    L2  300   300  19    3  10  10   1    1 |         3     4    1
      20    300    L3   20   300   2    1  10  10   1    1 |
      36     44    L1   44    36   3    1   2   2   1    1 |         1     2    1
      36     44    L2   44    44   3    1   2   2   1    1 |         1     2    1
      36     44    L3   36    44   3    1   2   2   1    1 |
      60     52    L1   52    60   4    1   2   2   1    1 |         1     2    1
      60     52    L2   52    52   4    1   2   2   1    1 |         1     2    1
      60     52    L3   60    52   4    1   2   2   1    1 |
     132    260    L1  260   132  17    3   5   5   1    1 |         2     3    1
     132    260    L2  260   260  17    3   9   9   1    1 |         3     3    3
     132    260    L3  132   260   9    2   9   9   1    1 |
     128    256    L1  256   128  16    2   4   4   1    1 |         1     4    1
     128    256    L2  256   256  16    2   8   8   1    1 |         2     4    2
     128    256    L3  128   256   8    1   8   8   1    1 |
     512   1100    L1 1100   512  69    9  16   8   2    2 |         4     4    4
     512   1100    L2 1100  1100  69    9  35  12   3    2 |         9     4    8
     512   1100    L3  512  1100  32    4  35  18   2    1 |
    2052   2048    L1 2048  2052 128   16  65   8   9    2 |        17     4   14
    2052   2048    L2 2048  2048 128   16  64   8   8    8 |        16     4   16
    2052   2048    L3 2052  2048 129   17  64   7  10    4 |

Which test runs which kernel instance:

* k_wl_gemm_act<1,8> <2,8> <3,6> <4,6>: test_every_row_tile_count (batches 1 / 15,
  16 / 17, 33 / 48 / 49, 63) and the 64-row masters (<4,6>);
* k_wl_gemm<1..4,2,4,8> (L3 of the fused passes): the same runs;
  <5..8,2,4,8> (all three stages): batches 65 / 81 / 97 / 113, 127, 129 and
  the 128-row masters; second and third passes of MT 1, 4, 5: 129, 192, 200, 257;
* k_wl_gemm<1..4,1,8,16> and <1..4,2,4,10> (NFK_WL_CFG=1 / 2): test_ab_instances
  (rows 1, 17, 33, 64 in a child process each);
* k_wl_act at MT <= 4: test_ab_instances (NFK_WL_FUSED=0); at MT > 4: every
  run above 64 rows;
* k_wl_rows as the input split, as the coupling that writes the next
  fragments and as the last coupling: every run; the last coupling of a layer
  writing the next layer's fragments: test_chain_bitwise_per_layer.

Measured on an MI355X against the fp64 reference, the largest ratio (kernel
error / fp32 reference error; max or p99, z or log|det|; both directions,
64 and 128 rows) per shape and gain:

    half hidden   gain 1   gain 3
       4     16     1.22     1.54  (2.62 with the coupling in fp32)
      20    300     1.06     0.94
      36     44     1.37     0.99
      60     52     1.17     1.00
     132    260     1.44     0.91
     128    256     1.20     1.11
     512   1100     0.82     0.74  (1.71 / 1.85 with one accumulator per tile)
    2052   2048     1.46        -  (3.29 with one)

What these tests found, both fixed in nfk_wide_rnvp.hip:

* With one accumulator per tile, k_wl_gemm's partial sums were low by 2e-10
  per s on average (0.03 ulp of s), whatever the sign of the sum: read back
  from the workspace and compared with the exact products of the very
  fragments the GEMM read, the L3 partial sums were off by -7 units of the
  scaled accumulator per element at (512, 1100) and at (2052, 2048), where
  the restatement's round-to-nearest accumulation has no such offset.  Summed
  over the 2 half columns of log|det| the offset grows linearly while
  rounding errors grow as the root: -8.4e-07 +- 3.3e-07 per row at
  (2052, 2048), 3.29 x the fp32 reference's error.  k_wl_gemm now adds the
  even k-blocks of a chunk to one accumulator and the odd ones, negated, to a
  second, and writes the difference: the offset cancels.
* The coupling (x - t) expf(-s) in fp32 was 1.5 ulp off at the largest
  outputs: at (4, 16), gain 3, inverse, z = 2.0502545 came out as 2.05025482
  where the restatement with the host's exp gave 2.05025458 -- the value one
  ulp more of exp(-s) gives.  3.63e-07 against the reference's 1.39e-07
  (2.62 x).  k_wl_rows now evaluates the coupling and its exp in double and
  rounds once.
"""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

import widernvp as wr  # noqa: E402
from normalizingflow_amd import kernels as K_  # noqa: E402

pytestmark = pytest.mark.gpu

MASTERS = [(s, g) for s in wr.SHAPES for g in (1, 3) if not (s == wr.LARGE and g == 3)]
EDGE = [(36, 44), (132, 260)]
SENT = 12345.0


def _mid(case):
    return "%s-g%d" % (wr.ids(case[0]), case[1])


def pack_layer(Ws, bs, dev):
    half, hidden = Ws[4].shape
    packs = [K_.wlin_pack(W.to(dev)) for W in Ws]
    return K_.WideRnvpPack(packs, [b.to(dev).contiguous() for b in bs], half, hidden)


def run(wp, x, inverse, mode=1, ld=None, z=None):
    z = torch.full_like(x, float("nan"), memory_format=torch.contiguous_format) if z is None else z
    if mode != 0 and ld is None:
        ld = torch.full((x.shape[0],), float("nan"), device=x.device)
    K_.wide_rnvp(x, wp, z, logdet=ld if mode != 0 else None, logdet_mode=mode, inverse=inverse)
    return z, (ld if mode != 0 else None)


class Case:
    """One shape and gain: weights, X, the device pack, and (lazily) the
    references and the two masters per direction, each computed once."""

    def __init__(self, shape, gain, dev):
        self.shape, self.gain, self.dev = shape, gain, dev
        self.half, self.hidden = shape
        self.Ws, self.bs = wr.make_layer(*shape, gain)
        self.X = wr.make_x(self.half)
        self.Xd = self.X.to(dev)
        self.wp = pack_layer(self.Ws, self.bs, dev)
        self._refs, self._masters = {}, {}

    def refs(self, inverse, rows):
        """(z64, ld64, z32, ld32) of X[:rows]: computed once at 128 rows."""
        if inverse not in self._refs:
            self._refs[inverse] = wr.refs(self.X, self.Ws, self.bs, inverse)
        return tuple(t[:rows] for t in self._refs[inverse])

    def master(self, inverse, rows):
        key = (inverse, rows)
        if key not in self._masters:
            self._masters[key] = run(self.wp, self.Xd[:rows], inverse)
            torch.cuda.synchronize()
        return self._masters[key]

    def expect(self, inverse, m):
        """The first m rows of the master of an m-row pass."""
        z, ld = self.master(inverse, 64 if m <= 64 else 128)
        return z[:m], ld[:m]


_CASES = {}


def case(shape, gain, dev):
    key = (shape, gain)
    if key not in _CASES:
        _CASES[key] = Case(shape, gain, dev)
    return _CASES[key]


class counted:
    """The launches of the wrappers inside the block, by entry point."""

    def __enter__(self):
        K_.TIMER = K_.KernelTimer()
        self.n = None
        return self

    def __exit__(self, *exc):
        try:
            torch.cuda.synchronize()
            self.n = {k: v[0] for k, v in K_.TIMER.summary().items()}
        finally:
            K_.TIMER = None


# ---------------------------------------------------------------------------
# 1. masters
@pytest.mark.parametrize("cs", MASTERS, ids=_mid)
def test_masters_vs_fp64(cs, hip_device):
    """The error rule, z and log|det|, both directions, 64 and 128 rows."""
    c = case(*cs, hip_device)
    bad, worst = [], 0.0
    for inverse in (False, True):
        for rows in (64, 128):
            z, ld = c.master(inverse, rows)
            z64, ld64, z32, ld32 = c.refs(inverse, rows)
            label = "%s %s %d" % (_mid(cs), "inv" if inverse else "fwd", rows)
            for what, k, r, t in (("z", z, z32, z64), ("ld", ld, ld32, ld64)):
                ok, ratio = wr.rule(k, r, t, label + " " + what)
                worst = max(worst, ratio)
                if not ok:
                    bad.append("%s %s %.2f" % (label, what, ratio))
    print("largest ratio %s: %.2f" % (_mid(cs), worst))
    assert not bad, bad


@pytest.mark.parametrize("cs", MASTERS, ids=_mid)
def test_masters_round_trip(cs, hip_device):
    """inverse(forward(x)) = x to twice the fp32 reference's own round-trip error."""
    c = case(*cs, hip_device)
    for rows in (64, 128):
        zf, _ = c.master(False, rows)
        xk, _ = run(c.wp, zf, True)
        x = c.X[:rows]
        z32 = wr.rnvp_ref(x, c.Ws, c.bs, False, torch.float32)[0]
        x32 = wr.rnvp_ref(z32, c.Ws, c.bs, True, torch.float32)[0]
        ek, er = float((xk.cpu() - x).abs().max()), float((x32 - x).abs().max())
        print("round trip %s %d rows: max |x' - x| ours %.3g ref %.3g ratio %.2f" % (_mid(cs), rows, ek, er, ek / er))
        assert ek <= wr.FACTOR * er, (ek, er)


# ---------------------------------------------------------------------------
# 2. every row-tile count
@pytest.mark.parametrize("inverse", [False, True], ids=["fwd", "inv"])
@pytest.mark.parametrize("shape", wr.SMALL, ids=wr.ids)
def test_every_row_tile_count(shape, inverse, hip_device):
    c = case(shape, 1, hip_device)
    outs = []
    with counted() as cnt:
        for B in wr.BATCHES:
            outs.append(run(c.wp, wr.batch_of(c.Xd, B), inverse))
    assert cnt.n == {"nfk_wide_rnvp": len(wr.BATCHES)}, cnt.n
    for B, (z, ld) in zip(wr.BATCHES, outs):
        for r0, m in wr.passes(B):
            ez, eld = c.expect(inverse, m)
            assert torch.equal(z[r0:r0 + m], ez), "z: batch %d, pass at row %d (%d rows)" % (B, r0, m)
            assert torch.equal(ld[r0:r0 + m], eld), "log|det|: batch %d, pass at row %d (%d rows)" % (B, r0, m)


# ---------------------------------------------------------------------------
# 3. calling convention
def _strided(x, pad_l, pad_r, fill):
    buf = torch.full((x.shape[0], x.shape[1] + pad_l + pad_r), fill, device=x.device)
    view = buf[:, pad_l:pad_l + x.shape[1]]
    if not (isinstance(fill, float) and fill != fill):
        view.fill_(float("nan"))
    return buf, view


def _pads_intact(buf, pad_l, cols, before):
    a, b = buf.clone(), before.clone()
    a[:, pad_l:pad_l + cols] = 0
    b[:, pad_l:pad_l + cols] = 0
    return torch.equal(a.view(torch.int32), b.view(torch.int32))


@pytest.mark.parametrize("inverse", [False, True], ids=["fwd", "inv"])
@pytest.mark.parametrize("rows", [49, 130])
@pytest.mark.parametrize("shape", EDGE, ids=wr.ids)
def test_strides_modes_and_aliasing(shape, rows, inverse, hip_device):
    c = case(shape, 1, hip_device)
    x = wr.batch_of(c.Xd, rows)
    zc, ldc = run(c.wp, x, inverse)
    for r0, m in wr.passes(rows):
        ez, eld = c.expect(inverse, m)
        assert torch.equal(zc[r0:r0 + m], ez) and torch.equal(ldc[r0:r0 + m], eld)
    # x and z as column slices of wider buffers: ldx != ldz != 2 half, views at a non-zero column
    xbuf, xv = _strided(x, 3, 4, float("nan"))
    xv.copy_(x)
    zbuf, zv = _strided(x, 5, 7, SENT)
    xb0, zb0 = xbuf.clone(), zbuf.clone()
    assert xv.stride(0) != zv.stride(0) and xv.stride(0) != 2 * c.half and zv.stride(0) != 2 * c.half
    _, lds = run(c.wp, xv, inverse, z=zv)
    assert torch.equal(zv, zc) and torch.equal(lds, ldc)
    assert torch.equal(xbuf.view(torch.int32), xb0.view(torch.int32))
    assert _pads_intact(zbuf, 5, 2 * c.half, zb0)
    # logdet_mode 0: no log|det|, z bitwise; 2 on zeros: bitwise mode 1; 2 on a
    # preset p: fl(fl(p + a) + b) against p + fl(a + b), a and b the two
    # couplings' sums: three roundings of 2^-24 each, of |p + a|, |p + a + b|
    # <= |p| + S and |a + b| <= S, S = sum |s| of the row (1.001: S is the
    # reference's, a and b the kernel's)
    z0, none = run(c.wp, x, inverse, mode=0)
    assert none is None and torch.equal(z0, zc)
    z2, ld2 = run(c.wp, x, inverse, mode=2, ld=torch.zeros(rows, device=hip_device))
    assert torch.equal(z2, zc) and torch.equal(ld2, ldc)
    p = torch.linspace(-3.0, 5.0, rows, device=hip_device)
    z2, ld2 = run(c.wp, x, inverse, mode=2, ld=p.clone())
    assert torch.equal(z2, zc)
    sabs = wr.rnvp_ref(x.cpu(), c.Ws, c.bs, inverse, torch.float64)[3]
    err = (ld2.cpu().double() - (p.cpu().double() + ldc.cpu().double())).abs()
    assert bool((err <= 1.001 * 2.0 ** -24 * (2 * p.cpu().double().abs() + 3 * sabs)).all()), float(err.max())
    # z aliasing x
    xi = x.clone()
    _, ldi = run(c.wp, xi, inverse, z=xi)
    assert torch.equal(xi, zc) and torch.equal(ldi, ldc)


# ---------------------------------------------------------------------------
# 4. the chain
_CHAINS = {}


def _chain_layers(shape, dev):
    if shape not in _CHAINS:
        _CHAINS[shape] = [pack_layer(*wr.make_layer(*shape, 1, seed=wr.SEED + 10 + l), dev) for l in range(4)]
    return _CHAINS[shape]


def _per_layer(wps, x, inverse, mode, ld):
    cur = x
    for i, wp in enumerate(wps):
        cur, ld = run(wp, cur, inverse, mode=(mode if i == 0 else 2) if mode != 0 else 0, ld=ld)
    return cur, ld


@pytest.mark.parametrize("nlayers", [1, 2, 3, 4])
@pytest.mark.parametrize("shape", EDGE, ids=wr.ids)
def test_chain_bitwise_per_layer(shape, nlayers, hip_device):
    """nfk_wide_rnvp_chain = the per-layer nfk_wide_rnvp calls (the inverse:
    the layers last to first), bitwise: both ping-pong parities, one and two
    row blocks (200 rows: a second pass of MT 5), strided x / z, every
    logdet mode, z aliasing x; one launch per call."""
    half = shape[0]
    layers = _chain_layers(shape, hip_device)[:nlayers]
    X = wr.make_x(half, rows=200, seed=wr.SEED + 3).to(hip_device)
    for inverse in (False, True):
        wps = list(reversed(layers)) if inverse else layers
        chain = K_.WideRnvpChain(wps)
        for rows in (40, 100, 200):
            x = X[:rows]
            for mode in (0, 1, 2):
                preset = torch.linspace(-1.0, 2.0, rows, device=hip_device)
                ld_e = preset.clone() if mode == 2 else None
                ze, ld_e = _per_layer(wps, x, inverse, mode, ld_e)
                xbuf, xv = _strided(x, 1, 2, float("nan"))
                xv.copy_(x)
                zbuf, zv = _strided(x, 6, 3, SENT)
                zb0 = zbuf.clone()
                ld = preset.clone() if mode == 2 else (torch.full((rows,), float("nan"), device=hip_device)
                                                       if mode == 1 else None)
                with counted() as cnt:
                    K_.wide_rnvp_chain(xv, chain, zv, logdet=ld, logdet_mode=mode, inverse=inverse)
                where = "%d layers, %s, %d rows, mode %d" % (nlayers, "inv" if inverse else "fwd", rows, mode)
                assert cnt.n == {"nfk_wide_rnvp_chain": 1}, cnt.n
                assert torch.equal(zv, ze), where
                assert mode == 0 or torch.equal(ld, ld_e), where
                assert _pads_intact(zbuf, 6, 2 * half, zb0), where
            xi = x.clone()
            ldi = torch.empty(rows, device=hip_device)
            K_.wide_rnvp_chain(xi, chain, xi, logdet=ldi, logdet_mode=1, inverse=inverse)
            ze, ld_e = _per_layer(wps, x, inverse, 1, None)
            assert torch.equal(xi, ze) and torch.equal(ldi, ld_e), "in place, %d rows" % rows


# ---------------------------------------------------------------------------
# 5. the workspace
def _raw(entry, x, z, ld, mode, inverse, pk, bs, half, hidden, ws, nws, nlayers=None, batch=None, ldx=None, ldz=None):
    """The C entry itself (include/nfk.h nfk_wide_rnvp / nfk_wide_rnvp_chain)."""
    dev = x.device
    args = [x.data_ptr(), x.stride(0) if ldx is None else ldx, pk, bs]
    if nlayers is not None:
        args.append(nlayers)
    args += [half, hidden, z.data_ptr(), z.stride(0) if ldz is None else ldz, None if ld is None else ld.data_ptr(),
             mode, x.shape[0] if batch is None else batch, 1 if inverse else 0, None if ws is None else ws.data_ptr(),
             nws, torch.cuda.current_stream(dev).cuda_stream]
    return K_._lib.call(entry, *args)


def _poisoned(n, dev, tail=4096):
    """n floats of 0xFF bytes (NaN as float and as half) and a sentinel tail."""
    buf = torch.full((4 * (n + tail),), 0xFF, dtype=torch.uint8, device=dev).view(torch.float32)
    buf[n:] = SENT
    return buf


@pytest.mark.parametrize("inverse", [False, True], ids=["fwd", "inv"])
@pytest.mark.parametrize("shape", [(20, 300), (132, 260)], ids=wr.ids)
def test_workspace_written_before_read_and_bounded(shape, inverse, hip_device):
    """With the workspace NaN-filled (as floats and as halfs) the results are
    bitwise the wrapper's: every fragment, pad feature and partial sum a stage
    reads was written by the stage before it; nothing is written past
    nfk_wide_rnvp_workspace floats."""
    c = case(shape, 1, hip_device)
    lib = K_._lib.load()
    for rows in (1, 17, 64, 65, 129):
        x = wr.batch_of(c.Xd, rows)
        n = int(lib.nfk_wide_rnvp_workspace(c.half, c.hidden, rows))
        ws = _poisoned(n, hip_device)
        z, ld = torch.full_like(x, SENT), torch.full((rows,), SENT, device=hip_device)
        _raw("nfk_wide_rnvp", x, z, ld, 1, inverse, c.wp.pk, c.wp.bs, c.half, c.hidden, ws, n)
        for r0, m in wr.passes(rows):
            ez, eld = c.expect(inverse, m)
            assert torch.equal(z[r0:r0 + m], ez) and torch.equal(ld[r0:r0 + m], eld), rows
        assert bool((ws[n:] == SENT).all()), "written past the workspace at %d rows" % rows
        # one float too few
        z.fill_(SENT)
        with pytest.raises(ValueError, match="workspace too small"):
            _raw("nfk_wide_rnvp", x, z, ld, 1, inverse, c.wp.pk, c.wp.bs, c.half, c.hidden, ws, n - 1)
        torch.cuda.synchronize()
        assert bool((z == SENT).all())


@pytest.mark.parametrize("shape", [(20, 300), (132, 260)], ids=wr.ids)
def test_chain_workspace_written_before_read_and_bounded(shape, hip_device):
    layers = _chain_layers(shape, hip_device)[:3]
    chain = K_.WideRnvpChain(layers)
    half, hidden = shape
    lib = K_._lib.load()
    X = wr.make_x(half, rows=129, seed=wr.SEED + 4).to(hip_device)
    for rows in (1, 17, 64, 65, 129):
        x = X[:rows]
        ze, lde = torch.empty_like(x), torch.empty(rows, device=hip_device)
        K_.wide_rnvp_chain(x, chain, ze, logdet=lde, logdet_mode=1)
        n = int(lib.nfk_wide_rnvp_chain_workspace(half, hidden, rows))
        assert n == int(lib.nfk_wide_rnvp_workspace(half, hidden, rows)) + 128 * 2 * half
        ws = _poisoned(n, hip_device)
        z, ld = torch.full_like(x, SENT), torch.full((rows,), SENT, device=hip_device)
        _raw("nfk_wide_rnvp_chain", x, z, ld, 1, False, chain.pk, chain.bs, half, hidden, ws, n, nlayers=3)
        assert torch.equal(z, ze) and torch.equal(ld, lde), rows
        assert bool((ws[n:] == SENT).all()), "written past the workspace at %d rows" % rows
        z.fill_(SENT)
        with pytest.raises(ValueError, match="workspace too small"):
            _raw("nfk_wide_rnvp_chain", x, z, ld, 1, False, chain.pk, chain.bs, half, hidden, ws, n - 1, nlayers=3)
        torch.cuda.synchronize()
        assert bool((z == SENT).all())


# ---------------------------------------------------------------------------
# 6. nfk_wlin_pack against its definition
def _pack_raw(W):
    """nfk_wlin_pack into a block of 0xFF bytes of the test's own."""
    N, K = W.shape
    n = int(K_._lib.load().nfk_wlin_pack_floats(N, K))
    buf = _poisoned(n, W.device, tail=64)
    K_._lib.call("nfk_wlin_pack", W.data_ptr(), N, K, buf.data_ptr(), torch.cuda.current_stream(W.device).cuda_stream)
    assert bool((buf[n:] == SENT).all())
    return buf[:n]


def _check_pack(W, dev):
    N, K = W.shape
    Wd = W.to(dev).contiguous()
    pack = _pack_raw(Wd)
    hdr, body, tail = wr.pack_decode(pack, N, K)
    rh, rb, rt = wr.wlin_pack_ref(W)
    ex, mx = wr.pack_exp(W)
    assert float(hdr[0]) == 2.0 ** (ex - 15) and float(hdr[1]) == mx
    assert torch.equal(hdr.view(torch.int32), rh.view(torch.int32))  # (words 2 ... 63 zero)
    assert torch.equal(tail, rt)
    diff = body != rb
    assert not bool(diff.any()), "%d of %d halfs differ, first at [nt, kb, part, lane, j] = %s" % (
        int(diff.sum()), diff.numel(), diff.nonzero()[0].tolist())
    # packed a second time into the same poisoned block, and through the wrapper: the same words
    assert torch.equal(_pack_raw(Wd).view(torch.int32), pack.view(torch.int32))
    assert torch.equal(K_.wlin_pack(Wd).view(torch.int32), pack.view(torch.int32))
    # what hi + lo still holds of 2^s w: 2^-22 |2^s w|, or 2^-25 where lo is a subnormal half
    h = body.view(torch.float16).double()
    NT, KB = body.shape[:2]
    back = (h[:, :, 0] + h[:, :, 1]).view(NT, KB, 4, 16, 8).permute(0, 3, 1, 2, 4).reshape(16 * NT, 32 * KB)
    ws = W.double() * 2.0 ** (15 - ex)
    err = (back[:N, :K] - ws).abs()
    assert bool((err <= torch.maximum(ws.abs() * 2.0 ** -22, torch.tensor(2.0 ** -25, dtype=torch.float64))).all())
    assert float(back[N:].abs().max() if 16 * NT > N else 0.0) == 0.0
    assert float(back[:, K:].abs().max() if 32 * KB > K else 0.0) == 0.0


@pytest.mark.parametrize("NK", [(16, 4), (20, 40), (44, 36), (300, 20), (1100, 512)], ids=lambda s: "%dx%d" % s)
def test_wlin_pack_vs_reference(NK, hip_device):
    N, K = NK
    g = torch.Generator().manual_seed(N + K)
    _check_pack((torch.rand(N, K, generator=g) * 2 - 1) * 3.7 / K ** 0.5, hip_device)


@pytest.mark.parametrize("kind", ["zero", "pow2", "below-pow2", "one-large"])
def test_wlin_pack_special_matrices(kind, hip_device):
    N, K = 44, 36
    W = (torch.rand(N, K, generator=torch.Generator().manual_seed(9)) * 2 - 1) * 0.2
    if kind == "zero":
        W.zero_()                        # max|W| = 0: scale 2^15, every half zero
    elif kind == "pow2":
        W[17, 33] = -0.25                # max|W| = 2^-2 exactly: 2^s max = 2^14
    elif kind == "below-pow2":
        W[17, 33] = float(np.nextafter(np.float32(0.25), np.float32(0)))  # 2^s max = 2^15 (1 - 2^-24): hi = 2^15
    else:
        W[17, 33] = 0.2 * 2.0 ** 18      # the rest below 2^-3 after scaling: lo a subnormal half
    _check_pack(W, hip_device)
    if kind == "one-large":
        body = wr.wlin_pack_ref(W)[1].view(torch.float16)
        lo = body[:, :, 1].float().abs()
        assert bool(((lo > 0) & (lo < 2.0 ** -14)).any())  # (the case is what it says)


# ---------------------------------------------------------------------------
# 7. value edges
@pytest.mark.parametrize("rows", [20, 70])
@pytest.mark.parametrize("shape", EDGE, ids=wr.ids)
def test_zero_last_linear_is_identity(shape, rows, hip_device):
    c = case(shape, 1, hip_device)
    Ws, bs = list(c.Ws), list(c.bs)
    for cc in range(2):
        for g in range(2):
            Ws[6 * cc + 4 + g] = torch.zeros_like(Ws[6 * cc + 4 + g])
            bs[6 * cc + 4 + g] = torch.zeros_like(bs[6 * cc + 4 + g])
    wp = pack_layer(Ws, bs, hip_device)
    x = c.Xd[:rows]
    for inverse in (False, True):
        z, ld = run(wp, x, inverse)
        assert torch.equal(z, x) and bool((ld == 0).all())


def _edge_rows(c, rows):
    x = c.X[:rows].clone()
    x[3] = 0.0
    x[5, 7] = 1.0e4
    x[6, c.half + 2] = -1.0e4
    x[9] *= 1.0e-30
    return x


@pytest.mark.parametrize("rows", [20, 70])
@pytest.mark.parametrize("shape", EDGE, ids=wr.ids)
def test_scaled_and_non_finite_rows(shape, rows, hip_device):
    """A zero row, rows with one coordinate +-1e4 (in either half), a row
    scaled by 1e-30 (the e >= -64 clamp of the per-row scale) among ordinary
    rows: the error rule over the batch.  Then one row swapped for NaN: every
    other row is bitwise unchanged."""
    c = case(shape, 1, hip_device)
    x = _edge_rows(c, rows)
    xd = x.to(hip_device)
    bad = []
    for inverse in (False, True):
        z, ld = run(c.wp, xd, inverse)
        z64, ld64, z32, ld32 = wr.refs(x, c.Ws, c.bs, inverse)
        label = "%s edge rows %s %d" % (wr.ids(shape), "inv" if inverse else "fwd", rows)
        for what, k, r, t in (("z", z, z32, z64), ("ld", ld, ld32, ld64)):
            ok, ratio = wr.rule(k, r, t, label + " " + what)
            if not ok:
                bad.append("%s %s %.2f" % (label, what, ratio))
        xn = xd.clone()
        xn[4] = float("nan")
        zn, ldn = run(c.wp, xn, inverse)
        keep = [i for i in range(rows) if i != 4]
        assert torch.equal(zn[keep], z[keep]) and torch.equal(ldn[keep], ld[keep])
        assert bool(torch.isnan(zn[4]).any())
    assert not bad, bad


# ---------------------------------------------------------------------------
# 8. arguments
def test_supported_truth_table():
    lib = K_._lib.load()
    for half, ok in ((0, 0), (3, 0), (4, 1), (6, 0), (16384, 1), (16388, 0)):
        assert lib.nfk_wide_rnvp_supported(half, 64) == ok, half
        assert (lib.nfk_wide_rnvp_workspace(half, 64, 10) > 0) == bool(ok), half
    for hidden, ok in ((12, 0), (16, 1), (18, 0), (20, 1), (16384, 1), (16388, 0)):
        assert lib.nfk_wide_rnvp_supported(64, hidden) == ok, hidden
        assert (lib.nfk_wide_rnvp_chain_workspace(64, hidden, 10) > 0) == bool(ok), hidden
    assert lib.nfk_wide_rnvp_workspace(64, 64, 0) == 0


def test_bad_arguments_raise_and_launch_nothing(hip_device):
    c = case((36, 44), 1, hip_device)
    h, H, rows = c.half, c.hidden, 20
    x = c.Xd[:rows].contiguous()
    z = torch.full_like(x, SENT)
    ld = torch.full((rows,), SENT, device=hip_device)
    n = int(K_._lib.load().nfk_wide_rnvp_chain_workspace(h, H, rows))
    ws = torch.zeros(n, device=hip_device)
    one = dict(pk=c.wp.pk, bs=c.wp.bs, half=h, hidden=H, ws=ws, nws=n)
    with pytest.raises(ValueError, match="leading dimension"):
        _raw("nfk_wide_rnvp", x, z, ld, 1, False, ldx=2 * h - 1, **one)
    with pytest.raises(ValueError, match="leading dimension"):
        _raw("nfk_wide_rnvp", x, z, ld, 1, False, ldz=2 * h - 1, **one)
    with pytest.raises(ValueError, match="null logdet"):
        _raw("nfk_wide_rnvp", x, z, None, 1, False, **one)
    with pytest.raises(ValueError, match="null logdet"):
        _raw("nfk_wide_rnvp_chain", x, z, None, 2, False, nlayers=1, **one)
    with pytest.raises(ValueError, match="layer count"):
        _raw("nfk_wide_rnvp_chain", x, z, ld, 1, False, nlayers=0, **one)
    with pytest.raises(ValueError, match="bad batch"):
        _raw("nfk_wide_rnvp", x, z, ld, 1, False, batch=-1, **one)
    with pytest.raises(ValueError, match="null pointer"):
        _raw("nfk_wide_rnvp", x, z, ld, 1, False, **dict(one, ws=None))
    holed = (ctypes.c_void_p * 12)(*[t.data_ptr() for t in c.wp.packs])
    holed[7] = None
    with pytest.raises(ValueError, match="null pack or bias"):
        _raw("nfk_wide_rnvp", x, z, ld, 1, False, **dict(one, pk=ctypes.addressof(holed)))
    with pytest.raises(ValueError, match="not supported"):
        _raw("nfk_wide_rnvp", x, z, ld, 1, False, **dict(one, half=h + 2))
    with pytest.raises(ValueError, match="not supported"):
        _raw("nfk_wide_rnvp_chain", x, z, ld, 1, False, nlayers=1, **dict(one, hidden=12))
    # batch 0: nothing to do, no error
    assert _raw("nfk_wide_rnvp", x, z, ld, 1, False, batch=0, **one) == 0
    assert _raw("nfk_wide_rnvp_chain", x, z, ld, 1, False, batch=0, nlayers=1, **one) == 0
    torch.cuda.synchronize()
    assert bool((z == SENT).all()) and bool((ld == SENT).all())
    # the wrappers' own checks
    with pytest.raises(ValueError):
        K_.wide_rnvp(x[:, :-1], c.wp, z[:, :-1], logdet=ld, logdet_mode=1)
    with pytest.raises(ValueError):
        K_.WideRnvpPack(c.wp.packs[:11], c.wp.biases[:11], h, H)
    with pytest.raises(ValueError):
        K_.wlin_pack(torch.zeros(4, device=hip_device))


# ---------------------------------------------------------------------------
# 9. the A/B instances: NFK_WL_FUSED / NFK_WL_CFG are read once per process
AB_ROWS = (1, 17, 33, 64)


def _ab_cases(dev):
    """name -> array: the six small shapes, both directions, rows 1, 17, 33, 64."""
    out = {}
    for shape in wr.SMALL:
        c = case(shape, 1, dev)
        for inverse in (False, True):
            for rows in AB_ROWS:
                z, ld = run(c.wp, c.Xd[:rows], inverse)
                key = "%d_%d_%d_%d" % (shape[0], shape[1], int(inverse), rows)
                out[key + "_z"], out[key + "_ld"] = z.cpu().numpy(), ld.cpu().numpy()
    return out


def test_ab_instances(tmp_path, hip_device):
    """The instances behind the A/B switches, one child process at a time:
    NFK_WL_CFG=1 / 2 (k_wl_gemm<1..4,1,8,16> / <1..4,2,4,10> for L3: the same
    tiles and k order) give the 64-row master's rows bitwise; NFK_WL_FUSED=0
    (split-K GEMM + k_wl_act for L1 and L2 at <= 64 rows) gives the 128-row
    master's rows bitwise.  Each child's 64-row results meet the error rule."""
    for name, value in (("NFK_WL_FUSED", "0"), ("NFK_WL_CFG", "1"), ("NFK_WL_CFG", "2")):
        path = str(tmp_path / ("%s_%s.npz" % (name, value)))
        env = dict(os.environ)
        env.pop("NFK_WL_FUSED", None)
        env.pop("NFK_WL_CFG", None)
        env[name] = value
        flags = ["-s"] if sys.flags.no_user_site else []
        r = subprocess.run([sys.executable] + flags + [os.path.abspath(__file__), path], env=env, timeout=300,
                           stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
        assert r.returncode == 0, "%s=%s: exit %d\n%s" % (name, value, r.returncode, r.stdout.decode()[-2000:])
        got = np.load(path)
        split = name == "NFK_WL_FUSED"
        differs, bad = 0, []
        for shape in wr.SMALL:
            c = case(shape, 1, hip_device)
            for inverse in (False, True):
                mz, mld = c.master(inverse, 128 if split else 64)
                fz, fld = c.master(inverse, 64)
                for rows in AB_ROWS:
                    key = "%d_%d_%d_%d" % (shape[0], shape[1], int(inverse), rows)
                    z, ld = torch.from_numpy(got[key + "_z"]), torch.from_numpy(got[key + "_ld"])
                    where = "%s=%s %s" % (name, value, key)
                    assert torch.equal(z, mz[:rows].cpu()), where
                    assert torch.equal(ld, mld[:rows].cpu()), where
                    differs += int(not torch.equal(z, fz[:rows].cpu()))
                    if rows == 64:
                        z64, ld64, z32, ld32 = c.refs(inverse, 64)
                        for what, k, r_, t in (("z", z, z32, z64), ("ld", ld, ld32, ld64)):
                            ok, ratio = wr.rule(k, r_, t, where + " " + what)
                            if not ok:
                                bad.append("%s %s %.2f" % (where, what, ratio))
        # (the split-K sums round differently from the four waves' sums somewhere: the switch was read)
        assert differs > 0 if split else differs == 0
        assert not bad, bad


if __name__ == "__main__":
    if len(sys.argv) != 2:
        sys.exit("usage: python tests/test_gpu_wide_rnvp_kernels.py OUT.npz  (a child of test_ab_instances)")
    np.savez(sys.argv[1], **_ab_cases(torch.device("cuda:0")))
