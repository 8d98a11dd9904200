"""Shared pieces of test_gpu_row_kernels*.py: shapes, fp64 / fp32 CPU references
with autograd, operand layouts and the comparison rule.

Reference: plain torch on the CPU, evaluated in fp64 on the fp32 inputs
converted to double; the same function in fp32 runs alongside and decides
only whether a case may use the on-par fallback (``check_rows`` /
``check_sums``).  Gradients are autograd's, of ``(z * gz).sum() + (ld * gld).sum()``
with the term of a null cotangent dropped.
"""
import math
import os

import torch

from oracle import nf_oracle as orc
from test_gpu_grad import GRAD_TOL, rel_close
from test_gpu_parity import on_par

NAN = float("nan")
NLS = ["tanh", "leaky_relu", "elu"]

# width -> lane-group width W of the templated row kernels (lanes_for), column
# blocks of k_colsum_part (64 columns each) and blocks of k_colsum_final (256):
#   1 -> W 1 | 2 -> W 2 | 3, 4 -> W 4 | 5, 8 -> W 8 | 9, 16 -> W 16 | 17, 32 -> W 32
#   33, 63, 64 -> W 64, one trip | 65 ... 16384 -> W 64, 2 ... 256 trips
#   column blocks: <= 64 -> 1, 65 ... 128 -> 2, 257 -> 5, 16384 -> 256
#   final blocks: <= 256 -> 1, 257 and up -> 2 or more (also the second trip of
#   the 256-thread loops of planar_uhat / k_planar_bwd_params / k_radial_bwd_scalars)
WIDTHS = [1, 2, 3, 4, 5, 8, 9, 16, 17, 32, 33, 63, 64, 65, 100, 128, 129, 256, 257, 1000, 16384]
# 67: no multiple of the rows per wave (64 / W) or per block of any W, so the
# last wave is ragged; 259: two column-sum chunks of 130 and 129 rows
BATCHES = [1, 3, 67, 259]
SHAPES = [(3 if d >= 1000 else 67, d) for d in WIDTHS] + [(b, d) for b in (1, 3, 259) for d in (1, 5, 64, 65, 257)]
STRIDED = [(67, 5), (67, 64), (67, 100)]
NULLS = [(67, 5), (67, 65)]
GRID_STRIDE = (70001, 61)  # batch * n > 16,384 blocks * 256 threads


def lanes_for(n):
    w = 1
    while w < n and w < 64:
        w <<= 1
    return w


def ids(shape):
    return "b%d-d%d" % shape


def rnd(seed, *shape, scale=1.0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale


def uni(seed, n, bound):
    return (torch.rand(n, generator=torch.Generator().manual_seed(seed)) * 2 - 1) * bound


class Layout:
    """Device operands of one case.  Contiguous: plain tensors, outputs
    NaN-filled.  Strided: every matrix is the view [:, 1:1+cols] of its own
    NaN-filled buffer (4-byte but not 16-byte aligned), each buffer with another
    row stride: the first a multiple of 4, the second odd, the rest the next
    free ones.  ``pads_intact`` checks that no padding element was written."""

    def __init__(self, dev, strided):
        self.dev, self.strided, self.bufs, self.used = dev, strided, [], set()

    def _stride(self, cols):
        k, s = len(self.bufs), cols + 2
        while s in self.used or (k == 0 and s % 4) or (k == 1 and s % 2 == 0):
            s += 1
        self.used.add(s)
        return s

    def out(self, rows, cols, stride=None):
        if not self.strided:
            return torch.full((rows, cols), NAN, device=self.dev)
        buf = torch.full((rows, stride or self._stride(cols)), NAN, device=self.dev)
        self.bufs.append((buf, cols))
        return buf[:, 1:1 + cols]

    def inp(self, t, stride=None):
        v = self.out(t.shape[0], t.shape[1], stride)
        v.copy_(t)
        return v

    def pair(self, a, b):
        """Two operands that the entry point addresses with one row stride (s and
        t, g_s and g_t): CPU tensors to upload, or shapes of outputs."""
        va = self.inp(a) if torch.is_tensor(a) else self.out(*a)
        st = va.stride(0) if self.strided else None
        return va, (self.inp(b, st) if torch.is_tensor(b) else self.out(*b, st))

    def pads_intact(self):
        for buf, cols in self.bufs:
            assert bool(torch.isnan(buf[:, :1]).all()) and bool(torch.isnan(buf[:, 1 + cols:]).all()), \
                "a padding element of a [%d, %d] view (stride %d) was written" % (buf.shape[0], cols, buf.stride(0))
        if self.strided:
            strides = [b.stride(0) for b, _ in self.bufs]
            assert any(s % 4 == 0 for s in strides) and any(s % 2 for s in strides), strides


# ---------------------------------------------------------------------------- references
def ref_affine(x, s, t, inverse=False):
    """nf/flows.py:56,59: out = t + in * exp(s), log|det| = sum(s);
    :69,72 (inverse): out = (in - t) * exp(-s), log|det| = -sum(s)."""
    if inverse:
        return (x - t) * torch.exp(-s), -torch.sum(s, dim=1)
    return t + x * torch.exp(s), torch.sum(s, dim=1)


def ref_planar(x, w, u, b, nl="tanh"):
    return orc.planar(x, {"w": w, "u": u, "b": b}, "", nl)


def ref_radial(x, x0, la, be):
    return orc.radial(x, {"x0": x0, "log_alpha": la, "beta": be}, "")


def ref_actnorm(x, mu, ls, inverse=False):
    return orc.actnorm(x, {"mu": mu, "log_sigma": ls}, "", inverse)


def ref_maf(x, init, prm, c0=0, c1=0, inverse=False):
    """nf/flows_1.py:180-188 / :194-201 for the columns [c0, c1) with given
    (mu, alpha): column 0 takes ``init``, column i >= 1 takes
    prm[:, 2 (i - max(c0, 1)) + {0, 1}].  Returns the written columns stacked in
    the order of i (forward: out column dim-1-i; inverse: out column i)."""
    B, p0 = x.shape[0], max(c0, 1)
    npar = max(c1 - p0, 0)
    mu, al = prm[:, 0:2 * npar:2], prm[:, 1:2 * npar:2]  # columns p0 .. c1-1
    if c0 == 0 and c1 > 0:
        mu = torch.cat((init[0].expand(B, 1), mu), dim=1)
        al = torch.cat((init[1].expand(B, 1), al), dim=1)
    if inverse:  # x[:, i] = mu + exp(alpha) * z.flip(1)[:, i];  log_det += alpha
        return mu + torch.exp(al) * x.flip(dims=(1,))[:, c0:c1], al.sum(dim=1)
    return (x[:, c0:c1] - mu) / torch.exp(al), -al.sum(dim=1)  # z[:, i];  log_det -= alpha


def maf_out_cols(dim, c0, c1, inverse):
    """Output (and, mirrored, input) column of each i in [c0, c1)."""
    return [i if inverse else dim - 1 - i for i in range(c0, c1)]


def ref_trig(x, bnd=3.0):
    """nf/flows.py:172-173: cat(cos(pi x / B), sin(pi x / B))."""
    a = torch.tensor(math.pi, dtype=x.dtype) * x / bnd
    return torch.cat((torch.cos(a), torch.sin(a)), dim=-1), None


def ref_normal(z, var, logdet=None, sign=1):
    """orc.normal_log_prob (torch's MultivariateNormal) -/+ logdet; at 16,384
    columns, where a dense covariance does not fit, its closed form."""
    d = z.shape[1]
    if d <= 1000:
        lp = orc.normal_log_prob(z, var)
    else:
        lp = -0.5 * (d * math.log(2 * math.pi) + (z * z).sum(1) / var) - 0.5 * d * math.log(var)
    if logdet is not None:
        lp = lp + logdet.to(z.dtype) if sign >= 0 else lp - logdet.to(z.dtype)
    return lp


def run_ref(fn, inputs, wrt, gz, gld, dtype, **kw):
    """fn(**inputs as dtype, **kw) -> (z, ld); autograd of (z * gz).sum() + (ld * gld).sum()
    w.r.t. the inputs named in ``wrt`` (a null cotangent drops its term).
    Returns (z, ld, {name: grad})."""
    leaves = {k: v.to(dtype).clone().requires_grad_(k in wrt) for k, v in inputs.items()}
    z, ld = fn(**leaves, **kw)
    grads = {k: torch.zeros_like(leaves[k]) for k in wrt}
    terms = []
    if gz is not None:
        terms.append((z * gz.to(dtype)).sum())
    if gld is not None and ld is not None:
        terms.append((ld * gld.to(dtype)).sum())
    if wrt and terms and sum(terms).requires_grad:  # an empty column range has no gradient
        gs = torch.autograd.grad(sum(terms), [leaves[k] for k in wrt], allow_unused=True)
        grads = {k: (g if g is not None else torch.zeros_like(leaves[k])) for k, g in zip(wrt, gs)}
    return z.detach(), (None if ld is None else ld.detach()), grads


def both_refs(fn, inputs, wrt=(), gz=None, gld=None, **kw):
    return run_ref(fn, inputs, list(wrt), gz, gld, torch.float64, **kw), \
        run_ref(fn, inputs, list(wrt), gz, gld, torch.float32, **kw)


# ---------------------------------------------------------------------------- comparison
FALLBACKS = []  # (what, max err ours, max err fp32 reference): the cases that needed the fallback


def _case():
    return os.environ.get("PYTEST_CURRENT_TEST", "").split(" ")[0].split("::")[-1]


def _cpu64(t):
    return t.detach().cpu().double()


def check_rows(what, ours, r64, r32, rtol, atol):
    """Every element against fp64 at rtol / atol.  Only where the fp32 CPU
    reference itself misses that does the case fall back to test_gpu_parity's
    on-par rule (close_or_on_par's factor 2: our max and p99 error against fp64
    within twice the fp32 reference's own)."""
    o, t, r = _cpu64(ours), _cpu64(r64), _cpu64(r32)
    assert o.shape == t.shape, (what, o.shape, t.shape)
    if o.numel() == 0:
        return
    if bool(((r - t).abs() <= atol + rtol * t.abs()).all()):
        torch.testing.assert_close(o, t, rtol=rtol, atol=atol, msg=lambda m: "%s: %s" % (what, m))
        return
    eo, er = float((o - t).abs().max()), float((r - t).abs().max())
    print("FALLBACK %s %s: the fp32 reference misses rtol %g atol %g; max err vs fp64 ours %.3g, fp32 reference %.3g"
          % (_case(), what, rtol, atol, eo, er))
    FALLBACKS.append((what, eo, er))
    assert bool(torch.isfinite(o).all()), what
    on_par(o.flatten(), r.flatten(), t.flatten(), rtol, atol, within=0.0, factor=2.0)


def check_sums(what, ours, r64, r32):
    """Batch-summed parameter gradients: rel_close at GRAD_TOL (error over the
    tensor's maximum), same fallback rule."""
    o, t, r = _cpu64(ours).reshape(-1), _cpu64(r64).reshape(-1), _cpu64(r32).reshape(-1)
    assert o.shape == t.shape, (what, o.shape, t.shape)
    assert bool(torch.isfinite(o).all()), what
    scale = max(float(t.abs().max()), 1e-12)
    if float((r - t).abs().max()) / scale <= GRAD_TOL:
        rel_close(o, t, what=what)
        return
    eo, er = float((o - t).abs().max()), float((r - t).abs().max())
    print("FALLBACK %s %s: the fp32 reference misses rel %g; max err vs fp64 ours %.3g, fp32 reference %.3g"
          % (_case(), what, GRAD_TOL, eo, er))
    FALLBACKS.append((what, eo, er))
    on_par(o, r, t, GRAD_TOL, GRAD_TOL * scale, within=0.0, factor=2.0)


def ld_operand(mode, batch, dev, seed=99):
    """(device logdet operand or None, its start values on the CPU) of a
    logdet_mode: NONE passes none, WRITE a NaN-filled one, ACC random values."""
    if mode == 0:
        return None, None
    start = rnd(seed, batch) if mode == 2 else torch.full((batch,), NAN)
    return start.to(dev), (start if mode == 2 else torch.zeros(batch))


def planar_params(dim, seed, nl, negative_s=False, bias=None):
    """w, u ~ U(+-1/sqrt(dim)) as Planar.reset_parameters draws them; with
    ``negative_s``, u is shifted along w so that w.u = -3 (u_hat = u off tanh)."""
    bound = 1.0 / math.sqrt(dim)
    w, u, b = uni(seed, dim, bound), uni(seed + 1, dim, bound), uni(seed + 2, 1, bound)
    if negative_s:
        assert nl != "tanh"
        wd, ud = w.double(), u.double()
        u = (ud - (wd @ ud + 3.0) * wd / (wd @ wd)).float()
    if bias is not None:
        b = torch.tensor([float(bias)])
    return w, u, b


def planar_s(x, w, u, b, nl):
    """fp64 s = 1 + h'(lin) w.u_hat of every row (u_hat = u off tanh)."""
    lin = x.double() @ w.double() + b.double()
    return 1.0 + orc._PLANAR_DERIV[nl](lin) * (w.double() @ u.double())


def planar_negative_s_inputs(batch, dim, nl, seed):
    """Inputs with rows of both signs of s: w.u = -3, bias -0.6 (so that some
    rows have lin < -ln 3, where elu's s turns positive, and some lin > 0,
    where leaky_relu's turns negative); any row with fp64 |s| < 0.1 is redrawn."""
    w, u, b = planar_params(dim, seed, nl, negative_s=True, bias=-0.6)
    x = rnd(seed + 3, batch, dim)
    for k in range(100):
        bad = planar_s(x, w, u, b, nl).abs() < 0.1
        if not bool(bad.any()):
            break
        x[bad] = rnd(seed + 10 + k, int(bad.sum()), dim)
    s = planar_s(x, w, u, b, nl)
    assert bool((s.abs() >= 0.1).all())
    assert bool((s < 0).any()) and bool((s > 0).any()), "the batch needs rows of both signs of s"
    return x, w, u, b
