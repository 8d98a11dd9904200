"""GPU: the float knots of the fused NSF epilogue (knot_phase in
nfk_fused_impl.h: sequential partial sums of the second softmax, float
compares for the bin, knots in the normalised range [0, 1]) where they can go
wrong -- inputs on and around every knot and both tail bounds, saturated
softmaxes (bins at the minimum width), every K the kernel takes, and a NaN
conditioner input.  One NSF_CL layer (size 16, dim 2, hidden 100) through the
fused kernel, against the CPU oracle (nf/flows.py:216-253, nf/utils.py:27-152).

Tolerances as tests/test_gpu_fused_forms.py: z rtol 1e-5 / atol 5e-5;
log|det| rtol 1e-5 / atol 3e-4.  Every element is checked.
"""
import pytest
import torch

import nf.flows as nff
from normalizingflow_amd import kernels as K_
from oracle import nf_oracle as orc

pytestmark = pytest.mark.gpu

Z_RTOL, Z_ATOL = 1e-5, 5e-5
LD_RTOL, LD_ATOL = 1e-5, 3e-4
SIZE, DIM, HIDDEN, B, MASK = 16, 2, 100, 3, [0]


def make_layer(K=8, out_scale=1.0, seed=20, hidden=HIDDEN):
    torch.manual_seed(seed)
    layer = nff.NSF_CL(size=SIZE, dim=DIM, K=K, B=B, hidden_dim=hidden, mask=MASK)
    if out_scale != 1.0:
        with torch.no_grad():
            layer.psi.network[4].weight.mul_(out_scale)
            layer.psi.network[4].bias.mul_(out_scale)
    return layer, {k: v.detach().clone() for k, v in layer.state_dict().items()}


def oracle(x, sd, K, inverse=False, f64=False):
    """(z, log|det|) of the oracle in fp32, or in fp64 on the same fp32 inputs and weights."""
    if not f64:
        return orc.nsf_cl(x, sd, "", SIZE, DIM, K, B, MASK, inverse=inverse)
    prev = torch.get_default_dtype()
    torch.set_default_dtype(torch.float64)
    try:
        return orc.nsf_cl(x.double(), {k: v.double() for k, v in sd.items()}, "", SIZE, DIM, K, B, MASK,
                          inverse=inverse)
    finally:
        torch.set_default_dtype(prev)


def device_run(layer, x, inverse=False):
    with torch.no_grad():
        z, ld = layer.inverse(x) if inverse else layer(x)
    assert layer._pack_cache is not None  # the fused kernel ran
    return z.cpu(), ld.cpu()


def nudge(t, ulps):
    """t moved by `ulps` fp32 steps (towards +inf for ulps > 0)."""
    to = torch.full_like(t, float("inf") if ulps > 0 else float("-inf"))
    for _ in range(abs(ulps)):
        t = torch.nextafter(t, to)
    return t


def edge_inputs(sd, K=8, rows=64):
    """For `rows` conditioner inputs: every transformed coordinate on each of the
    oracle's fp32 interior width knots and 1 and 2 ulps either side of it, on
    -B and B exactly and one ulp inside and outside (one variant per row copy)."""
    base = torch.randn(rows, SIZE * DIM, generator=torch.Generator().manual_seed(31)) * 1.3
    g = base.reshape(rows, SIZE, DIM)
    lo = g[:, :, MASK].flatten(start_dim=1)
    n_up = SIZE * (DIM - len(MASK))
    raw = orc.fcnn(lo, sd, "psi.").reshape(rows, n_up, 3 * K - 1)
    cw, _ = orc._knots(2 * B * torch.softmax(raw[..., :K], dim=2), -float(B), float(B), orc.MIN_BIN_WIDTH)
    variants = [nudge(cw[..., j], d) for j in range(1, K) for d in (-2, -1, 0, 1, 2)]
    variants += [nudge(torch.full((rows, n_up), float(v)), d) for v in (-B, B) for d in (-1, 0, 1)]
    rest = [c for c in range(DIM) if c not in MASK]
    xs = []
    for v in variants:
        gv = g.clone()
        gv[:, :, rest] = v.reshape(rows, SIZE, len(rest))
        xs.append(gv.reshape(rows, SIZE * DIM))
    return torch.cat(xs, dim=0)


def saturated_inputs():
    return torch.randn(512, SIZE * DIM, generator=torch.Generator().manual_seed(32)) * 1.3


def err_stats(a, truth):
    e = (a.double() - truth).abs().flatten()
    return e.max().item(), torch.quantile(e, 0.99).item()


def assert_on_par(ours, ref32, truth, what, factor=2.0):
    """our max and p99 error against the fp64 truth within `factor` x the fp32
    oracle's own (tests/test_gpu_parity.py on_par / test_c3_error_vs_fp64)"""
    (mo, qo), (mr, qr) = err_stats(ours, truth), err_stats(ref32, truth)
    print("%s vs fp64: max ours %.3g ref %.3g; p99 ours %.3g ref %.3g" % (what, mo, mr, qo, qr))
    assert mo <= factor * mr + 1e-6, (what, mo, mr)
    assert qo <= factor * qr + 1e-6, (what, qo, qr)


def test_inputs_on_the_knots(hip_device):
    layer, sd = make_layer()
    x = edge_inputs(sd)
    assert x.shape[0] == 64 * (7 * 5 + 6)
    z64, ld64 = oracle(x, sd, 8, f64=True)
    dev = layer.to(hip_device)
    z, ld = device_run(dev, x.to(hip_device))
    print("on the knots: max |dz| %.3g, max |dld| %.3g"
          % ((z.double() - z64).abs().max(), (ld.double() - ld64).abs().max()))
    torch.testing.assert_close(z.double(), z64, rtol=Z_RTOL, atol=Z_ATOL)
    torch.testing.assert_close(ld.double(), ld64, rtol=LD_RTOL, atol=LD_ATOL)
    # forward then inverse: z sits on and around the height knots
    xr, ldr = device_run(dev, z.to(hip_device), inverse=True)
    print("round trip: max |dx| %.3g, max |ld + ld_inv| %.3g" % ((xr - x).abs().max(), (ldr + ld).abs().max()))
    torch.testing.assert_close(xr, x, rtol=Z_RTOL, atol=Z_ATOL)
    xi64, ldi64 = oracle(z, sd, 8, inverse=True, f64=True)
    torch.testing.assert_close(xr.double(), xi64, rtol=Z_RTOL, atol=Z_ATOL)
    torch.testing.assert_close(ldr.double(), ldi64, rtol=LD_RTOL, atol=LD_ATOL)


@pytest.mark.parametrize("inverse", [False, True])
def test_saturated_softmaxes(inverse, hip_device):
    """Output weights x30: the first softmax saturates and most bins collapse
    towards the minimum width (narrowest 0.02 of the range 6, 38 % under 0.03).
    The fp32 oracle itself misses the direct tolerances on these inputs (fp32 vs
    fp64 oracle on the CPU: z max 5.7e-4 forward / 8.5e-4 inverse, 8 of 16,384
    elements over; log|det| max 2.5e-3 / 4.3e-3, 1 / 7 of 512 rows over): a knot's
    ulp is amplified by the slope of such a bin for the reference as for us, so
    the criterion is the fp64-error rule of tests/test_gpu_parity.py, at 2x."""
    layer, sd = make_layer(out_scale=30.0)
    x = saturated_inputs()
    z32, ld32 = oracle(x, sd, 8, inverse=inverse)
    z64, ld64 = oracle(x, sd, 8, inverse=inverse, f64=True)
    z, ld = device_run(layer.to(hip_device), x.to(hip_device), inverse=inverse)
    assert bool(torch.isfinite(z).all()) and bool(torch.isfinite(ld).all())
    assert_on_par(z, z32, z64, "saturated z")
    assert_on_par(ld, ld32, ld64, "saturated log|det|")


def test_every_bin_count(hip_device):
    """K = 2 .. 16 at c3's hidden width 100 (with the f32 tail step) and at 128
    (without): a (K, hidden) runs wherever fused_nsf_supported takes it.  The
    16-coordinate kernel is instantiated for K = 4, 5, 6, 8, 10 (so K = 2, 3 run
    nowhere); K = 16 is the wide kernel's, at hidden 128 only."""
    ran = set()
    n_lo, n_up = len(MASK) * SIZE, (DIM - len(MASK)) * SIZE
    for K in (2, 3, 5, 8, 10, 16):
        for hidden in (100, 128):
            if not K_.fused_nsf_supported(n_lo, n_up, hidden, K):
                continue
            layer, sd = make_layer(K=K, seed=40 + K, hidden=hidden)
            x = torch.randn(300, SIZE * DIM, generator=torch.Generator().manual_seed(50 + K)) * 1.3
            dev = layer.to(hip_device)
            for inverse in (False, True):
                z_ref, ld_ref = oracle(x, sd, K, inverse=inverse)
                z, ld = device_run(dev, x.to(hip_device), inverse=inverse)
                tag = "K %d hidden %d inverse %s: " % (K, hidden, inverse)
                torch.testing.assert_close(z, z_ref, rtol=Z_RTOL, atol=Z_ATOL, msg=lambda m: tag + m)
                torch.testing.assert_close(ld, ld_ref, rtol=LD_RTOL, atol=LD_ATOL, msg=lambda m: tag + m)
            ran.add(K)
    assert 8 in ran and len(ran) >= 4, sorted(ran)


def test_nan_row_stays_in_its_row(hip_device):
    layer, _ = make_layer()
    x = torch.randn(129, SIZE * DIM, generator=torch.Generator().manual_seed(33)) * 1.3
    row = 77
    x[row].clamp_(-2.9, 2.9)  # every transformed coordinate inside the tails
    x[row, 5 * DIM + MASK[0]] = float("nan")  # conditioner input of particle 5
    dev = layer.to(hip_device)
    z, ld = device_run(dev, x.to(hip_device))
    g = z.reshape(129, SIZE, DIM)
    # the NaN cumsum makes every transformed coordinate of the row and its
    # log|det| NaN (utils.py:73-91); the conditioner inputs pass through
    assert bool(torch.isnan(g[row, :, len(MASK):]).all()) and bool(torch.isnan(ld[row]))
    x_lo = x.reshape(129, SIZE, DIM)[row][:, MASK]
    assert torch.equal(torch.nan_to_num(g[row, :, :len(MASK)], nan=7.0), torch.nan_to_num(x_lo, nan=7.0))
    keep = [i for i in range(129) if i != row]
    z0, ld0 = device_run(dev, x[keep].to(hip_device))
    assert bool(torch.isfinite(z0).all()) and bool(torch.isfinite(ld0).all())
    assert torch.equal(z[keep], z0) and torch.equal(ld[keep], ld0)
