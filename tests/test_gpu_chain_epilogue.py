"""GPU: the spline epilogues of the two-tile chain (k_nsf_chain2 in
nfk_fused_chain2.hip) at the places where their bookkeeping can go wrong:

* the unclamped table lookups (rows k and k + 1 of a K-row table: the row past
  the table is other LDS of the workgroup, thrown away by a select) -- so the
  inputs hit bin 0, bin K - 1 and the tails in every layer, and the same call
  is repeated after another kernel has filled the LDS with something else;
* the bisection bin search (three compares at K = 8), NaN inputs and NaN knots
  included: a row with a NaN in a coordinate that layer 1 transforms and
  layer 2 conditions on;
* the FULL instances (n_up a multiple of 16: plain reads, no padding column) at
  one and at two chunk-loop trips, and the general instance with a partial
  second chunk; a second tile and a second workgroup that hold a single row.

Checks: (a) z, log|det| and log_prob as int32 bit patterns against one launch
per layer (config.USE_CHAIN off), the NaN row included; (b) the CPU oracle at
the tolerances of tests/test_gpu_parity.py's c3 tests; (c) the call repeated
after a RealNVP chain launch, bit for bit.
"""
import pytest
import torch

import nf.flows as nff
import nf.models as nfm
from normalizingflow_amd import _lib, config
from oracle import nf_oracle as orc

pytestmark = pytest.mark.gpu

KBINS, HIDDEN, B, DIM = 8, 100, 3.0, 2
MASKS = [[0], [1]]
SIZES = [16, 32, 24]   # FULL one trip; FULL two trips (c3's shape); general, n_up = 24
BATCHES = [33, 129]    # a second tile with one row; a second workgroup with one row
NAN_ROW, NAN_COL = 5, 1  # coordinate 1 of particle 0: upper in layer 1, lower in layer 2

# tests/test_gpu_parity.py, c3: log_prob, z (forward), log|det|, x (inverse)
LP_TOL = dict(rtol=1e-5, atol=1e-5)
Z_TOL = dict(rtol=1e-5, atol=5e-5)
LD_TOL = dict(rtol=1e-5, atol=2e-4)
XI_TOL = dict(rtol=1e-5, atol=1e-4)


def _model(size):
    torch.manual_seed(1234)
    flows = [nff.NSF_CL(size=size, dim=DIM, K=KBINS, B=B, hidden_dim=HIDDEN, mask=MASKS[i]) for i in range(2)]
    D = size * DIM
    model = nfm.NormalizingFlowModel(torch.distributions.MultivariateNormal(torch.zeros(D), torch.eye(D)), flows)
    sd = {k: v.detach().clone() for k, v in model.state_dict().items()}
    return model, sd


def _to_dev(model, dev):
    D = model.prior.loc.shape[0]
    model = model.to(dev)
    model.prior = torch.distributions.MultivariateNormal(torch.zeros(D, device=dev), torch.eye(D, device=dev))
    return model


def _inputs(batch, D):
    """batch - 1 rows whose every column is a shuffled grid over [-B - 0.5,
    B + 0.5] holding exactly -B and B, and one row (NAN_ROW) with a NaN."""
    g = torch.Generator().manual_seed(batch * 1000 + D)
    n = batch - 1
    grid = torch.cat([torch.tensor([-B, B]), torch.linspace(-B - 0.5, B + 0.5, n - 2)])
    cols = [grid[torch.randperm(n, generator=g)] for _ in range(D)]
    clean = torch.stack(cols, dim=1)
    nan_row = torch.randn(1, D, generator=g)
    nan_row[0, NAN_COL] = float("nan")
    x = torch.cat([clean[:NAN_ROW], nan_row, clean[NAN_ROW:]])
    keep = torch.arange(batch) != NAN_ROW
    return x, keep


def _oracle_bins(sd, size, x, inverse):
    """Per layer in execution order: (bin index, inside) of every transformed
    element, from the oracle's own knots and search."""
    out = []
    order = [1, 0] if inverse else [0, 1]
    for i in order:
        prefix, mask = "flows.%d." % i, MASKS[i]
        rest = [c for c in range(DIM) if c not in mask]
        g = x.reshape(-1, size, DIM)
        lo, up = g[:, :, mask].flatten(start_dim=1), g[:, :, rest].flatten(start_dim=1)
        raw = orc.fcnn(lo, sd, prefix + "psi.").reshape(-1, len(rest) * size, 3 * KBINS - 1)
        uw, uh, _ = torch.split(raw, KBINS, dim=2)
        u = 2 * B * torch.softmax(uh if inverse else uw, dim=2)
        edges, _ = orc._knots(u, -B, B, orc.MIN_BIN_WIDTH)
        inside = (up >= -B) & (up <= B)
        k = orc._bin_of(edges, torch.where(inside, up, torch.zeros_like(up)))
        out.append((k, inside))
        x, _ = orc.nsf_cl(x, sd, prefix, size, DIM, KBINS, B, mask, inverse=inverse)
    return out


def _assert_inputs_reach_the_edges(sd, size, x):
    for inverse in (False, True):
        for k, inside in _oracle_bins(sd, size, x, inverse):
            assert bool((~inside).any()), "no element in the tails"
            assert bool((k[inside] == 0).any()), "bin 0 not hit"
            assert bool((k[inside] == KBINS - 1).any()), "bin K - 1 not hit"


def _run(model, xd, chain):
    """(z, log|det|, log_prob, x inverse, log|det| inverse); the data-dependent
    errors are off: the NaN row would raise them in both paths."""
    prev = config.USE_CHAIN, config.STRICT_CHECKS
    config.USE_CHAIN, config.STRICT_CHECKS = chain, False
    try:
        with torch.no_grad():
            z, _, ld = model(xd)
            if chain:
                assert _lib.load().nfk_debug_last_chain_form() == 1  # the two-tile kernel
            lp = model.log_prob(xd)
            xi, ldi = model.inverse(xd)
        torch.cuda.synchronize()
    finally:
        config.USE_CHAIN, config.STRICT_CHECKS = prev
    return z, ld, lp, xi, ldi


def _bits(t):
    return t.contiguous().view(torch.int32)


@pytest.fixture(scope="module")
def lds_filler(hip_device):
    """A launch of another LDS-heavy kernel: c2's RealNVP chain."""
    torch.manual_seed(7)
    flows = [nff.RealNVP(64, hidden_dim=100) for _ in range(8)]
    model = nfm.NormalizingFlowModel(torch.distributions.MultivariateNormal(torch.zeros(64), torch.eye(64)), flows)
    model = _to_dev(model, hip_device)
    x = torch.randn(4096, 64, generator=torch.Generator().manual_seed(3)).to(hip_device)

    def fill():
        with torch.no_grad():
            model.log_prob(x)
        torch.cuda.synchronize()
    return fill


_CACHE = {}


def _results(size, batch, dev, fill):
    """One evaluation per case, shared by the tests below: the oracle, the
    chain, the per-layer path, and the chain again after `fill`."""
    if (size, batch) in _CACHE:
        return _CACHE[size, batch]
    D = size * DIM
    model, sd = _model(size)
    x, keep = _inputs(batch, D)
    assert x.shape[0] == batch and bool(torch.isnan(x[NAN_ROW, NAN_COL]))
    _assert_inputs_reach_the_edges(sd, size, x[keep])
    specs = orc.nsf_cl_specs(2, size, DIM, KBINS, B, MASKS)
    z_ref, _, ld_ref = orc.model_forward(specs, sd, x[keep])
    lp_ref = orc.model_log_prob(specs, sd, x[keep])
    xi_ref, ldi_ref = orc.model_inverse(specs, sd, x[keep])
    model = _to_dev(model, dev)
    xd = x.to(dev)
    first = _run(model, xd, True)
    per_layer = _run(model, xd, False)
    fill()
    again = _run(model, xd, True)
    res = dict(keep=keep, first=first, per_layer=per_layer, again=again,
               ref=(z_ref, ld_ref, lp_ref, xi_ref, ldi_ref))
    _CACHE[size, batch] = res
    return res


NAMES = ("z", "logdet", "log_prob", "x_inverse", "logdet_inverse")
CASES = [(s, b) for s in SIZES for b in BATCHES]


@pytest.mark.parametrize("size,batch", CASES)
def test_chain_epilogue_bitwise_vs_per_layer(size, batch, hip_device, lds_filler):
    """(a) z and log|det| of both directions against one launch per layer, as
    bit patterns, the NaN row included."""
    r = _results(size, batch, hip_device, lds_filler)
    for name, a, b in zip(NAMES, r["first"], r["per_layer"]):
        if name != "log_prob":
            assert torch.equal(_bits(a), _bits(b)), name
    z, _, lp = r["first"][:3]
    assert bool(torch.isnan(z[NAN_ROW]).any()) and bool(torch.isnan(lp[NAN_ROW]))


@pytest.mark.parametrize("size,batch", CASES)
def test_chain_epilogue_log_prob_bitwise_vs_per_layer(size, batch, hip_device, lds_filler):
    """(a) log_prob against the per-layer path, as bit patterns, the NaN row
    included.  The per-layer path ends in nfk_normal_logprob, which at widths a
    chain can hold sums a row's squares in the order of the chains' prior
    epilogues (four lanes over the float4 groups q, q + 4, ..., then
    (m0 + m1) + (m2 + m3)); both write one canonical NaN.  Before that, 4 to 20
    of these 33 / 129 rows differed by one ulp (max |d| 3.05e-05), and the NaN
    row in its payload."""
    r = _results(size, batch, hip_device, lds_filler)
    a, b = r["first"][2], r["per_layer"][2]
    diff = _bits(a) != _bits(b)
    print("log_prob: %d of %d rows differ in bits, max |d| %.3g; NaN row %08x / %08x"
          % (int(diff.sum()), a.numel(), float((a - b)[~torch.isnan(a - b)].abs().max()),
             int(_bits(a)[NAN_ROW]) & 0xffffffff, int(_bits(b)[NAN_ROW]) & 0xffffffff))
    assert not bool(diff.any())


@pytest.mark.parametrize("size,batch", CASES)
def test_chain_epilogue_repeat_after_other_kernel(size, batch, hip_device, lds_filler):
    """(c) the same call after a RealNVP chain launch has rewritten the LDS:
    nothing from outside the tables reaches an output."""
    r = _results(size, batch, hip_device, lds_filler)
    for name, a, b in zip(NAMES, r["first"], r["again"]):
        assert torch.equal(_bits(a), _bits(b)), name


@pytest.mark.parametrize("size,batch", CASES)
def test_chain_epilogue_vs_oracle(size, batch, hip_device, lds_filler):
    """(b) the oracle, on the rows it can take (every row but the NaN one)."""
    r = _results(size, batch, hip_device, lds_filler)
    z, ld, lp, xi, ldi = (t.cpu()[r["keep"]] for t in r["first"])
    z_ref, ld_ref, lp_ref, xi_ref, ldi_ref = r["ref"]
    torch.testing.assert_close(lp, lp_ref, **LP_TOL)
    torch.testing.assert_close(z, z_ref, **Z_TOL)
    torch.testing.assert_close(ld, ld_ref, **LD_TOL)
    torch.testing.assert_close(xi, xi_ref, **XI_TOL)
    torch.testing.assert_close(ldi, ldi_ref, **LD_TOL)
