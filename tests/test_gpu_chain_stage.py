"""GPU checks of the two-tile chain's weight staging (k_nsf_chain2 in
nfk_fused_chain2.hip: the copy of every next sub-record is a compile-time
function of the wave number; SubCopy there).

The instance is fixed at K = 8 and a hidden width of three 32-blocks plus a
1-4 feature tail, so the cases vary what the staging depends on:

* the chunk count and partial chunks (n_up = 16: one chunk, 32: two, 24 and
  20: a partial second chunk; n_lo = 10 and 12: a partial layer-1 k-block);
* the hidden width: 100 (a full 4-feature tail) and 97 (one feature);
* 1, 2 and 3 layers: no next-layer copy, the last-layer case after one
  next-layer copy, a middle layer with both;
* 1, 31 and 129 rows: part of one tile, a full and a partial tile of one wave,
  two workgroups of which the second holds one row.

Each case: forward, log_prob and inverse through the chain equal one launch
per layer bitwise (log_prob at test_gpu_chain.py's ulp-level tolerance: the
prior's row sum runs in another order) and the CPU oracle at that file's
tolerances.  Which path ran is asserted with the kernel timer and the
library's record of the chain form.  A run of one layer is never grouped by
the model, so the one-layer cases launch the chain directly.

size 10, dim 3 has rows of 30 floats, which are not 16-byte aligned: the
model runs it per layer whatever config.USE_CHAIN says (asserted), so that
case checks the fallback; size 12, dim 3 (n_lo = 12, n_up = 24, 36 columns) is
the same staging shape on the chain.

The training form (FusedArgs::saves) is one template with the inference form;
its case compares the gradients of a 2-layer, 129-row train step with the
per-layer path at test_gpu_grad.py's tolerance.
"""
import pytest
import torch

import nf.flows as nff
import nf.models as nfm
from normalizingflow_amd import _lib, config
from normalizingflow_amd import kernels as K_
from oracle import nf_oracle as orc

pytestmark = pytest.mark.gpu

KBINS = 8
ROWS = (1, 31, 129)
GRAD_TOL = 1e-4  # tests/test_gpu_grad.py

# (size, dim, masks)
SHAPES = [
    (16, 2, [[0], [1]]),   # n_up 16: one chunk
    (32, 2, [[0], [1]]),   # n_up 32: two chunks
    (24, 2, [[0], [1]]),   # n_up 24: a partial chunk
    (10, 3, [[1], [0]]),   # n_lo 10, n_up 20 (30 columns: the per-layer fallback)
    (12, 3, [[1], [0]]),   # n_lo 12, n_up 24 on the chain
]


def _model(n_layers, size, dim, hidden, masks, dev):
    torch.manual_seed(1234)
    flows = [nff.NSF_CL(size=size, dim=dim, K=KBINS, B=3, hidden_dim=hidden, mask=masks[i % len(masks)])
             for i in range(n_layers)]
    D = size * dim
    prior = torch.distributions.MultivariateNormal(torch.zeros(D), torch.eye(D))
    model = nfm.NormalizingFlowModel(prior, flows)
    sd = {k: v.detach().clone() for k, v in model.state_dict().items()}
    model = model.to(dev)
    model.prior = torch.distributions.MultivariateNormal(torch.zeros(D, device=dev), torch.eye(D, device=dev))
    return model, sd


def _with_chain(on, fn):
    prev = config.USE_CHAIN
    config.USE_CHAIN = on
    try:
        return fn()
    finally:
        config.USE_CHAIN = prev


def _counted(fn):
    """fn() under a kernel timer -> (result, {kernel: launches})."""
    prev = K_.TIMER
    K_.TIMER = K_.KernelTimer()
    try:
        out = fn()
        torch.cuda.synchronize()
        return out, {k: v[0] for k, v in K_.TIMER.summary().items()}
    finally:
        K_.TIMER = prev


def _chain_direct(model, x, inverse):
    """One chain launch over all of the model's layers (also a run of one)."""
    run = list(model.flows)[::-1] if inverse else list(model.flows)
    shape = run[0]._chain_shape(x.device)
    logdet = torch.zeros(x.shape[0], device=x.device)
    status = torch.zeros(len(run), dtype=torch.int32, device=x.device)
    z = model._run_chain(run, shape, x, inverse, logdet, status)
    return z, logdet


def _chain_log_prob_direct(model, x):
    run = list(model.flows)
    n_lo, n_up, hidden, K, B = run[0]._chain_shape(x.device)
    wp, cm = model._chain_args(run, n_lo + n_up, False, x)
    iso = model._prior_consts()
    out = torch.empty(x.shape[0], device=x.device)
    status = torch.zeros(len(run), dtype=torch.int32, device=x.device)
    K_.fused_nsf_chain(x, wp, cm, len(run), n_lo, n_up, hidden, None, logdet=None, logdet_mode=K_.MODE_NONE,
                       K=K, tail_bound=B, inverse=False, status=status, log_prob=out, prior_scale=iso[0],
                       prior_hld=iso[1])
    return out


def _chain_results(model, x, n_layers, on_chain):
    """(z, prior lp, logdet, log_prob, x inverse, logdet inverse) through the
    chain, with the path asserted."""
    lib = _lib.load()
    if n_layers == 1 and on_chain:
        (z, ld), c1 = _counted(lambda: _chain_direct(model, x, False))
        lp, c2 = _counted(lambda: _chain_log_prob_direct(model, x))
        (xi, ldi), c3 = _counted(lambda: _chain_direct(model, x, True))
        plp = model._prior_log_prob(z)
    else:
        (z, plp, ld), c1 = _counted(lambda: _with_chain(True, lambda: model(x)))
        lp, c2 = _counted(lambda: _with_chain(True, lambda: model.log_prob(x)))
        (xi, ldi), c3 = _counted(lambda: _with_chain(True, lambda: model.inverse(x)))
    if on_chain:  # one chain launch each, no per-layer launch
        for c in (c1, c2, c3):
            assert c.get("nfk_fused_nsf_chain") == 1 and "nfk_fused_nsf" not in c, (c1, c2, c3)
        assert lib.nfk_debug_last_chain_form() == 1  # the two-tile kernel, not the one-tile chain
    else:
        assert all("nfk_fused_nsf_chain" not in c for c in (c1, c2, c3)), (c1, c2, c3)
    return z, plp, ld, lp, xi, ldi


@pytest.mark.parametrize("n_layers", [1, 2, 3])
@pytest.mark.parametrize("hidden", [100, 97])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "s%d_d%d" % s[:2])
def test_chain_stage_bitwise_vs_per_layer_and_oracle(shape, hidden, n_layers, hip_device):
    size, dim, masks = shape
    D = size * dim
    model, sd = _model(n_layers, size, dim, hidden, masks, hip_device)
    on_chain = D % 4 == 0
    if on_chain:
        assert K_.fused_nsf_chain_max(len(masks[0]) * size, D - len(masks[0]) * size, hidden, KBINS) >= n_layers
    xall = torch.randn(max(ROWS), D, generator=torch.Generator().manual_seed(5)) * 1.3
    specs = orc.nsf_cl_specs(n_layers, size, dim, KBINS, 3, masks)
    ref_lp = orc.model_log_prob(specs, sd, xall)  # rows are independent: one reference, sliced
    ref_xi, ref_ldi = orc.model_inverse(specs, sd, xall)
    for rows in ROWS:
        xd = xall[:rows].to(hip_device)
        with torch.no_grad():
            zc, plc, ldc, lpc, xic, ldic = _chain_results(model, xd, n_layers, on_chain)
            zs, pls, lds = _with_chain(False, lambda: model(xd))
            lps = _with_chain(False, lambda: model.log_prob(xd))
            xis, ldis = _with_chain(False, lambda: model.inverse(xd))
        for a, b, what in ((zc, zs, "z"), (plc, pls, "prior lp"), (ldc, lds, "logdet"), (xic, xis, "inverse x"),
                           (ldic, ldis, "inverse logdet")):
            assert torch.equal(a, b), (what, rows)
        torch.testing.assert_close(lpc, lps, rtol=2e-7, atol=2e-5)
        torch.testing.assert_close(lpc, plc + ldc, rtol=2e-7, atol=2e-5)
        torch.testing.assert_close(lpc.cpu(), ref_lp[:rows], rtol=1e-5, atol=1e-4)
        torch.testing.assert_close(xic.cpu(), ref_xi[:rows], rtol=1e-5, atol=1e-4)
        torch.testing.assert_close(ldic.cpu(), ref_ldi[:rows], rtol=1e-5, atol=3e-4)


def _rel_close(a, b, what):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    assert a.shape == b.shape, (what, a.shape, b.shape)
    err = float((a - b).abs().max()) / max(float(b.abs().max()), 1e-12)
    assert err <= GRAD_TOL, "%s: rel err %.3g" % (what, err)


def test_chain_stage_training_form_grads(hip_device, monkeypatch):
    """The saves form at 129 rows (two workgroups, the second with one row) and
    2 layers: one nfk_fused_nsf_chain_saved launch; z and log|det| bitwise and
    every gradient within test_gpu_grad.py's tolerance of the per-layer path."""
    model, _ = _model(2, 32, 2, 100, [[0], [1]], hip_device)
    x = (torch.randn(129, 64, generator=torch.Generator().manual_seed(129)) * 1.2).to(hip_device)
    calls = []
    real = K_.fused_nsf_chain_saved

    def counted(*a, **k):
        calls.append(a[4])  # nlayers
        return real(*a, **k)

    monkeypatch.setattr(K_, "fused_nsf_chain_saved", counted)

    def step(chain):
        monkeypatch.setattr(config, "USE_TRAIN_CHAIN", chain)
        model.zero_grad(set_to_none=True)
        xg = x.clone().requires_grad_(True)
        z, plp, ld = model(xg)
        (-torch.mean(plp + ld)).backward()
        return z.detach(), ld.detach(), xg.grad.clone(), {k: p.grad.clone() for k, p in model.named_parameters()}

    zc, ldc, gxc, gc = step(True)
    assert calls == [2]
    zs, lds, gxs, gs = step(False)
    assert calls == [2]
    assert torch.equal(zc, zs) and torch.equal(ldc, lds)
    _rel_close(gxc, gxs, "x.grad")
    for k in gc:
        _rel_close(gc[k], gs[k], k)
