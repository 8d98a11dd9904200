"""GPU checks of normalizingflow_amd.systems (nfk_systems.hip): the Einstein
crystal, Gaussian mixture and Lennard-Jones kernels against the reference's
``sys_*`` golden vectors, as priors of NormalizingFlowModel (fused log|det|,
status word, autograd node, HIP graph) and under the application layer's
losses and Q matrix.

Parity follows tests/test_gpu_parity.py's close_or_on_par convention (restated
here): a case passes at rtol 1e-5 / atol 1e-4 against the reference's fp32
values, or when our max and p99 error against the fp64 companion is within 2x
the reference's own fp32 error.
"""
import pytest
import torch

import golden_io as gio
import nf.flows as nff
import nf.models as nfm
from normalizingflow_amd import app, systems
from normalizingflow_amd import kernels as K_
from normalizingflow_amd.graphs import GraphedLogProb, GraphedSample

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
RTOL, ATOL = 1e-5, 1e-4
GRAD_TOL = 1e-4  # tests/test_gpu_grad.py's tolerance for layer gradients
L32 = 2.92402    # LJ.yaml's box (rho 1.28, 32 particles)
NAMES = gio.names("sys_")
_CACHE = {}


def fixture(name):
    if name not in _CACHE:
        _CACHE[name] = gio.load(name)[:2]
    return _CACHE[name]


def close_or_on_par(ours, ref, truth, what, rtol=RTOL, atol=ATOL, factor=2.0):
    o, r, t = ours.detach().cpu().double(), ref.detach().cpu().double(), truth.double()
    try:
        torch.testing.assert_close(o, r, rtol=rtol, atol=atol)
        return
    except AssertionError:
        pass
    eo, er = (o - t).abs().flatten(), (r - t).abs().flatten()
    qo, qr = torch.quantile(eo, 0.99).item(), torch.quantile(er, 0.99).item()
    print("%s: on-par decides: max ours %.3g ref %.3g (ratio %.3g), p99 ours %.3g ref %.3g (ratio %.3g)"
          % (what, eo.max(), er.max(), eo.max() / max(er.max().item(), 1e-30), qo, qr, qo / max(qr, 1e-30)))
    assert eo.max().item() <= factor * er.max().item() + 1e-6, (what, eo.max().item(), er.max().item())
    assert qo <= factor * qr + 1e-6, (what, qo, qr)


def rel_close(a, b, tol=GRAD_TOL, what=""):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    assert a.shape == b.shape, (what, a.shape, b.shape)
    scale = max(float(b.abs().max()), 1e-12)
    err = float((a - b).abs().max()) / scale
    assert err <= tol, "%s: rel err %.3g" % (what, err)


def build(meta, data, device=DEV):
    if meta["kind"] == "einstein":
        obj = systems.EinsteinCrystal(data["centers"], meta["dim"], boxlength=meta["boxlength"],
                                      alpha=meta["alpha"], device=device)
        return obj, obj.log_prob
    if meta["kind"] == "gmix":
        obj = systems.GaussianMixture(meta["centers"], meta["vars"], meta["npart"], meta["dim"], device=device)
        return obj, obj.log_prob
    obj = systems.LJ(boxlength=meta["boxlength"], sigma=meta["sigma"], epsilon=meta["epsilon"],
                     cutoff=meta["cutoff"], shift=meta["shift"], device=device)
    return obj, obj.potential


def run(fn, x, w):
    xr = x.detach().clone().requires_grad_()
    out = fn(xr)
    g, = torch.autograd.grad((out * w).sum(), xr)
    return out.detach(), g


def counts_of(fn):
    prev = K_.TIMER
    K_.TIMER = K_.KernelTimer()
    try:
        fn()
        torch.cuda.synchronize()
        return {k: v[0] for k, v in K_.TIMER.summary().items()}
    finally:
        K_.TIMER = prev


def no_torch_path(obj, monkeypatch):
    def boom(*a, **k):
        raise AssertionError("the torch path ran")
    monkeypatch.setattr(obj, "_log_prob_torch" if hasattr(obj, "_log_prob_torch") else "_potential_torch", boom)


# ---------------------------------------------------------------- fixture parity
def _row_index(rows):
    if rows == 37:
        return torch.arange(37)
    if rows == 1:
        return torch.tensor([5])
    g = torch.Generator().manual_seed(rows)
    return (torch.arange(rows) % 37)[torch.randperm(rows, generator=g)]  # tiled, row order shuffled


@pytest.mark.parametrize("rows", [1, 37, 500])
@pytest.mark.parametrize("name", NAMES)
def test_fixture_parity(name, rows, hip_device, monkeypatch):
    meta, data = fixture(name)
    idx = _row_index(rows)
    obj, fn = build(meta, data)
    no_torch_path(obj, monkeypatch)
    x, w = data["x"][idx].to(DEV), data["w"][idx].to(DEV)
    out, grad = run(fn, x, w)
    assert out.shape == (rows,) and grad.shape == x.shape and out.dtype == torch.float32
    ref_o, ref_g = data["out"][idx], data["grad"][idx]
    tru_o, tru_g = data["out64"][idx], data["grad64"][idx]
    out, grad = out.cpu(), grad.cpu()
    if meta.get("far"):
        # the far particles: log(0) = -inf for the row, 0/0 = NaN for their gradient
        far = torch.isinf(ref_o)
        assert torch.equal(torch.isinf(out), far) and (out[far] < 0).all()
        assert torch.equal(torch.isnan(grad), torch.isnan(ref_g))
        keep = ~torch.isnan(ref_g)
        out, ref_o, tru_o = out[~far], ref_o[~far], tru_o[~far]
        grad, ref_g, tru_g = grad[keep], ref_g[keep], tru_g[keep]
    close_or_on_par(out, ref_o, tru_o, name + " out")
    close_or_on_par(grad, ref_g, tru_g, name + " grad")


LAYOUT_CASES = ["sys_einstein_32x3_box_a600", "sys_einstein_5x2_box_a600", "sys_gmix_yaml", "sys_lj_n32_cut_shift",
                "sys_lj_n100_cut_shift"]


@pytest.mark.parametrize("name", LAYOUT_CASES)
def test_strided_and_misaligned_inputs(name, hip_device):
    meta, data = fixture(name)
    obj, fn = build(meta, data)
    x2 = data["x"].reshape(37, -1).to(DEV)
    shape = data["x"].shape
    width = x2.shape[1]
    w = data["w"].to(DEV)
    out, grad = run(lambda t: fn(t.reshape(shape)), x2, w)
    # rows longer than the width (ldx > width)
    base = torch.zeros(37, width + 3, device=DEV)
    base[:, :width] = x2
    base.requires_grad_()
    xs = base[:, :width]
    assert xs.stride(0) == width + 3
    o1 = fn(xs if len(shape) == 2 else xs.unflatten(1, shape[1:]))
    g1 = torch.autograd.grad((o1 * w).sum(), base)[0][:, :width]
    # 4 bytes off 16-byte alignment
    flat = torch.zeros(37 * width + 1, device=DEV)
    flat[1:] = x2.flatten()
    flat.requires_grad_()
    xm = flat[1:].view(shape)
    assert xm.data_ptr() % 16 == 4
    o2 = fn(xm)
    g2 = torch.autograd.grad((o2 * w).sum(), flat)[0][1:].view(37, width)
    if meta["kind"] == "einstein" and width % 4 == 0:
        # the float4 form multiplies by 1/scale where the scalar form divides: <= 1 ulp per element
        for o, g in ((o1, g1), (o2, g2)):
            torch.testing.assert_close(o, out, rtol=2e-6, atol=2e-5)
            torch.testing.assert_close(g, grad, rtol=2e-6, atol=2e-5)
        assert torch.equal(o1, o2) and torch.equal(g1, g2)
    else:
        for o, g in ((o1, g1), (o2, g2)):
            assert torch.equal(o, out) and torch.equal(g, grad)


def test_lj_force_and_unsupported_sizes(hip_device):
    meta, data = fixture("sys_lj_n32_cut_shift")
    lj, _ = build(meta, data)
    x = data["x"].to(DEV)
    out, grad = run(lj.potential, x, torch.ones(37, device=DEV))
    assert torch.equal(lj.force(x), -grad)
    assert lj.potential(x[0]).shape == () and lj.potential(x.reshape(1, 37, 32, 3)).shape == (1, 37)
    # more particles than the kernels take: the row-chunked torch path on the device
    big = torch.rand(3, 300, 3, device=DEV) * 8.0
    lj8 = systems.LJ(boxlength=8.0, cutoff=1.6, device=DEV)
    assert not K_.lj_supported(300, 3) and K_.lj_supported(256, 3) and not K_.lj_supported(32, 4)
    torch.testing.assert_close(lj8.potential(big).cpu(), systems.LJ(boxlength=8.0, cutoff=1.6).potential(big.cpu()),
                               rtol=1e-4, atol=1e-3)
    with pytest.raises(TypeError):
        systems.LJ(device=DEV).potential(x)


def test_lj_bitwise_deterministic(hip_device):
    meta, data = fixture("sys_lj_n54_cut_shift")
    lj, _ = build(meta, data)
    idx = _row_index(500)
    x, w = data["x"][idx].to(DEV), data["w"][idx].to(DEV)
    a = run(lj.potential, x, w)
    b = run(lj.potential, x, w)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


# ------------------------------------------------------------ model integration
def _einstein_prior(boxlength):
    centers = fixture("sys_einstein_32x3_box_a600")[1]["centers"]
    return systems.EinsteinCrystal(centers, 3, boxlength=boxlength, alpha=600, device=DEV)


@pytest.fixture(scope="module")
def models():
    """Einstein.yaml's flow (2 x NSF_AR(96, K = 32, hidden 354)) and a 2-layer
    NSF_CL behind the Einstein prior; Gaussian_rnvp.yaml's behind a mixture."""
    torch.manual_seed(1234)
    B = L32 / 2
    ar = nfm.NormalizingFlowModel(_einstein_prior(L32),
                                  [nff.NSF_AR(dim=96, K=32, B=B, hidden_dim=354) for _ in range(2)]).to(DEV)
    cl = nfm.NormalizingFlowModel(_einstein_prior(None),
                                  [nff.NSF_CL(size=32, dim=3, K=8, B=B, hidden_dim=100, mask=[i])
                                   for i in range(2)]).to(DEV)
    gm = nfm.NormalizingFlowModel(systems.GaussianMixture([[-0.5, -0.5], [0.5, 0.5]], [0.25, 0.2], 20, 2, device=DEV),
                                  [nff.RealNVP(dim=40, hidden_dim=80) for _ in range(2)]).to(DEV)
    return {"ar": ar, "cl": cl, "gm": gm}


def _cpu_prior(prior):
    if isinstance(prior, systems.EinsteinCrystal):
        return systems.EinsteinCrystal(prior.centers.cpu(), prior.dim, boxlength=prior.boxlength, alpha=prior.alpha)
    return systems.GaussianMixture(prior.centers.cpu(), prior.vars.cpu(), prior.nparticles, prior.dim)


@pytest.mark.parametrize("kind", ["ar", "cl", "gm"])
def test_model_forward_log_prob_sample(kind, models, hip_device, monkeypatch):
    model = models[kind]
    prior = model.prior
    no_torch_path(prior, monkeypatch)
    cpu = _cpu_prior(prior)
    torch.manual_seed(7)
    x = prior.sample(40)
    with torch.no_grad():
        z, plp, ld = model(x)
        lp = model.log_prob(x)
    assert z.shape == (40, prior.width) and plp.shape == (40,) and ld.shape == (40,)
    torch.testing.assert_close(plp.cpu(), cpu.log_prob(z.cpu()), rtol=RTOL, atol=ATOL)
    torch.testing.assert_close(lp, plp + ld, rtol=2e-7, atol=2e-5)
    xs, lpx, zs = model.sample(40)
    assert xs.shape == (40, prior.width) and lpx.shape == (40,) and zs.shape == (40, prior.width)
    with torch.no_grad():
        xi, ldi = model.inverse(zs)
    torch.testing.assert_close(xi, xs, rtol=1e-6, atol=1e-6)
    torch.testing.assert_close(lpx.cpu(), cpu.log_prob(zs.cpu()) - ldi.cpu(), rtol=RTOL, atol=ATOL)
    name = "nfk_einstein_logprob" if kind != "gm" else "nfk_gmix_logprob"
    for call in (lambda: model.log_prob(x), lambda: model(x), lambda: model.sample(40)):
        assert counts_of(call).get(name) == 1


@pytest.mark.parametrize("kind", ["cl", "gm"])
def test_nan_row_raises_value_error(kind, models, hip_device):
    model = models[kind]
    prior = model.prior
    torch.manual_seed(8)
    x = prior.sample(40)
    model.log_prob(x)
    model(x)
    prior.log_prob(x)
    bad = x.clone()
    bad[17, 3] = float("nan")
    with pytest.raises(ValueError):
        model.log_prob(bad)
    with pytest.raises(ValueError):
        model(bad)
    with pytest.raises(ValueError):
        prior.log_prob(bad)
    with pytest.raises(ValueError):
        prior.log_prob(bad.requires_grad_())


@pytest.mark.parametrize("kind", ["ar", "cl"])
def test_train_step_grads_match_torch_path_prior(kind, models, hip_device):
    model = models[kind]
    prior = model.prior
    torch.manual_seed(9)
    x = prior.sample(40)
    opt = torch.optim.SGD(model.parameters(), lr=0.0)  # the step changes nothing; the gradients stay
    try:
        counts = counts_of(lambda: app.train_step(model, opt, x))
        assert counts.get("nfk_einstein_logprob") == 1 and counts.get("nfk_einstein_logprob_bwd") == 1
        got = {k: p.grad.clone() for k, p in model.named_parameters()}
        prior.use_kernels = False
        counts = counts_of(lambda: app.train_step(model, opt, x))
        assert "nfk_einstein_logprob" not in counts
        for k, p in model.named_parameters():
            assert torch.isfinite(got[k]).all(), k
            rel_close(got[k], p.grad, what=k)
    finally:
        del prior.use_kernels
        opt.zero_grad(set_to_none=True)


def test_reverse_kl_grads_match_cpu_path(hip_device):
    torch.manual_seed(11)
    layer = nff.RealNVP(dim=40, hidden_dim=80)
    sd = {k: v.detach().clone() for k, v in layer.state_dict().items()}

    def make(device):
        prior = systems.GaussianMixture([[-0.5, -0.5]], 0.25, 20, 2, device=device)
        target = systems.GaussianMixture([[-1., -1.], [1., 1.]], [0.4, 0.3], 20, 2, device=device)
        return prior, target

    prior, target = make(DEV)
    model = nfm.NormalizingFlowModel(prior, [layer]).to(DEV)
    torch.manual_seed(12)
    z = prior.sample((64,))

    class Fixed:  # the same draws for both paths
        def __init__(self, p, zz):
            self.p, self.zz = p, zz

        def sample(self, n):
            return self.zz

        def log_prob(self, v):
            return self.p.log_prob(v)

    def loss_and_grads(force_torch):
        prior.use_kernels = target.use_kernels = not force_torch
        try:
            model.prior = Fixed(prior, z)
            model.zero_grad(set_to_none=True)
            counts = counts_of(lambda: app.reverse_kl(model, target, 64).backward())
        finally:
            model.prior = prior
            del prior.use_kernels, target.use_kernels
        return counts, {k: p.grad.clone() for k, p in model.named_parameters()}

    counts, got = loss_and_grads(False)
    assert counts.get("nfk_gmix_logprob") == 2 and counts.get("nfk_gmix_logprob_bwd") == 1
    counts, want = loss_and_grads(True)
    assert "nfk_gmix_logprob" not in counts
    for k in got:
        assert torch.isfinite(got[k]).all() and got[k].abs().max() > 0, k
        rel_close(got[k], want[k], what=k)
    # and the CPU path's value of the loss on the same draws
    pc, tc = make("cpu")
    with torch.no_grad():
        x, ld = model.inverse(z)
        dev_loss = -target.log_prob(x).mean() + (prior.log_prob(z) - ld).mean()
        cpu_loss = -tc.log_prob(x.cpu()).mean() + (pc.log_prob(z.cpu()) - ld.cpu()).mean()
    torch.testing.assert_close(dev_loss.cpu(), cpu_loss, rtol=RTOL, atol=ATOL)


# ------------------------------------------------------------------------ graphs
def test_graphed_log_prob_and_sample(models, hip_device):
    model = models["ar"]
    torch.manual_seed(13)
    x = model.prior.sample(40)
    eager = model.log_prob(x).clone()
    graphed = GraphedLogProb(model, x)
    assert torch.equal(graphed(x), eager)
    x2 = model.prior.sample(40)
    eager2 = model.log_prob(x2).clone()
    assert torch.equal(graphed(x2), eager2)
    model.invalidate_caches()
    assert torch.equal(model.log_prob(x), eager)
    assert torch.equal(graphed(x), eager)

    cl = models["cl"]
    gs = GraphedSample(cl, 40)
    xs, lpx, zs = (t.clone() for t in gs())
    xs2, _, zs2 = gs()
    assert not torch.equal(zs, zs2) and xs.shape == (40, 96)  # every replay draws fresh values
    with torch.no_grad():
        xi, ldi = cl.inverse(zs)
    assert torch.equal(xi, xs)
    torch.testing.assert_close(lpx.cpu(), _cpu_prior(cl.prior).log_prob(zs.cpu()) - ldi.cpu(), rtol=RTOL, atol=ATOL)


# ---------------------------------------------------------------------- q_matrix
def test_q_matrix(models, hip_device):
    model = models["cl"]
    traj = fixture("sys_lj_n32_cut_shift")[1]["x"][torch.arange(64) % 37]
    lj = systems.LJ(pos_dir=traj, boxlength=L32, device=DEV, cutoff=1.6, shift=True)
    cfg = app.get_cfg_defaults()
    cfg.dataset.nparticles, cfg.dataset.dim, cfg.dataset.kT = 32, 3, 2.0
    torch.manual_seed(21)
    Q = app.q_matrix(cfg, model, lj, nsamples=100, batchsize=50)
    assert Q.shape == (2, 100, 2) and Q.device.type == "cuda" and Q.dtype == torch.float32
    # the same draws again: the flow's samples, then the trajectory rows
    torch.manual_seed(21)
    traj0, q00 = app.generate_from_nf(model, 100, batchsize=50)
    traj1 = lj.sample(100)
    assert torch.equal(Q[0, :, 0], q00)
    assert torch.equal(Q[1, :, 0], torch.cat([model.evaluate(traj1[:50]), model.evaluate(traj1[50:])]))
    cpu = systems.LJ(boxlength=L32, cutoff=1.6, shift=True)
    for col, tr in ((Q[0, :, 1], traj0), (Q[1, :, 1], traj1)):
        pos = tr.cpu().reshape(-1, 32, 3)
        ref = -cpu.potential(pos) / 2.0
        truth = -cpu.potential(pos.double()) / 2.0
        close_or_on_par(col, ref, truth, "q_matrix energies")
