"""CPU checks of the multistate layer: ``normalizingflow_amd.mbar``'s fp64 torch
path against the ``mbar_*`` golden vectors (tests/golden/make_mbar_golden.py),
its covariance, bootstrap and ``MBAR`` forms, and ``app.fe_estimates(...,
emus=True)`` / ``app.fe_diff_no_training`` (test.py:61-63, 74-88).

Tolerance of every comparison with an fp64 value of the fixtures:

    tol = 64 N 2^-53 max(1, max|f|) max(1, kappa)

Two any-order fp64 sums of N positive terms differ by about N 2^-53 relative, a
few ulps of exp / log on arguments of size |f| add to it, and a Newton step
amplifies an error of the gradient by at most ||H_r^{-1}||; kappa is the
fixture's ``||H_r^{-1}||_inf max N_k`` over the Newton steps taken.  The K = 2
cases give 8e-14 to 6.7e-7 (kappa 2 to 350), the wells 3e-9 to 7e-8.
"""
import math

import numpy as np
import pytest
import torch

import golden_io as gio
from normalizingflow_amd import app
from normalizingflow_amd import bar as B
from normalizingflow_amd import mbar as M

MBAR_CASES = gio.names("mbar_")
_CACHE = {}


def fixture(name):
    """(meta, data) of an ``mbar_*`` fixture, with ``u`` rebuilt for the K = 2
    views: u[:n_f] = (0, w_f), u[n_f:] = (w_r, 0)."""
    if name not in _CACHE:
        meta, data, _ = gio.load(name)
        if "source" in meta:
            src = gio.load(meta["source"])[1]
            n_f, n_r = src["w_f"].numel(), src["w_r"].numel()
            u = torch.zeros(n_f + n_r, 2)
            u[:n_f, 1] = src["w_f"]
            u[n_f:, 0] = src["w_r"]
            data["u"] = u
        data["n_k"] = [int(n) for n in data["n_k"]]
        _CACHE[name] = (meta, data)
    return _CACHE[name]


def tol_of(N, f, kappa):
    return 64 * N * 2.0 ** -53 * max(1.0, float(torch.as_tensor(f).abs().max())) * max(1.0, float(kappa))


def case_tol(data):
    return tol_of(data["u"].shape[0], data["hist_64"][-1], data["kappa"])


def boot_rows(P, n_k, seed):
    """Explicit int32 stratified bootstrap rows (CPU generator; moved to a device by the caller)."""
    g = torch.Generator().manual_seed(seed)
    blocks, o = [], 0
    for n in n_k:
        blocks.append(torch.randint(n, (P, n), dtype=torch.int32, generator=g) + o)
        o += n
    return torch.cat(blocks, dim=1)


def cpu_reference(u, n_k, idx=None, **kw):
    """The fp64 CPU path on u (rows ``idx``), with the tolerance of every problem
    worked out from its own run: (f, iters, gram, tol [P]), kappa taken over the
    Newton steps the run took, as the generator takes it."""
    u64 = u.double()
    rows = u64.unsqueeze(0) if idx is None else u64[idx.long()]
    trace = []
    f, iters, gram = M._solve_torch(rows, list(n_k), torch.zeros(len(n_k), dtype=torch.float64),
                                    kw.get("maximum_iterations", 1000), kw.get("relative_tolerance", 1e-8),
                                    trace=trace)
    kappa = torch.zeros(rows.shape[0], dtype=torch.float64)
    for taken, H in trace:
        k = torch.linalg.inv_ex(H).inverse.abs().sum(dim=2).amax(dim=1) * max(n_k)
        kappa = torch.where(taken, torch.maximum(kappa, k), kappa)
    tol = [tol_of(rows.shape[1], f[p], kappa[p]) for p in range(rows.shape[0])]
    return f, iters, gram, tol


def check_against_fixture(solve, data, label):
    """The fixture checks shared by the CPU path and the kernel: iterate by
    iterate, then the default stop with ``iters``, ``gram`` and the outside
    reference.  ``solve(**kw)`` returns mbar_solve's (f, iters, gram)."""
    tol = case_tol(data)
    hist = data["hist_64"]
    for k in range(1, len(hist) + 1):
        f, iters, _ = solve(relative_tolerance=0.0, maximum_iterations=k)
        err = float((f[0] - hist[k - 1]).abs().max())
        print("%s iterate %d: err %.3g tol %.3g" % (label, k, err, tol))
        assert int(iters[0]) == k
        assert err <= tol, (label, k, err, tol)
    f, iters, gram = solve()
    err = float((f[0] - hist[-1]).abs().max())
    gerr = float((gram[0] - data["gram_64"]).abs().max())
    print("%s default stop: iters %d err %.3g gram err %.3g tol %.3g" % (label, int(iters[0]), err, gerr, tol))
    assert float(f[0, 0]) == 0.0
    assert int(iters[0]) == int(data["iters_64"])
    assert err <= tol
    assert gerr <= tol
    assert torch.equal(gram[0], gram[0].T)
    if "root_64" in data:  # the reference's BAR root, within 2x the reference's own |bar_64 - root_64|
        rerr = abs(float(f[0, 1]) - float(data["root_64"]))
        print("%s: |f_1 - root_64| %.3g, reference's own %.3g" % (label, rerr, float(data["bar_root_err"])))
        assert rerr <= tol
        assert rerr <= 2 * max(float(data["bar_root_err"]), tol)
    else:          # the SciPy minimum, within its own first-order error
        berr = float((f[0] - data["f_bfgs"]).abs().max())
        print("%s: |f - f_bfgs| %.3g, BFGS's own %.3g" % (label, berr, float(data["bfgs_err"])))
        assert berr <= tol + 2 * float(data["bfgs_err"])


def test_fixture_set():
    assert len(MBAR_CASES) == 9
    ks = sorted((gio.load(n)[0]["K"], len(gio.load(n)[1]["n_k"])) for n in MBAR_CASES)
    assert ks == [(2, 2)] * 6 + [(3, 3), (5, 5), (8, 8)]
    assert sorted(gio.load(n)[0]["source"] for n in MBAR_CASES if n.startswith("mbar_k2_")) == gio.names("fe_bar_")


@pytest.mark.parametrize("name", MBAR_CASES)
def test_cpu_path_against_fixture(name):
    _, data = fixture(name)
    check_against_fixture(lambda **kw: M.mbar_solve(data["u"], data["n_k"], **kw), data, name)
    f, _, _ = M.mbar_solve(data["u"].numpy(), data["n_k"], relative_tolerance=1e-13)
    assert float((f[0] - data["f_root"]).abs().max()) <= case_tol(data)


@pytest.mark.parametrize("name", ["mbar_k2_n500_d300", "mbar_k2_n4096_d120", "mbar_k8_wells"])
def test_derived_tolerance_is_the_fixtures(name):
    """``cpu_reference`` works the tolerance of a run out of the run itself (the
    GPU tests use it on shapes no fixture holds); on a fixture it must give the
    generator's."""
    _, data = fixture(name)
    f, iters, gram, tol = cpu_reference(data["u"], data["n_k"])
    assert int(iters[0]) == int(data["iters_64"])
    assert abs(tol[0] / case_tol(data) - 1.0) <= 1e-6


def test_start_and_other_state_counts():
    """A start at the root stops at the first iteration; K = 9, which the kernel
    is not built for, is the torch path's like any other."""
    _, data = fixture("mbar_k3_wells")
    f, iters, _ = M.mbar_solve(data["u"], data["n_k"], f0=data["f_root"] + 5.0)  # the gauge is taken out
    assert int(iters[0]) == 1 and float((f[0] - data["f_root"]).abs().max()) <= case_tol(data)
    g = torch.Generator().manual_seed(4)
    K, n = 9, 40
    mu = torch.linspace(0.0, 2.0, K)
    x = (mu.repeat_interleave(n) + torch.randn(K * n, generator=g)).double()
    u = 0.5 * (x[:, None] - mu[None, :].double()) ** 2 + 3.0 * torch.arange(K)
    f, iters, gram = M.mbar_solve(u, [n] * K)
    W = torch.softmax((math.log(n) + f[0])[None, :] - u, dim=1)
    assert float((W.sum(0) - n).abs().max()) <= 1e-6 and 1 < int(iters[0]) < 20
    assert float((f[0] - 3.0 * torch.arange(K)).abs().max()) < 1.0  # equal widths: f is the offsets, up to sampling
    assert gram.shape == (1, K, K)


def test_covariance_against_the_definition():
    """Theta = W_w^T (I - W_w N W_w^T)^+ W_w with W_w = W / N_k, on N = 180."""
    g = torch.Generator().manual_seed(3)
    n_k = [60, 70, 50]
    mu, sig = torch.tensor([0.0, 0.8, 1.5]), torch.tensor([1.0, 0.8, 0.6])
    x = torch.cat([mu[k] + sig[k] * torch.randn(n_k[k], generator=g) for k in range(3)]).double()
    u = 0.5 * ((x[:, None] - mu[None, :].double()) / sig[None, :].double()) ** 2
    f, _, gram = M.mbar_solve(u, n_k, relative_tolerance=1e-12)
    n = torch.tensor(n_k, dtype=torch.float64)
    Ww = torch.softmax((n.log() + f[0])[None, :] - u, dim=1) / n
    direct = Ww.T @ torch.linalg.pinv(torch.eye(180, dtype=torch.float64) - Ww @ torch.diag(n) @ Ww.T) @ Ww
    theta = M.mbar_covariance(gram, n_k)[0]

    def dvar(T):
        d = torch.diagonal(T)
        return d[:, None] + d[None, :] - 2 * T

    # Theta is defined up to the gauge (a multiple of 1 1^T); differences f_j - f_i are not
    err = float((dvar(theta) - dvar(direct)).abs().max())
    print("covariance: max |dvar - definition| %.3g" % err)
    assert err <= 1e-12 * float(dvar(direct).abs().max()) * 180
    for i, j in ((0, 1), (0, 2), (1, 2)):
        assert abs(float(M.mbar_std(gram, n_k, i, j)[0]) - math.sqrt(float(dvar(direct)[i, j]))) <= 1e-10


def test_asymptotic_sd_against_a_bootstrap():
    _, data = fixture("mbar_k2_n500_d37")
    u, n_k = data["u"], data["n_k"]
    _, _, gram = M.mbar_solve(u, n_k)
    sd = float(M.mbar_std(gram, n_k, 0, 1)[0])
    f, iters, _ = M.bootstrap(u, n_k, 200, generator=torch.Generator().manual_seed(12))
    assert f.shape == (200, 2) and iters.shape == (200,)
    boot = float(f[:, 1].std())
    print("asymptotic sd %.4g, 200-replica bootstrap %.4g" % (sd, boot))
    assert boot / 1.5 <= sd <= boot * 1.5


def test_bootstrap_rows_identity_and_stratification():
    _, data = fixture("mbar_k3_wells")
    u, n_k = data["u"], data["n_k"]
    N = sum(n_k)
    plain = M.mbar_solve(u, n_k)
    ident = M.mbar_solve(u, n_k, idx=torch.arange(N, dtype=torch.int32).reshape(1, -1))
    assert all(torch.equal(a, b) for a, b in zip(plain, ident))
    # bootstrap draws its blocks in state order through the generator, chunk by chunk
    out = M.bootstrap(u, n_k, 5, generator=torch.Generator().manual_seed(3))
    idx = boot_rows(5, n_k, 3)
    assert all(torch.equal(a, b) for a, b in zip(out, M.mbar_solve(u, n_k, idx=idx)))
    o = 0
    for n in n_k:  # positions of state k's block hold rows of state k's block
        blk = idx[:, o:o + n]
        assert int(blk.min()) >= o and int(blk.max()) < o + n and len(blk.unique()) > n // 2
        o += n
    chunked = M.bootstrap(u, n_k, 5, generator=torch.Generator().manual_seed(3), chunk_bytes=2 * 4 * N)
    g = torch.Generator().manual_seed(3)
    rows = []
    for c in (2, 2, 1):
        blocks, o = [], 0
        for n in n_k:
            blocks.append(torch.randint(n, (c, n), dtype=torch.int32, generator=g) + o)
            o += n
        rows.append(M.mbar_solve(u, n_k, idx=torch.cat(blocks, dim=1))[0])
    assert torch.equal(chunked[0], torch.cat(rows))
    # a problem on gathered rows is the plain problem on the gathered matrix
    # (to the tolerance: a batched and a single matrix product need not sum in one order)
    f, it, gr, tol = cpu_reference(u[idx[1].long()], n_k)
    assert int(it[0]) == int(out[1][1])
    assert float((f[0] - out[0][1]).abs().max()) <= tol[0] and float((gr[0] - out[2][1]).abs().max()) <= tol[0]


def test_mbar_class_is_the_reference_call_shape():
    meta, data, _ = gio.load("fe_q_lj")
    Q = data["Q"] - torch.stack((data["Q"][1][:, 0].min(), data["Q"][1][:, 1].min()))
    solver = M.MBAR(-Q)
    c = solver.norm_const(niter=40)
    assert c.shape == (2,) and c.dtype == torch.float64 and float(c[0]) == 1.0
    f, iters, _ = M.mbar_solve((-Q).reshape(-1, 2), [64, 64], maximum_iterations=40)
    assert torch.equal(torch.exp(-f[0]), c) and int(solver.iters[0]) == int(iters[0]) < 40
    capped = M.MBAR((-Q).numpy())
    capped.norm_const(niter=2)
    assert int(capped.iters[0]) == 2 < int(solver.iters[0])
    with pytest.raises(ValueError):
        M.MBAR(-Q[0])
    assert not hasattr(solver, "norm_const_err")


def test_fe_estimates_emus_against_fixture():
    """For two states the multistate fixed point is the BAR root, so ``emus``
    equals ``bar`` evaluated at the converged root."""
    meta, data, _ = gio.load("fe_q_lj")
    cfg = app.get_cfg_defaults()
    cfg.dataset.nparticles, cfg.dataset.kT = meta["nparticles"], meta["kT"]
    Q = data["Q"].clone()
    three = app.fe_estimates(cfg, Q)
    four = app.fe_estimates(cfg, Q, emus=True)
    assert torch.equal(Q, data["Q"]), "fe_estimates modified Q"
    assert len(three) == 3 and len(four) == 4
    assert all(float(a) == float(b) for a, b in zip(three, four[:3]))
    for v, key in zip(three, ("bar", "md", "nf")):  # the default call returns what it returned
        assert abs(float(v) - float(data[key])) <= (64 * 128 * 2.0 ** -53 * abs(float(data["delta_64"]))
                                                    / meta["nparticles"] * meta["kT"])  # tests/test_fe_cpu.py's
    emus = four[3]
    assert emus.dim() == 0 and emus.dtype == torch.float64
    root = B.BAR(data["w_f"], data["w_r"], relative_tolerance=1e-13)
    s0, s1 = data["Q"][1][:, 0].min(), data["Q"][1][:, 1].min()
    want = (float(s0 - s1) + root) / meta["nparticles"] * meta["kT"]
    u = -(data["Q"] - torch.stack((s0, s1))).reshape(-1, 2)
    f, _, gram = M.mbar_solve(u, [64, 64])
    # kappa of this problem, as the generator defines it, at the solution
    n = torch.tensor([64.0, 64.0], dtype=torch.float64)
    kappa = 64.0 / float(n[1] - gram[0, 1, 1])
    tol = tol_of(128, f[0], kappa) / meta["nparticles"] * meta["kT"]
    print("emus %.12g bar-at-root %.12g err %.3g tol %.3g" % (float(emus), want, abs(float(emus) - want), tol))
    assert abs(float(emus) - want) <= tol
    eight = app.fe_estimates(cfg, Q, nboot=50, generator=torch.Generator().manual_seed(5), emus=True)
    six = app.fe_estimates(cfg, Q, nboot=50, generator=torch.Generator().manual_seed(5))
    assert len(eight) == 8 and len(six) == 6
    assert all(float(a) == float(b) for a, b in zip(eight[:4], four))
    assert all(float(a) == float(b) for a, b in zip(eight[4:7], six[3:]))
    want_err = float(M.mbar_std(gram, [64, 64], 0, 1)[0]) / meta["nparticles"] * meta["kT"]
    assert eight[7].dim() == 0 and float(eight[7]) == want_err and 0.0 < want_err < 1.0
    assert float(six[3]) / 2 <= want_err <= float(six[3]) * 2  # the bootstrap sd of bar, 50 replicas


class _Target:
    """A normalised Gaussian N(mu, s^2 I) on nparticles x dim with the targets'
    ``potential`` / ``sample`` signatures: U = -log p, so its free energy is 0."""

    def __init__(self, width, mu, s, generator):
        self.width, self.mu, self.s, self.g = width, mu, s, generator

    def potential(self, x):
        x = x.reshape(len(x), -1)
        return (0.5 * ((x - self.mu) / self.s).square().sum(1)
                + self.width * (math.log(self.s) + 0.5 * math.log(2 * math.pi)))

    def sample(self, n):
        return (self.mu + self.s * torch.randn(n, self.width, generator=self.g)).reshape(n, 2, 2)


class _PriorOnly:
    def __init__(self, prior):
        self.prior = prior


def test_fe_diff_no_training_between_two_normalised_densities():
    """A Normal prior against a normalised Gaussian target at kT = 1: both free
    energies are 0, and the estimate must land within 5 asymptotic standard
    errors of it; it is mbar_solve of the Q that the same seeded draws give."""
    torch.manual_seed(99)
    cfg = app.get_cfg_defaults()
    cfg.dataset.nparticles, cfg.dataset.dim, cfg.dataset.kT = 2, 2, 1.0
    prior = torch.distributions.MultivariateNormal(torch.zeros(4), torch.eye(4))
    target = _Target(4, 0.5, 0.8, torch.Generator().manual_seed(9))
    out = app.fe_diff_no_training(cfg, _PriorOnly(prior), target, 400)
    assert out.shape == (2,) and out.dtype == torch.float64 and float(out[0]) == 0.0
    torch.manual_seed(99)
    target.g.manual_seed(9)
    x0 = prior.sample((400,))
    x1 = target.sample(400).reshape(400, -1)
    u = -torch.cat((torch.stack((prior.log_prob(x0), -target.potential(x0)), 1),
                    torch.stack((prior.log_prob(x1), -target.potential(x1)), 1)))
    f, _, gram = M.mbar_solve(u, [400, 400])
    assert torch.equal(out, f[0] / 2)
    sd = float(M.mbar_std(gram, [400, 400], 0, 1)[0]) / 2
    print("fe_diff_no_training %.4g +- %.4g" % (float(out[1]), sd))
    assert 0.0 < sd < 0.1 and abs(float(out[1])) <= 5 * sd


def test_argument_errors():
    _, data = fixture("mbar_k3_wells")
    u, n_k = data["u"], data["n_k"]
    with pytest.raises(ValueError, match="at least 2 states"):
        M.mbar_solve(u[:, :1], [u.shape[0]])
    with pytest.raises(ValueError, match="at least 1"):
        M.mbar_solve(u, [n_k[0] + n_k[1], 0, n_k[2]])
    with pytest.raises(ValueError, match="sum to"):
        M.mbar_solve(u, [n_k[0], n_k[1], n_k[2] + 1])
    with pytest.raises(ValueError, match="K = len"):
        M.mbar_solve(u, n_k + [1])
    with pytest.raises(ValueError, match="maximum_iterations"):
        M.mbar_solve(u, n_k, maximum_iterations=0)
    with pytest.raises(ValueError, match="relative_tolerance"):
        M.mbar_solve(u, n_k, relative_tolerance=float("nan"))
    with pytest.raises(ValueError, match="idx must be"):
        M.mbar_solve(u, n_k, idx=torch.zeros(2, 5, dtype=torch.int32))
    with pytest.raises(ValueError, match="f0"):
        M.mbar_solve(u, n_k, f0=[0.0, 1.0])
    with pytest.raises(ValueError, match="at least 1"):
        M.mbar_covariance(torch.eye(2, dtype=torch.float64), [3, 0])


def test_nan_energy_ends_the_loop():
    _, data = fixture("mbar_k3_wells")
    u = data["u"].clone()
    u[17, 1] = float("nan")
    f, iters, gram = M.mbar_solve(u, data["n_k"], maximum_iterations=50)
    assert bool(torch.isnan(f[0, 1:]).all()) and int(iters[0]) == 1
    assert bool(torch.isnan(gram).any())
