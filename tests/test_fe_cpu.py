"""CPU checks of the free-energy layer: ``normalizingflow_amd.bar``'s fp64
restatement of the reference's BAR (applications/src/bar.py) against the
``fe_bar_*`` golden vectors, its batched / bootstrap forms, and
``app.fe_estimates`` / ``app.fe_diff`` (test.py:33-72).

Tolerance of every comparison with an fp64 value of the reference:

    tol = 64 (n_f + n_r) 2^-53 max(1, |Delta|)

Any-order fp64 summation of n positive terms is off by at most (n - 1) 2^-53
relative, an iterate holds two such sums, exp / log1p add a few ulps each, and
the map is a contraction with ratio <= 0.5 on these fixtures (the generator
asserts it), so the error of an iterate is at most doubled by the iterates
before it; 64 covers those terms with room to spare.
"""
import math

import numpy as np
import pytest
import torch

import golden_io as gio
from normalizingflow_amd import app, systems
from normalizingflow_amd import bar as B

BAR_CASES = gio.names("fe_bar_")
_CACHE = {}


def fixture(name):
    if name not in _CACHE:
        _CACHE[name] = gio.load(name)[:2]
    return _CACHE[name]


def tol_of(n_f, n_r, delta):
    return 64 * (n_f + n_r) * 2.0 ** -53 * max(1.0, abs(float(delta)))


def case_tol(data):
    return tol_of(data["w_f"].numel(), data["w_r"].numel(), data["bar_64"])


def boot_indices(P, n_f, n_r, seed):
    """Explicit int32 bootstrap rows (CPU generator; moved to a device by the caller)."""
    g = torch.Generator().manual_seed(seed)
    return (torch.randint(n_f, (P, n_f), dtype=torch.int32, generator=g),
            torch.randint(n_r, (P, n_r), dtype=torch.int32, generator=g))


def check_against_fixture(solve, data, label):
    """The three fixture checks shared by the CPU path and the kernel: iterate by
    iterate, the default stop, and the exponential averages.  ``solve(**kw)``
    returns bar_solve's (out, iters) for the fixture's work values."""
    tol = case_tol(data)
    hist = data["hist_64"]
    for k in range(1, len(hist) + 1):
        out, iters = solve(relative_tolerance=0.0, maximum_iterations=k)
        err = abs(float(out[0, 0]) - float(hist[k - 1]))
        print("%s iterate %d: err %.3g tol %.3g" % (label, k, err, tol))
        assert int(iters[0]) == k
        assert err <= tol, (label, k, err, tol)
    out, iters = solve()
    err = abs(float(out[0, 0]) - float(data["bar_64"]))
    ref_err = abs(float(data["bar_ref"]) - float(data["bar_64"]))
    print("%s default stop: iters %d err %.3g tol %.3g reference's own %.3g" % (label, int(iters[0]), err, tol,
                                                                               ref_err))
    assert int(iters[0]) == int(data["iters_64"])
    assert err <= tol
    assert err <= 2 * max(ref_err, tol)  # the project's convention: within 2x the reference's own error
    assert abs(float(out[0, 1]) - float(data["lme_f_64"])) <= tol
    assert abs(float(out[0, 2]) - float(data["lme_r_64"])) <= tol


def test_fixture_set():
    assert len(BAR_CASES) == 6 and "fe_q_lj" in gio.names("fe_")
    shapes = sorted((gio.load(n)[0]["n_f"], gio.load(n)[0]["n_r"]) for n in BAR_CASES)
    assert shapes == [(1, 1), (37, 29), (500, 400), (500, 400), (500, 400), (4096, 3277)]


@pytest.mark.parametrize("name", BAR_CASES)
def test_cpu_path_against_fixture(name):
    _, data = fixture(name)
    check_against_fixture(lambda **kw: B.bar_solve(data["w_f"], data["w_r"], **kw), data, name)
    assert abs(B.BAR(data["w_f"].numpy(), data["w_r"].numpy(), relative_tolerance=1e-13)
               - float(data["root_64"])) <= case_tol(data)


def test_reference_names_and_return_types():
    _, data = fixture("fe_bar_n37_d07")
    wf, wr = data["w_f"], data["w_r"]
    v = B.BAR(wf.numpy(), wr.numpy())
    assert isinstance(v, float) and isinstance(B.BAR(wf, wr), float)
    assert v == B.BAR(wf, wr) == float(B.bar_solve(wf, wr)[0][0, 0])
    # BARzero is zeroed by the root, and one iteration is D - BARzero(D)
    assert abs(B.BARzero(wf.numpy(), wr.numpy(), float(data["root_64"]))) <= 4 * case_tol(data)
    first = float(B.bar_solve(wf, wr, relative_tolerance=0.0, maximum_iterations=1)[0][0, 0])
    assert 0.0 - B.BARzero(wf.numpy(), wr.numpy(), 0.0) == first
    a = np.array([-3.0, 700.0, 710.5])
    assert abs(B.logsum(a) - (710.5 + math.log(math.exp(-713.5) + math.exp(-10.5) + 1.0))) <= 1e-12
    with pytest.raises(ValueError):
        B.bar_solve(wf, wr, maximum_iterations=0)
    with pytest.raises(ValueError):
        B.bar_solve(wf, wr, relative_tolerance=float("nan"))


def test_identity_index_same_bits():
    _, data = fixture("fe_bar_n500_d37")
    wf, wr = data["w_f"], data["w_r"]
    plain = B.bar_solve(wf, wr)
    ident = B.bar_solve(wf, wr, idx_f=torch.arange(500, dtype=torch.int32).reshape(1, -1),
                        idx_r=torch.arange(400, dtype=torch.int32).reshape(1, -1))
    assert torch.equal(plain[0], ident[0]) and torch.equal(plain[1], ident[1])


def test_joint_call_equals_separate_calls():
    _, data = fixture("fe_bar_n500_dm3")
    wf, wr = data["w_f"], data["w_r"]
    idx_f, idx_r = boot_indices(2, 500, 400, 11)
    out, iters = B.bar_solve(wf, wr, idx_f=idx_f, idx_r=idx_r)
    assert out.shape == (2, 3) and out.dtype == torch.float64 and iters.dtype == torch.int32
    for p in range(2):
        o, i = B.bar_solve(wf, wr, idx_f=idx_f[p:p + 1], idx_r=idx_r[p:p + 1])
        assert torch.equal(o[0], out[p]) and int(i[0]) == int(iters[p])
    # and a problem on gathered rows is the plain problem on the gathered vectors
    o, i = B.bar_solve(wf[idx_f[1].long()], wr[idx_r[1].long()])
    assert torch.equal(o[0], out[1]) and int(i[0]) == int(iters[1])


def test_bootstrap_draws_idx_f_then_idx_r_per_chunk():
    _, data = fixture("fe_bar_n37_d07")
    wf, wr = data["w_f"], data["w_r"]
    out = B.bootstrap(wf, wr, 5, generator=torch.Generator().manual_seed(3))
    assert out.shape == (5, 3) and out.dtype == torch.float64
    g = torch.Generator().manual_seed(3)
    idx_f = torch.randint(37, (5, 37), dtype=torch.int32, generator=g)
    idx_r = torch.randint(29, (5, 29), dtype=torch.int32, generator=g)
    assert torch.equal(out, B.bar_solve(wf, wr, idx_f=idx_f, idx_r=idx_r)[0])
    # chunks of two problems: 2 * 4 * (37 + 29) bytes of indices each
    chunked = B.bootstrap(wf, wr, 5, generator=torch.Generator().manual_seed(3), chunk_bytes=2 * 4 * 66)
    g = torch.Generator().manual_seed(3)
    rows = []
    for c in (2, 2, 1):
        jf = torch.randint(37, (c, 37), dtype=torch.int32, generator=g)
        jr = torch.randint(29, (c, 29), dtype=torch.int32, generator=g)
        rows.append(B.bar_solve(wf, wr, idx_f=jf, idx_r=jr)[0])
    assert torch.equal(chunked, torch.cat(rows))


def test_fe_estimates_against_fixture():
    meta, data = fixture("fe_q_lj")
    cfg = app.get_cfg_defaults()
    cfg.dataset.nparticles, cfg.dataset.kT = meta["nparticles"], meta["kT"]
    Q = data["Q"].clone()
    bar, md, nf = app.fe_estimates(cfg, Q)
    assert torch.equal(Q, data["Q"]), "fe_estimates modified Q"
    tol = tol_of(64, 64, data["delta_64"]) / meta["nparticles"] * meta["kT"]
    for ours, key in ((bar, "bar"), (md, "md"), (nf, "nf")):
        assert ours.dim() == 0 and ours.dtype == torch.float64
        err = abs(float(ours) - float(data[key]))
        print("fe_q_lj %s: err %.3g tol %.3g" % (key, err, tol))
        assert err <= tol
    six = app.fe_estimates(cfg, Q, nboot=50, generator=torch.Generator().manual_seed(5))
    assert len(six) == 6 and all(float(a) == float(b) for a, b in zip(six[:3], (bar, md, nf)))
    assert all(e.dim() == 0 and 0.0 < float(e) < 1.0 for e in six[3:])


def test_non_finite_work_values_end_the_loop_with_nan():
    """With the max-shifted sums of the iteration, a +inf among finite forward
    (or reverse) values is a zero term: g(+inf) = -inf on the forward side,
    g(-inf) - inf = -inf on the reverse side, and the estimate stays finite, as
    the reference's does.  A work vector that holds nothing but +inf has an
    all -inf sum, whose shift is inf - inf; a -inf reverse value gives
    g(+inf) + inf.  Both are NaN at the first iterate, which ends the loop."""
    _, data = fixture("fe_bar_n37_d07")
    wf, wr = data["w_f"], data["w_r"]
    inf = float("inf")
    for f, r in ((torch.full((3,), inf), wr), (wf, torch.full((2,), inf)),
                 (wf, torch.cat((wr, torch.tensor([-inf]))))):
        out, iters = B.bar_solve(f, r, maximum_iterations=50)
        assert math.isnan(float(out[0, 0])) and int(iters[0]) == 1 < 50
    out, iters = B.bar_solve(torch.cat((wf, torch.tensor([inf]))), wr, maximum_iterations=50)
    assert math.isfinite(float(out[0, 0])) and 1 < int(iters[0]) < 50


def test_large_exponents_stay_finite():
    """n_f = n_r = 1 and w_f = -w_r = w: M = 0 and both exponents are a = w - D,
    so an iterate is D' = fl(g(a) - w_r) - g(a) = fl(g(a) + w) - g(a).  From
    D = 0 with w = 900, g(900) = -(900 + log1p(exp(-900))) = -900 exactly and
    D' = 0 - (-900) = w exactly; with w = -900, g(-900) = -(0 + log1p(0)) = -0
    and D' = -900 + 0 = w.  The second iterate has a = 0, g = -log 2, and
    D' = fl(w - log 2) + log 2: w to within an ulp of 900, which stops the loop.
    The reference's form evaluates exp(900) here."""
    for w in (900.0, -900.0):
        wf, wr = torch.tensor([w]), torch.tensor([-w])
        out, iters = B.bar_solve(wf, wr, maximum_iterations=1)
        assert float(out[0, 0]) == w and int(iters[0]) == 1
        out, iters = B.bar_solve(wf, wr)
        assert abs(float(out[0, 0]) - w) <= 2 * 2.0 ** -43 and int(iters[0]) == 2  # ulp(900) = 2^-43
        assert float(out[0, 1]) == w and float(out[0, 2]) == -w


class _GaussianFlow:
    """A stand-in for a trained flow (the flows refuse CPU tensors): N(0, sigma^2 I)
    with the model's ``sample`` / ``evaluate`` signatures."""

    def __init__(self, width, sigma, generator):
        self.width, self.sigma, self.g = width, sigma, generator

    def evaluate(self, x):
        return (-0.5 * (x / self.sigma).square().sum(1)
                - self.width * (math.log(self.sigma) + 0.5 * math.log(2 * math.pi)))

    def sample(self, n):
        x = torch.randn(n, self.width, generator=self.g) * self.sigma
        return x, self.evaluate(x), None


def test_fe_diff_between_two_normalised_densities_is_zero():
    """fe_diff's plumbing on the CPU path: both the stand-in flow and the
    Gaussian-mixture target are normalised densities (kT = 1), so the log ratio
    of their normalisers is 0 and ``bar`` must land within 5 bootstrap standard
    errors of it.  Seed 2024 with N = 2000 passes on the CPU path (checked when
    this test was written: bar = -0.0252, bar_err = 0.0135 per particle, 1.9
    standard errors)."""
    torch.manual_seed(2024)
    cfg = app.get_cfg_defaults()
    cfg.dataset.nparticles, cfg.dataset.dim, cfg.dataset.kT = 2, 2, 1.0
    target = systems.GaussianMixture([[-1.0, -1.0], [1.0, 1.0]], 0.5, 2, 2)
    model = _GaussianFlow(4, 1.5, torch.Generator().manual_seed(2024))
    res = app.fe_diff(cfg, model, target, 2000, return_err=True, nboot=200, batchsize=500,
                      generator=torch.Generator().manual_seed(7))
    bar, md, nf, bar_err, md_err, nf_err = (float(v) for v in res)
    print("bar %.4g +- %.4g  md %.4g +- %.4g  nf %.4g +- %.4g" % (bar, bar_err, md, md_err, nf, nf_err))
    assert all(v.dim() == 0 and v.dtype == torch.float64 for v in res)
    assert 0.0 < bar_err < 0.1
    assert abs(bar) <= 5 * bar_err
    torch.manual_seed(2024)
    model.g.manual_seed(2024)
    three = app.fe_diff(cfg, model, target, 2000)
    assert len(three) == 3 and all(float(a) == b for a, b in zip(three, (bar, md, nf)))
