"""Hamiltonian switching on the per-step path (systems.Switch, app.switching_work,
app.fe_switching, app.fe_stratified) in fp64 on the CPU: the integrator and the
work against a restatement written here, chunks and row blocks, the instantaneous
switch, the exact answer between two normalised Einstein crystals, and the
argument errors."""
import math

import numpy as np
import pytest
import torch

from normalizingflow_amd import app, bar, rng, systems

F64 = torch.float64


def _pair(n=2, alpha=80.0, L=10.0, seed=5):
    """An Einstein crystal and an LJ target over n particles near a line of
    spacing 1.1, and 6 fp64 configurations."""
    g = torch.Generator().manual_seed(seed)
    centers = torch.zeros(n, 3, dtype=F64)
    centers[:, 0] = 1.1 * torch.arange(n, dtype=F64) - 0.55 * (n - 1)
    A = systems.EinsteinCrystal(centers, 3, boxlength=None, alpha=alpha)
    A.centers = centers  # fp64 centres: the restatement below uses the same numbers
    B = systems.LJ(boxlength=L, cutoff=2.5)
    x = centers + 0.05 * torch.randn(6, n, 3, generator=g, dtype=F64)
    return A, B, x


def test_three_steps_against_the_hand_restatement():
    """u_A = alpha/2 |x - c|^2 + D/2 log(2 pi / alpha); U_B of two particles is one
    shifted, cut pair term; forces by autograd of these two lines; the integrator,
    the coefficients and the work from the issue's formulas."""
    alpha, kT, dt, gamma, mass, seed, step0, row_base = 80.0, 0.7, 0.004, 3.0, 1.3, 11, 2, 4
    A, B, x0 = _pair(2, alpha)
    c = A.centers
    lam = np.array([0.0, 0.0, 0.0, 0.25, 0.25, 1.0], dtype=np.float32)  # steps 2, 3, 4: ramp, flat, ramp
    s6 = (1.0 / 2.5) ** 6

    def u_a(x):
        return 0.5 * alpha * ((x - c) ** 2).sum((1, 2)) + 0.5 * 6 * math.log(2 * math.pi / alpha)

    def u_b(x):
        r = (x[:, 0] - x[:, 1]).norm(dim=-1)
        p6 = (1.0 / r) ** 6
        return 4.0 * (p6 * p6 - p6 - s6 * s6 + s6)

    def force(fn, x):
        x = x.detach().requires_grad_()
        return -torch.autograd.grad(fn(x).sum(), x)[0]

    v0 = math.sqrt(kT / mass) * rng.philox_normal(seed, 6, 2, 3, step0, row_base, tag=1, dtype=F64)
    hb, hd, c1 = 0.5 * dt / mass, 0.5 * dt, math.exp(-gamma * dt)
    c2 = math.sqrt(kT / mass * (1.0 - c1 * c1))
    x, v, w = x0.clone(), v0.clone(), torch.zeros(6, dtype=F64)
    for k in range(3):
        l0, l1 = float(lam[step0 + k]), float(lam[step0 + k + 1])
        if l1 != l0:
            w = w + (l1 - l0) * (u_b(x) / kT - u_a(x))
        a, b = (1.0 - l1) * kT, l1
        xi = rng.philox_normal(seed, 6, 2, 3, step0 + k, row_base, tag=0, dtype=F64)
        v = v + hb * (a * force(u_a, x) + b * force(u_b, x))  # g_A = d log p_A / dx = -du_A / dx
        x = x + hd * v
        v = c1 * v + c2 * xi
        x = x + hd * v
        v = v + hb * (a * force(u_a, x) + b * force(u_b, x))
    sw = systems.Switch(A, B, kT=kT)
    sw.set_velocity(None)
    xs, ws, en = sw.switch(lam, nsteps=3, dt=dt, gamma=gamma, mass=mass, seed=seed, init_pos=x0, step0=step0,
                           row_base=row_base)
    assert xs.dtype == F64 and ws.dtype == F64 and en.shape == (6, 2)
    for got, want, what in ((xs, x, "x"), (sw.get_velocity(), v, "v"), (ws, w, "w"), (en[:, 0], u_a(x), "u_A"),
                            (en[:, 1], u_b(x), "U_B")):
        err = float((got - want).abs().max())
        print("hand restatement %s: max error %.3g" % (what, err))
        assert err <= 1e-12, (what, err)
    assert float(ws.abs().min()) > 0


def test_chunks_and_row_blocks_join_exactly():
    A, B, x0 = _pair(5)
    lam = torch.linspace(0, 1, 12)
    kw = dict(dt=0.004, seed=7)
    sw = systems.Switch(A, B, kT=0.9)
    sw.set_velocity(None)
    whole = sw.switch(lam, init_pos=x0, record_every=2, **kw)
    v_whole = sw.get_velocity()
    assert len(whole) == 5 and whole[3].shape == (5, 6, 5, 3) and whole[4].shape == (5, 6, 2)
    v0 = math.sqrt(0.9) * rng.philox_normal(7, 6, 5, 3, 0, tag=1, dtype=F64)
    # 4 + 7 with step0 and the work carried
    first = sw.switch(lam, nsteps=4, init_pos=x0, init_velocity=v0, **kw)
    second = sw.switch(lam, nsteps=7, step0=4, work=first[1], **kw)
    for a, b in zip(whole[:3] + (v_whole,), second + (sw.get_velocity(),)):
        assert torch.equal(a, b)
    assert not torch.equal(first[1], second[1])  # the carried buffer is not modified
    # rows 0-3 and 4-5 with row_base
    lo = sw.switch(lam, init_pos=x0[:4], init_velocity=v0[:4], record_every=2, **kw)
    hi = sw.switch(lam, init_pos=x0[4:], init_velocity=v0[4:], record_every=2, row_base=4, **kw)
    for a, l, h in zip(whole, lo, hi):
        assert torch.equal(a, torch.cat((l, h), dim=0 if a.shape[0] == 6 else 1))


def test_the_instantaneous_switch_is_the_energy_difference():
    A, B, x0 = _pair(5)
    sw = systems.Switch(A, B, kT=0.8)
    sw.set_velocity(None)
    _, w, _ = sw.switch([0.0, 1.0], nsteps=1, init_pos=x0)
    u_a, u_b = sw.energies(x0)
    assert torch.equal(u_a, A.potential(x0.reshape(6, -1))) and torch.equal(u_b, B.potential(x0))
    assert torch.equal(w, u_b * (1.0 / 0.8) - u_a)  # the work multiplies by 1 / kT, as the kernel does
    assert torch.equal(sw.potential(x0, 0.25), 0.75 * u_a + 0.25 * (u_b / 0.8))
    x, w0, en = sw.switch([0.0, 1.0], nsteps=0, init_pos=x0)
    assert torch.equal(x, x0) and not w0.any() and torch.equal(en, torch.stack((u_a, u_b), -1))


def _einstein_pair(natoms=4, seed=0):
    g = torch.Generator().manual_seed(seed)
    c = torch.rand(natoms, 3, generator=g, dtype=F64)
    A = systems.EinsteinCrystal(c, 3, alpha=50)
    B = systems.EinsteinCrystal(c + 0.05, 3, alpha=200)
    A.centers, B.centers = c, c + 0.05
    return A, B


DT_EXACT = 0.005  # the dt of the exact-answer runs (the default; no visible bias at this value)


def _bar_and_std(w_f, w_r, seed):
    est = bar.bar_solve(w_f, w_r)[0][0, 0]
    boot = bar.bootstrap(w_f, w_r, 200, generator=torch.Generator().manual_seed(seed))[:, 0]
    return float(est), float(boot.std())


def test_einstein_to_einstein_gives_zero():
    """Both ends are normalised, so the reduced free-energy difference is 0.  256
    rows each way, 100 steps, fp64, fixed seeds; |BAR| within 4 bootstrap standard
    deviations of 0, and a smaller standard deviation than the nsteps = 1 estimator
    has on the same starting samples."""
    A, B = _einstein_pair()
    torch.manual_seed(123)
    xa, xb = A.sample(256).double(), B.sample(256).double()
    res = {}
    for nsteps in (1, 100):
        w = []
        for (x0, lam, seed) in ((xa, torch.linspace(0, 1, nsteps + 1), 3), (xb, torch.linspace(1, 0, nsteps + 1), 4)):
            sw = systems.Switch(A, B, kT=1.0)
            sw.set_velocity(None)
            w.append(sw.switch(lam, init_pos=x0, dt=DT_EXACT, seed=seed)[1])
        res[nsteps] = _bar_and_std(w[0], w[1], 9)
        print("Einstein to Einstein, %d steps (dt %g): BAR %.4f +- %.4f, mean dissipation %.3f"
              % (nsteps, DT_EXACT, res[nsteps][0], res[nsteps][1], float(w[0].mean() + w[1].mean())))
    est, sd = res[100]
    assert abs(est) <= 4 * sd, res
    assert sd < res[1][1], res


def _cfg(natoms, kT=1.0):
    cfg = app.get_cfg_defaults()
    cfg.device = "cpu"
    cfg.dataset.nparticles, cfg.dataset.dim, cfg.dataset.kT = natoms, 3, kT
    return cfg


def test_switching_work_sign_and_shape():
    A, B = _einstein_pair()
    cfg = _cfg(4)
    torch.manual_seed(5)
    w_f = app.switching_work(cfg, A, B, 16, 1)
    torch.manual_seed(5)
    x = A.sample(16)
    assert w_f.dtype == F64 and w_f.shape == (16,)
    torch.testing.assert_close(w_f, (B.potential(x) - A.potential(x)).double(), rtol=0, atol=1e-12)
    x1 = B.sample(16)
    w_r = app.switching_work(cfg, A, B, 16, 1, direction="reverse", x0=x1)
    torch.testing.assert_close(w_r, (A.potential(x1) - B.potential(x1)).double(), rtol=0, atol=1e-12)
    # equilibration at constant lambda adds no work of its own
    w_e = app.switching_work(cfg, A, B, 16, 5, equil=3, schedule=[0, 0.1, 0.2, 0.5, 0.9, 1.0])
    assert w_e.shape == (16,) and torch.isfinite(w_e).all()


def test_fe_switching_and_fe_stratified_agree_on_the_exact_case():
    """The tuple layout of fe_estimates, and two routes to the same (zero)
    difference: BAR over 256 + 256 switching trajectories of 100 steps, MBAR over
    three constant-lambda strata.  They agree within 4 combined standard
    deviations (the margin of the exact-answer test: fixed seeds, and the strata's
    asymptotic error takes correlated frames for independent ones, which the
    stride of 25 steps at gamma = 10, dt = 0.005 -- 1.25 damping times -- keeps
    mild)."""
    A, B = _einstein_pair()
    cfg = _cfg(4)
    torch.manual_seed(17)
    three = app.fe_switching(cfg, A, B, 256, 100, seed=2)
    assert len(three) == 3 and all(t.dtype == F64 and t.dim() == 0 for t in three)
    torch.manual_seed(17)
    six = app.fe_switching(cfg, A, B, 256, 100, nboot=100, generator=torch.Generator().manual_seed(1), seed=2)
    assert len(six) == 6 and all(t.dtype == F64 and t.dim() == 0 for t in six)
    for a, b in zip(three, six[:3]):
        assert torch.equal(a, b)
    bar_est, bar_err = float(six[0]), float(six[3])
    torch.manual_seed(18)
    strat, strat_err = app.fe_stratified(cfg, A, B, [0.0, 0.5, 1.0], 256, 50, 25, chains=64, seed=6)
    assert strat.dtype == F64 and strat.dim() == 0 and strat_err.dim() == 0
    comb = math.hypot(bar_err, float(strat_err))
    print("fe_switching %.5f +- %.5f, fe_stratified %.5f +- %.5f (per particle, kT = 1)"
          % (bar_est, bar_err, float(strat), float(strat_err)))
    assert abs(bar_est - float(strat)) <= 4 * comb
    assert abs(float(strat)) <= 4 * float(strat_err) and abs(bar_est) <= 4 * bar_err


def test_argument_errors():
    A, B = _einstein_pair()
    cfg = _cfg(4)
    sw = systems.Switch(A, B)
    x = A.sample(3).double()
    with pytest.raises(ValueError, match="schedule is too short"):
        sw.switch([0.0, 0.5, 1.0], nsteps=3, init_pos=x)
    with pytest.raises(ValueError, match="schedule is too short"):
        sw.switch([0.0, 0.5, 1.0], nsteps=1, step0=2, init_pos=x)
    with pytest.raises(ValueError, match="too short"):
        app.switching_work(cfg, A, B, 4, 5, schedule=[0.0, 0.5, 1.0])
    with pytest.raises(ValueError, match="K <= 8"):
        app.fe_stratified(cfg, A, B, np.linspace(0, 1, 9), 8, 1, 1)
    with pytest.raises(ValueError, match="K <= 8"):
        app.fe_stratified(cfg, A, B, [0.5], 8, 1, 1)
    lj = systems.LJ(boxlength=10.0, cutoff=2.5)
    with pytest.raises(ValueError, match="normalised"):
        app.fe_switching(cfg, lj, B, 4, 2)
    with pytest.raises(ValueError, match="coordinates"):
        app.switching_work(_cfg(5), A, B, 4, 2)
    five = systems.EinsteinCrystal(torch.zeros(5, 3), 3, alpha=50)
    with pytest.raises(ValueError, match="coordinates"):
        systems.Switch(five, B).switch([0.0, 1.0], init_pos=x)
    with pytest.raises(ValueError, match="direction"):
        app.switching_work(cfg, A, B, 4, 2, direction="sideways")
    with pytest.raises(ValueError, match="kT"):
        systems.Switch(A, B, kT=0.0)
