"""CPU checks of the dynamics layer: ``integration_step`` of
normalizingflow_amd.systems on its per-step torch path against the
reference's ``dyn_*`` golden vectors, the two integration schemes, shapes,
``nf.hmc.HMC`` and the batched application functions (collect_hmc_data,
integrate_out_v, relaxation_step) against per-frame loops written here.
"""
import math

import pytest
import torch

import golden_io as gio
from normalizingflow_amd import app, systems
from nf.hmc import HMC

RTOL, ATOL = 1e-5, 1e-4
L32 = 2.92402
TRAJ = [n for n in gio.names("dyn_") if gio.load(n)[0]["kind"] in ("einstein", "gmix")]


def build(meta, data, dtype=torch.float32):
    if meta["kind"] == "einstein":
        obj = systems.EinsteinCrystal(data["centers"], meta["dim"], boxlength=meta["boxlength"],
                                      alpha=meta["alpha"])
    else:
        obj = systems.GaussianMixture(meta["centers"], meta["vars"], meta["npart"], meta["dim"])
        obj.vars = obj.vars.to(dtype)
    obj.centers = obj.centers.to(dtype)
    return obj


def lj_f64(pos, L=L32, sigma=1.0, epsilon=1.0, cutoff=1.6, shift=True):
    """LJ.potential (systems.py:166-189) restated in the input's dtype; also returns
    the wrapped pair components and distances."""
    pd = pos.unsqueeze(-2) - pos.unsqueeze(-3)
    raw = pd
    pd = pd - (torch.abs(pd) > 0.5 * L) * torch.sign(pd) * L
    d = torch.linalg.norm(pd, axis=-1)
    inv = 1 / (d + (d == 0))
    if cutoff is not None:
        inv = inv - (d > cutoff) * inv
    p6 = torch.pow(sigma * inv, 6)
    u = torch.pow(p6, 2) - p6
    if cutoff is not None and shift:
        s6 = (sigma / cutoff) ** 6
        u = u - s6 ** 2 + s6
    u = epsilon * 4 * u * inv * d
    return torch.sum(u, axis=(-1, -2)) / 2, raw, d


def lj_force64(pos, **kw):
    with torch.enable_grad():
        x = pos.detach().requires_grad_()
        u = lj_f64(x, **kw)[0]
        return -torch.autograd.grad(u.sum(), x)[0]


def lj_integrate64(x, v, steps, dt, scheme, watch=None, **kw):
    """The header's scheme in the input's dtype (fp64 here): (x, v, potential)."""
    G = lj_force64(x, **kw)
    for _ in range(steps):
        xn = (x + v * dt) + (G * 0.5) * dt ** 2
        Gn = lj_force64(xn if scheme == "verlet" else x, **kw)
        v = v + (dt * (G + Gn)) * 0.5
        x, G = xn, Gn
        if watch is not None:
            watch(x)
    return x, v, lj_f64(x, **kw)[0].detach()


_STATE = {}


def fcc32_state(rows=16, seed=5, steps=50, dt=0.002, cutoff=1.6):
    """The reversal test's inputs: an fcc lattice of 32 in L32 plus 0.03 noise, v ~ N(0, 2).
    The force jumps where a pair crosses the cutoff or a pair component crosses L/2, and a
    pair that a step leaves within rounding of either may fall on the other side on the way
    back; that is a tie of the inputs, not an error of the integrator.  As the fixture
    generators do, the rows are chosen free of ties: of 512 candidates the first
    16 (``rows`` of them are returned) whose fp64 runs (both schemes) keep every pair 5e-6 away from both at every step (the
    fp32 path stays within 1e-6 of fp64 in x over these steps, a pair vector within 2e-6)."""
    key = (seed, steps, dt, cutoff)
    if key not in _STATE:
        basis = [(0, 0, 0), (.5, .5, 0), (.5, 0, .5), (0, .5, .5)]
        pts = [((i + b[0]) / 2, (j + b[1]) / 2, (k + b[2]) / 2)
               for i in range(2) for j in range(2) for k in range(2) for b in basis]
        lat = (torch.tensor(pts, dtype=torch.float64) * L32 - L32 / 2 + L32 / 8).float()
        assert rows <= 16
        g = torch.Generator().manual_seed(seed)
        x = lat + 0.03 * torch.randn(512, 32, 3, generator=g)
        v = math.sqrt(2.0) * torch.randn(512, 32, 3, generator=g)
        tie = torch.zeros(512, dtype=torch.bool)

        def watch(pos):
            _, raw, d = lj_f64(pos, cutoff=cutoff)
            bad = ((raw.abs() - 0.5 * L32).abs() <= 5e-6).any(-1)
            if cutoff is not None:
                bad |= (d - cutoff).abs() <= 5e-6
            tie.__ior__(bad.any(-1).any(-1))

        watch(x.double())
        for scheme in ("verlet", "reference"):
            lj_integrate64(x.double(), v.double(), steps, dt, scheme, watch, cutoff=cutoff)
        keep = (~tie).nonzero().flatten()[:16]
        assert len(keep) == 16, "too few tie-free rows"
        _STATE[key] = (x[keep].contiguous(), v[keep].contiguous())
    x, v = _STATE[key]
    return x[:rows].clone(), v[:rows].clone()


def test_fixture_set():
    assert len(TRAJ) == 4 and "dyn_hmc_vdist" in gio.names("dyn_")
    for n in TRAJ:
        meta, data, _ = gio.load(n)
        assert data["x0"].shape[0] == 37 and meta["paths"] == [1, 12] and meta["dt"] == 0.005


@pytest.mark.parametrize("path_len", [1, 12])
@pytest.mark.parametrize("name", TRAJ)
def test_torch_path_matches_reference(name, path_len):
    meta, data, _ = gio.load(name)
    sim = build(meta, data)
    pos, pot = sim.integration_step(path_len, meta["dt"], data["x0"].clone(), data["v0"].clone())
    assert pos.shape == data["x0"].shape and pot.shape == (37,) and not pos.requires_grad
    for ours, key in ((pos, "x"), (sim.get_velocity(), "v"), (pot, "pot")):
        torch.testing.assert_close(ours, data["%s%d" % (key, path_len)], rtol=RTOL, atol=ATOL)
    # the reference's own call shape: one flattened vector for the whole batch
    pos1, pot1 = sim.integration_step(path_len, meta["dt"], data["x0"].flatten(), data["v0"].flatten())
    assert pos1.shape == (data["x0"].numel(),)
    assert torch.equal(pos1, pos.flatten()) and torch.equal(pot1, pot)


@pytest.mark.parametrize("path_len", [1, 12])
@pytest.mark.parametrize("name", TRAJ)
def test_torch_path_in_double(name, path_len):
    meta, data, _ = gio.load(name)
    sim = build(meta, data, torch.float64)
    pos, pot = sim.integration_step(path_len, meta["dt"], data["x0"].double(), data["v0"].double())
    assert pos.dtype == torch.float64
    for ours, key in ((pos, "x"), (sim.velocity, "v"), (pot, "pot")):
        torch.testing.assert_close(ours, data["%s%d_64" % (key, path_len)], rtol=1e-10, atol=1e-10)


def test_verlet_is_reversible_on_lj_and_the_lagged_scheme_is_not():
    lj = systems.LJ(boxlength=L32, cutoff=1.6)
    x0, v0 = fcc32_state()
    miss = {}
    for scheme in ("verlet", "reference"):
        x1, _ = lj.integration_step(50, 0.002, x0, v0, scheme=scheme)
        x2, _ = lj.integration_step(50, 0.002, x1, -lj.get_velocity(), scheme=scheme)
        miss[scheme] = (float((x2 - x0).abs().max()), float((-lj.get_velocity() - v0).abs().max()))
    print("reversal miss (x, v):", miss)
    assert miss["verlet"][0] <= 1e-4 and miss["verlet"][1] <= 1e-3
    assert miss["reference"][0] > 1e-2


def test_schemes_differ_after_12_steps():
    meta, data, _ = gio.load("dyn_gmix_m2_20x2")
    sim = build(meta, data)
    a, _ = sim.integration_step(12, 0.005, data["x0"], data["v0"])
    b, _ = sim.integration_step(12, 0.005, data["x0"], data["v0"], scheme="verlet")
    assert float((a - b).abs().max()) > 1e-4
    with pytest.raises(ValueError):
        sim.integration_step(1, 0.005, data["x0"], data["v0"], scheme="leapfrog")


def test_shapes_state_and_force_method():
    meta, data, _ = gio.load("dyn_gmix_m3_5x3")
    sim = build(meta, data)
    x0, v0 = data["x0"], data["v0"]
    one, pot1 = sim.integration_step(3, None, x0[4], v0[4])          # 1-D, dt=None -> 0.005
    many, pot = sim.integration_step(3, 0.005, x0, v0)               # [B, W]
    assert one.shape == (15,) and pot1.shape == (1,) and many.shape == (37, 15) and pot.shape == (37,)
    torch.testing.assert_close(one, many[4], rtol=0, atol=0)
    assert sim.get_position() is many and sim.get_velocity().shape == (37, 15)
    assert sim.last_force.shape == (37, 15)
    torch.testing.assert_close(sim.get_potential(), pot, rtol=0, atol=0)
    torch.testing.assert_close(sim.get_potential(x0), sim.potential(x0), rtol=0, atol=0)
    # the reference's `self.force = ...` would have replaced the method by a tensor
    assert callable(sim.force) and sim.force(x0.clone()).shape == (37, 15)
    # LJ keeps [..., n, dim]
    lj = systems.LJ(boxlength=L32, cutoff=1.6)
    x, v = fcc32_state(rows=3)
    p, u = lj.integration_step(2, 0.002, x, v)
    assert p.shape == (3, 32, 3) and u.shape == (3,) and lj.nparticles == 32
    p1, u1 = lj.integration_step(2, 0.002, x[1], v[1])
    assert p1.shape == (32, 3) and u1.shape == ()
    torch.testing.assert_close(p1, p[1], rtol=0, atol=0)
    with pytest.raises(ValueError):
        lj.integration_step(1, 0.002, x.flatten(), v.flatten())  # no particle count to split by
    ein = systems.EinsteinCrystal(torch.zeros(4, 3), 3, alpha=600)
    assert ein.nparticles == 4


@pytest.mark.parametrize("scheme", ["reference", "verlet"])
def test_path_len_zero(scheme):
    meta, data, _ = gio.load("dyn_einstein_5x2_nobox_a600")
    sim = build(meta, data)
    pos, pot = sim.integration_step(0, 0.005, data["x0"], data["v0"], scheme=scheme)
    assert torch.equal(pos, data["x0"]) and torch.equal(sim.velocity, data["v0"])
    torch.testing.assert_close(pot, sim.potential(data["x0"]), rtol=0, atol=0)
    with pytest.raises(ValueError):
        sim.integration_step(-1, 0.005, data["x0"], data["v0"])


def test_velocity_log_prob_matches_reference():
    meta, data, _ = gio.load("dyn_hmc_vdist")
    sim = systems.EinsteinCrystal(torch.zeros(meta["nparticles"], meta["dim"]), meta["dim"], alpha=600)
    run = HMC(sim, beta=meta["beta"], mass=torch.tensor(meta["mass"]), dim=meta["dim"],
              init_beta=meta["init_beta"])
    torch.testing.assert_close(run.log_prob(data["v"]), data["log_prob"], rtol=1e-5, atol=1e-3)
    torch.testing.assert_close(run.log_prob(data["v"].double()), data["log_prob_64"], rtol=1e-10, atol=1e-8)
    torch.testing.assert_close(run.v_dist.log_prob(data["v"]), data["log_prob"], rtol=1e-5, atol=1e-3)
    sim.set_position(torch.zeros(500, 96))
    v, lp = run.generate_v()
    assert v.shape == (500, 96) and lp.shape == (500,)
    std = math.sqrt(1 / (meta["mass"][0] * meta["init_beta"]))
    assert abs(float(v.std()) / std - 1) < 0.02


def _gmix():
    return systems.GaussianMixture([[-1., -1.], [1., 1.]], [0.1, 0.05], 20, 2)


def test_hmc_reference_call_shape_and_seed():
    sim = _gmix()
    torch.manual_seed(3)
    x0 = sim.sample(6)
    run = HMC(sim, path_len=3, dt=0.01, dim=2)            # no position held yet: accepted
    torch.manual_seed(11)
    pos, pot, lp, acc = run.hmc(5, x0[0])                 # one chain: the reference's shapes
    assert pos.shape == (5, 40) and pot.shape == (5,) and lp.shape == (1,) and isinstance(acc, float)
    assert torch.equal(pos[0], x0[0]) and 0.0 <= acc <= 1.0
    torch.manual_seed(11)
    pos2, pot2, _, acc2 = run.hmc(5, x0[0])
    assert torch.equal(pos, pos2) and torch.equal(pot, pot2) and acc == acc2
    torch.manual_seed(12)
    posc, potc, lpc, accc = run.hmc(5, x0)                # six chains
    assert posc.shape == (5, 6, 40) and potc.shape == (5, 6) and lpc.shape == (6,)
    assert run.naccept.shape == (6,) and run.naccept.dtype == torch.int32
    assert abs(accc - float(run.naccept.sum()) / 30) < 1e-12
    # entry i is the state before move i; a rejected chain repeats its row
    moved = (posc[1:] != posc[:-1]).any(-1)
    assert int(moved.sum()) <= int(run.naccept.sum())
    torch.manual_seed(12)
    fin, ufin, _, acc3 = run.hmc(5, x0, record=False)
    assert fin.shape == (6, 40) and ufin.shape == (6,) and acc3 == accc
    torch.testing.assert_close(ufin, sim.potential(fin), rtol=1e-6, atol=1e-6)
    # the systems the reference reached only through LAMMPS, or not at all
    ein = systems.EinsteinCrystal(torch.zeros(4, 3), 3, alpha=600)
    assert HMC(ein, path_len=2, dt=0.01).hmc(2, ein.sample(1)[0])[0].shape == (2, 12)
    lj = systems.LJ(boxlength=L32, cutoff=1.6)
    assert HMC(lj, path_len=2, dt=1e-3).hmc(2, fcc32_state(rows=1)[0][0])[0].shape == (2, 96)


def test_hamiltonian_needs_unit_mass():
    with pytest.raises(ValueError):
        HMC(_gmix(), mass=torch.tensor([55.845]), hamiltonian=True)


def test_metropolis_step_in_torch():
    run = HMC(_gmix(), dim=2, beta=2.0)
    x_cur, x_new = torch.zeros(4, 40), torch.ones(4, 40)
    u_cur = torch.tensor([1.0, 1.0, 1.0, 1.0])
    u_new = torch.tensor([0.5, 2.0, float("nan"), 1.0])
    r = torch.tensor([0.99, 0.5, 0.0, 0.5])
    nacc = torch.zeros(4, dtype=torch.int32)
    run._accept(x_cur, x_new, u_cur, u_new, None, None, r, nacc)
    assert nacc.tolist() == [1, 0, 0, 1]               # exp(-2) < 0.5; NaN rejects; exp(0) = 1 > 0.5
    assert x_cur[:, 0].tolist() == [1.0, 0.0, 0.0, 1.0] and u_cur.tolist() == [0.5, 1.0, 1.0, 1.0]
    run._accept(x_cur, x_new, u_cur, torch.full((4,), 3.0), torch.full((4,), 5.0), torch.zeros(4),
                torch.full((4,), 0.9), nacc)
    assert nacc.tolist() == [2, 1, 1, 2]               # the kinetic terms outweigh the potential's rise


# ------------------------------------------------------------- application layer
class _Model:
    """Stand-in flow model: a fixed quadratic log-density and a seeded sampler."""

    def __init__(self, width):
        self.w = torch.linspace(0.5, 1.5, width)

    def evaluate(self, x):
        return -(x * x * self.w).sum(1)

    def sample(self, n):
        x = 0.1 * torch.randn(n, len(self.w)) + torch.tensor([-1., -1.] * (len(self.w) // 2))
        return x, self.evaluate(x), x


def _cfg(kT=0.7):
    cfg = app.get_cfg_defaults()
    cfg.device = "cpu"
    cfg.dataset.kT, cfg.dataset.dim, cfg.dataset.nparticles = kT, 2, 20
    return cfg


def test_collect_hmc_data():
    sim, model = _gmix(), _Model(40)
    run = HMC(sim, path_len=2, dt=0.01, dim=2)
    torch.manual_seed(21)
    traj, acc = app.collect_hmc_data(_cfg(), model, run, burnin=3, epochs=8)
    torch.manual_seed(21)
    samples, _, _ = model.sample(1)
    ref, _, _, acc_ref = run.hmc(epochs=8, init_pos=samples.flatten())
    assert traj.shape == (5, 40) and torch.equal(traj, ref[3:]) and acc == acc_ref


def _per_frame_integrate_out_v(model, run, frame, vs):
    traj = []
    for v in vs:                                         # dynamics.py:30-34
        run.simulation.set_position(frame)
        position, _, _ = run.run_sim(v)
        traj.append(position.flatten().float())
    q_nf = model.evaluate(torch.stack(traj))
    return torch.logsumexp(q_nf, 0) - torch.log(torch.tensor(float(len(vs))))


def test_integrate_out_v_equals_per_frame_loop(monkeypatch):
    sim, model = _gmix(), _Model(40)
    run = HMC(sim, path_len=4, dt=0.01, dim=2)
    torch.manual_seed(5)
    frames = sim.sample(7)
    V = 0.3 * torch.randn(7 * 10, 40)
    monkeypatch.setattr(run, "generate_v", lambda: (V, run.log_prob(V)))
    got = app.integrate_out_v(model, run, frames, npoints=10)
    want = torch.stack([_per_frame_integrate_out_v(model, run, frames[i], V[10 * i:10 * i + 10])
                        for i in range(7)])
    assert got.shape == (7,)
    torch.testing.assert_close(got, want, rtol=1e-6, atol=1e-6)
    one = app.integrate_out_v(model, run, frames[0], npoints=70)
    assert one.shape == ()


def test_relaxation_step_equals_per_frame_loop(monkeypatch):
    sim, model, cfg = _gmix(), _Model(40), _cfg()
    torch.manual_seed(6)
    traj = sim.sample(5)
    draws = [0.3 * torch.randn(5, 40), 0.3 * torch.randn(5 * 4, 40)]
    calls = []

    def fake_generate_v(self):
        v = draws[len(calls)]
        calls.append(v)
        return v, self.log_prob(v)

    monkeypatch.setattr(HMC, "generate_v", fake_generate_v)
    new, q_learned, q_fe = app.relaxation_step(cfg, model, sim, traj, path_len=3, npoints=4)
    assert len(calls) == 2 and new.shape == (5, 40) and q_learned.shape == (5,) and q_fe.shape == (5,)
    for i in range(5):                                   # dynamics.py:38-56, one frame at a time
        run = HMC(sim, beta=1 / cfg.dataset.kT, path_len=3, dim=2)
        sim.set_position(traj[i])
        position, potential, _ = run.run_sim(draws[0][i])
        torch.testing.assert_close(new[i], position, rtol=1e-6, atol=1e-6)
        torch.testing.assert_close(q_fe[i], -potential[0] / cfg.dataset.kT, rtol=1e-6, atol=1e-6)
        want = _per_frame_integrate_out_v(model, run, position, draws[1][4 * i:4 * i + 4])
        torch.testing.assert_close(q_learned[i], want, rtol=1e-6, atol=1e-6)
