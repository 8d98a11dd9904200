"""GPU checks of the dynamics layer (nfk_dynamics.hip): whole trajectories of
the Einstein crystal, the Gaussian mixture and Lennard-Jones in one launch
against the reference's ``dyn_*`` golden vectors, bit for bit against the
per-step path of force kernels and torch elementwise ops, and against an fp64
restatement; nfk_hmc_accept against a torch restatement; ``nf.hmc.HMC`` as a
sampler; the batched application functions against per-frame loops.

Parity follows tests/test_gpu_systems.py's close_or_on_par: rtol 1e-5 / atol
1e-4 against the reference's fp32 values, or max and p99 error against the fp64
companion within 2x the reference's own.
"""
import math

import pytest
import torch

import golden_io as gio
import nf.flows as nff
import nf.models as nfm
from nf.hmc import HMC
from normalizingflow_amd import app, systems
from normalizingflow_amd import kernels as K_
from test_dynamics_cpu import L32, TRAJ, fcc32_state, lj_f64, lj_integrate64
from test_gpu_systems import close_or_on_par, counts_of

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
RTOL, ATOL = 1e-5, 1e-4
_CACHE = {}


def fixture(name):
    if name not in _CACHE:
        _CACHE[name] = gio.load(name)[:2]
    return _CACHE[name]


def build(meta, data):
    if meta["kind"] == "einstein":
        return systems.EinsteinCrystal(data["centers"], meta["dim"], boxlength=meta["boxlength"],
                                       alpha=meta["alpha"], device=DEV)
    return systems.GaussianMixture(meta["centers"], meta["vars"], meta["npart"], meta["dim"], device=DEV)


def fused_only(obj, monkeypatch):
    def boom(*a, **k):
        raise AssertionError("the per-step path ran")
    monkeypatch.setattr(obj, "_force_detached", boom)


def _row_index(rows):
    if rows == 37:
        return torch.arange(37)
    if rows == 1:
        return torch.tensor([5])
    g = torch.Generator().manual_seed(rows)
    return (torch.arange(rows) % 37)[torch.randperm(rows, generator=g)]  # tiled, row order shuffled


# ---------------------------------------------------------------- fixture parity
@pytest.mark.parametrize("rows", [1, 37, 500])
@pytest.mark.parametrize("name", TRAJ)
def test_fixture_parity(name, rows, hip_device, monkeypatch):
    meta, data = fixture(name)
    idx = _row_index(rows)
    sim = build(meta, data)
    fused_only(sim, monkeypatch)
    x0, v0 = data["x0"][idx].to(DEV), data["v0"][idx].to(DEV)
    for P in meta["paths"]:
        pos, pot = sim.integration_step(P, meta["dt"], x0, v0)
        assert pos.shape == x0.shape and pot.shape == (rows,) and pos.dtype == torch.float32
        assert not pos.requires_grad and not pot.requires_grad
        for ours, key in ((pos, "x"), (sim.get_velocity(), "v"), (pot, "pot")):
            close_or_on_par(ours, data["%s%d" % (key, P)][idx], data["%s%d_64" % (key, P)][idx],
                            "%s %s%d" % (name, key, P))


# ------------------------------------------------- bitwise against the per-step path
def _sc_state(n, dim, rows, seed, spacing=1.1):
    """n particles on a simple-cubic lattice (the first n sites) plus 0.03 noise; v ~ N(0, 1)."""
    m = math.ceil(n ** (1 / dim) - 1e-9)
    L = spacing * m
    grid = torch.stack(torch.meshgrid(*[torch.arange(m, dtype=torch.float32)] * dim, indexing="ij"), -1)
    lat = grid.reshape(-1, dim)[:n] * spacing - L / 2 + spacing / 2
    g = torch.Generator().manual_seed(seed)
    return (lat + 0.03 * torch.randn(rows, n, dim, generator=g), torch.randn(rows, n, dim, generator=g), L)


def _lj_case(n, dim, cutoff=1.6, shift=True):
    x, v, L = _sc_state(n, dim, 37, 100 + n)
    return systems.LJ(boxlength=L, cutoff=cutoff, shift=shift, device=DEV), x, v, 0.002


def _einstein_case(natoms, dim, box):
    g = torch.Generator().manual_seed(7 + natoms)
    centers = (torch.rand(natoms, dim, generator=g) - 0.5) * L32
    sim = systems.EinsteinCrystal(centers, dim, boxlength=L32 if box else None, alpha=600, device=DEV)
    x = centers.flatten() + torch.randn(37, natoms * dim, generator=g) / math.sqrt(600)
    if box:  # some coordinates one box away: the wrap fires
        x = x + (torch.rand(37, natoms * dim, generator=g) < 0.05) * L32
    return sim, x, torch.randn(37, natoms * dim, generator=g), 0.005


def _gmix_case(centers, vars_, npart, dim):
    sim = systems.GaussianMixture(centers, vars_, npart, dim, device=DEV)
    torch.manual_seed(17)
    x = sim.sample(37).cpu()
    return sim, x, torch.randn(37, npart * dim), 0.005


BITWISE = {
    "lj_n3_d2": lambda: _lj_case(3, 2),
    "lj_n32_d3": lambda: _lj_case(32, 3),
    "lj_n33_ragged": lambda: _lj_case(33, 3),
    "lj_n100_two_per_lane": lambda: _lj_case(100, 3),
    "lj_n32_noshift": lambda: _lj_case(32, 3, shift=False),
    "lj_n32_nocut": lambda: _lj_case(32, 3, cutoff=None),
    "einstein_5x2_nobox": lambda: _einstein_case(5, 2, False),
    "einstein_32x3_box": lambda: _einstein_case(32, 3, True),
    "gmix_m1": lambda: _gmix_case([[-0.5, -0.5]], 0.25, 20, 2),
    "gmix_m3_d3": lambda: _gmix_case([[-1., 0., 1.], [1., 1., 0.], [0., -1., -1.]], [0.1, 0.05, 0.2], 7, 3),
}


@pytest.mark.parametrize("scheme", ["reference", "verlet"])
@pytest.mark.parametrize("case", sorted(BITWISE))
def test_fused_equals_per_step_bitwise(case, scheme, hip_device):
    sim, x, v, dt = BITWISE[case]()
    for rows in (1, 37):
        x0, v0 = x[:rows].to(DEV), v[:rows].to(DEV)
        for P in (0, 1, 12, 50):
            sim.fused_dynamics = True
            n = counts_of(lambda: sim.integration_step(P, dt, x0, v0, scheme=scheme))
            xf, vf = sim.get_position(), sim.get_velocity()
            pot = sim.get_potential()  # potential(x_out) by the energy kernel
            xf2, potf = sim.integration_step(P, dt, x0, v0, scheme=scheme)
            ff = sim.last_force
            sim.fused_dynamics = False
            xs, _ = sim.integration_step(P, dt, x0, v0, scheme=scheme)
            vs, fs = sim.get_velocity(), sim.last_force
            what = "%s %s rows %d path_len %d" % (case, scheme, rows, P)
            assert torch.isfinite(xs).all() and torch.isfinite(vs).all(), what
            assert [k for k in n if k.endswith("_trajectory")] == list(n) and sum(n.values()) == 1, (what, n)
            assert torch.equal(xf, xs) and torch.equal(vf, vs) and torch.equal(xf2, xf), what
            assert torch.equal(ff, fs), what
            assert xf.shape == x0.shape and vf.shape == x0.shape
            torch.testing.assert_close(potf, pot, rtol=RTOL, atol=ATOL, msg=what)


# ------------------------------------------------------------------ fp64 restatement
@pytest.mark.parametrize("scheme", ["reference", "verlet"])
@pytest.mark.parametrize("path_len", [12, 50])
def test_lj_against_fp64_restatement(path_len, scheme, hip_device, monkeypatch):
    """x and v of the fused launch against the fp64 trajectory.  The potential is not
    compared with the fp64 trajectory's: it is taken at OUR x_out, and dU = F . dx turns an
    x error inside the tolerance (7e-7 measured) into 2.5e-4 of energy at forces of ~70.
    Its own check is test_fused_equals_per_step_bitwise's, against potential(x_out); here
    it is compared with the fp64 energy of our x_out by the on-par rule of the energy
    kernel's own fixtures (tests/test_gpu_systems.py), the fp32 torch energy as reference."""
    x0, v0 = fcc32_state()
    lj = systems.LJ(boxlength=L32, cutoff=1.6, device=DEV)
    fused_only(lj, monkeypatch)
    pos, pot = lj.integration_step(path_len, 0.002, x0.to(DEV), v0.to(DEV), scheme=scheme)
    x64, v64, _ = lj_integrate64(x0.double(), v0.double(), path_len, 0.002, scheme)
    for ours, want, what in ((pos, x64, "x"), (lj.get_velocity(), v64, "v")):
        err = float((ours.cpu().double() - want).abs().max())
        print("%s after %d %s steps: max error against fp64 %.3g" % (what, path_len, scheme, err))
        torch.testing.assert_close(ours.cpu().double(), want, rtol=RTOL, atol=ATOL)
    close_or_on_par(pot, lj_f64(pos.cpu())[0], lj_f64(pos.cpu().double())[0], "potential at x_out")


# ---------------------------------------------------------------------------- layout
def _layouts(t):
    """t [B, W] as a column slice of wider rows and 4 bytes off 16-byte alignment."""
    B, W = t.shape
    wide = torch.zeros(B, W + 3, device=DEV)
    wide[:, :W] = t
    flat = torch.zeros(B * W + 1, device=DEV)
    flat[1:] = t.flatten()
    off = flat[1:].view(B, W)
    assert wide[:, :W].stride(0) == W + 3 and off.data_ptr() % 16 == 4
    return wide[:, :W], off


@pytest.mark.parametrize("kind", ["einstein", "gmix", "lj"])
def test_strided_misaligned_and_aliased(kind, hip_device):
    if kind == "lj":
        sim, x, v, dt = _lj_case(33, 3)
        x, v = x.reshape(37, -1), v.reshape(37, -1)
        launch = lambda *a: K_.lj_trajectory(*a, path_len=12, dt=dt, scheme=1, n=33, dim=3, **sim._kw())  # noqa: E731
    elif kind == "einstein":
        sim, x, v, dt = _einstein_case(32, 3, True)
        scale, hld = sim._consts()
        launch = lambda *a: K_.einstein_trajectory(*a, sim.centers, path_len=12, dt=dt, scheme=1,  # noqa: E731
                                                   scale=scale, hld=hld, boxlength=sim.boxlength)
    else:
        sim, x, v, dt = _gmix_case([[-1., -1.], [1., 1.]], [0.1, 0.05], 20, 2)
        scales, hlds = sim._consts()
        launch = lambda *a: K_.gmix_trajectory(*a, sim.centers, scales, hlds, path_len=12, dt=dt,  # noqa: E731
                                               scheme=1, npart=20)
    x, v = x.to(DEV), v.to(DEV)
    xo, vo, pot = torch.empty_like(x), torch.empty_like(v), torch.empty(37, device=DEV)
    launch(x, v, xo, vo, pot)
    for xa, va in zip(_layouts(x), _layouts(v)):
        W = x.shape[1]  # outputs with their own leading dimension
        xb = torch.full((37, W + 5), float("nan"), device=DEV)[:, :W]
        vb = torch.full((37, W + 1), float("nan"), device=DEV)[:, :W]
        pb = torch.empty(37, device=DEV)
        launch(xa, va, xb, vb, pb)
        assert torch.equal(xb, xo) and torch.equal(vb, vo) and torch.equal(pb, pot)
        pc = torch.empty(37, device=DEV)
        launch(xa, va, xa, va, pc)  # x_out aliases x_in, v_out aliases v_in
        assert torch.equal(xa, xo) and torch.equal(va, vo) and torch.equal(pc, pot)
    with pytest.raises(ValueError):
        launch(x, v, xo, vo[:, :-1], pot)


def test_bad_arguments_never_reach_the_device(hip_device):
    sim, x, v, dt = _lj_case(3, 2)
    x, v = x.reshape(37, -1).to(DEV), v.reshape(37, -1).to(DEV)
    out = torch.empty_like(x), torch.empty_like(v), torch.empty(37, device=DEV)
    for kw in (dict(path_len=-1, scheme=0), dict(path_len=1, scheme=2)):
        with pytest.raises(ValueError):
            K_.lj_trajectory(x, v, *out, dt=dt, n=3, dim=2, **kw, **sim._kw())
    with pytest.raises(ValueError, match="not supported"):
        K_.lj_trajectory(torch.zeros(2, 300 * 3, device=DEV), torch.zeros(2, 300 * 3, device=DEV),
                         torch.zeros(2, 300 * 3, device=DEV), torch.zeros(2, 300 * 3, device=DEV),
                         torch.zeros(2, device=DEV), path_len=1, dt=dt, scheme=0, n=300, dim=3, **sim._kw())
    # an unsupported shape takes the per-step path
    big, L = torch.rand(2, 300, 3, device=DEV) * 8.0, 8.0
    lj = systems.LJ(boxlength=L, cutoff=1.6, device=DEV)
    n = counts_of(lambda: lj.integration_step(1, 1e-4, big, torch.zeros_like(big)))
    assert not any(k.endswith("_trajectory") for k in n)


# ------------------------------------------------------------------- nfk_hmc_accept
@pytest.mark.parametrize("kinetic", [False, True])
@pytest.mark.parametrize("chains,width", [(1, 96), (37, 10), (4096, 12)])
def test_hmc_accept(chains, width, kinetic, hip_device):
    g = torch.Generator().manual_seed(chains + width)
    x_cur, x_new = torch.randn(chains, width, generator=g), torch.randn(chains, width, generator=g)
    u_cur, u_new = torch.randn(chains, generator=g), torch.randn(chains, generator=g)
    k_cur = torch.rand(chains, generator=g) if kinetic else None
    k_new = torch.rand(chains, generator=g) if kinetic else None
    r = torch.rand(chains, generator=g)
    nacc = torch.randint(0, 5, (chains,), generator=g, dtype=torch.int32)
    beta = 1.7
    if chains > 1:
        u_new[3] = float("nan")
    d = u_cur - u_new
    if kinetic:
        d = (d + k_cur) - k_new
    p = torch.exp(d * beta)
    acc = r < p
    judged = ~((r - p).abs() <= 1e-5)  # a NaN probability is judged: it rejects
    assert (~judged).sum() <= 0.01 * chains
    want_x = torch.where(acc.unsqueeze(1), x_new, x_cur)
    want_u = torch.where(acc, u_new, u_cur)
    want_n = nacc + acc.to(torch.int32)
    dev = [None if t is None else t.to(DEV) for t in (x_cur, x_new, u_cur, u_new, r, nacc, k_cur, k_new)]
    K_.hmc_accept(*dev[:6], beta=beta, k_cur=dev[6], k_new=dev[7])
    got_x, got_u, got_n = dev[0].cpu(), dev[2].cpu(), dev[5].cpu()
    took = got_n - nacc
    assert ((took == 0) | (took == 1)).all()
    assert torch.equal(took[judged].bool(), acc[judged])
    if chains > 1:
        assert took[3] == 0
    # whatever a chain decided, its row, potential and count moved together and exactly
    t = took.bool()
    assert torch.equal(got_x, torch.where(t.unsqueeze(1), x_new, x_cur))
    assert torch.equal(got_u[~t], u_cur[~t]) and torch.equal(got_u[t], u_new[t])
    assert torch.equal(got_x[judged], want_x[judged]) and torch.equal(got_n[judged], want_n[judged])
    assert torch.equal(got_u[judged & ~torch.isnan(want_u)], want_u[judged & ~torch.isnan(want_u)])


# ---------------------------------------------------------------------------- sampler
def _einstein_4x3():
    g = torch.Generator().manual_seed(3)
    return systems.EinsteinCrystal((torch.rand(4, 3, generator=g) - 0.5) * 2, 3, alpha=600, device=DEV)


def test_sampler_is_stationary_on_the_einstein_crystal(hip_device, monkeypatch):
    sim = _einstein_4x3()
    fused_only(sim, monkeypatch)
    run = HMC(sim, scheme="verlet", hamiltonian=True, dt=0.02, path_len=8)
    torch.manual_seed(1)
    x0 = sim.sample(4096)
    pos, pot, _, acc = run.hmc(20, x0, record=False)
    dev = pos - sim.centers.flatten()
    var = float(600 * dev.double().var())
    move = float(((pos - x0).double() ** 2).mean().sqrt() * math.sqrt(600))
    print("acceptance %.3f, alpha * variance %.4f, rms move * sqrt(alpha) %.3f" % (acc, var, move))
    assert acc > 0.85
    assert 0.97 <= var <= 1.03
    assert move > 0.5
    torch.testing.assert_close(pot, sim.potential(pos), rtol=RTOL, atol=ATOL)


def test_one_launch_pair_per_epoch_and_seeds_repeat(hip_device):
    sim = systems.GaussianMixture([[-1., -1.], [1., 1.]], [0.1, 0.05], 20, 2, device=DEV)
    torch.manual_seed(2)
    x0 = sim.sample(37)
    run = HMC(sim, path_len=5, dt=0.01, dim=2)
    outs = []
    for _ in range(2):
        torch.manual_seed(9)
        outs.append(run.hmc(6, x0))
    (p1, u1, l1, a1), (p2, u2, l2, a2) = outs
    assert p1.shape == (6, 37, 40) and u1.shape == (6, 37) and p1.is_cuda
    assert torch.equal(p1, p2) and torch.equal(u1, u2) and torch.equal(l1, l2) and a1 == a2
    assert 0 < int(run.naccept.sum()) <= 6 * 37
    n = counts_of(lambda: run.hmc(3, x0, record=False))
    assert n.get("nfk_gmix_trajectory") == 3 and n.get("nfk_hmc_accept") == 3, n
    # the reference's call shape on one chain of each system
    pos, pot, lp, acc = HMC(sim, path_len=2, dt=0.01, dim=2).hmc(3, x0[0])
    assert pos.shape == (3, 40) and pot.shape == (3,) and lp.shape == (1,)
    ein = _einstein_4x3()
    assert HMC(ein, path_len=2, dt=0.01).hmc(3, ein.sample(1)[0])[0].shape == (3, 12)
    lj = systems.LJ(boxlength=L32, cutoff=1.6, device=DEV)
    assert HMC(lj, path_len=2, dt=1e-3).hmc(3, fcc32_state(rows=1)[0][0].to(DEV))[0].shape == (3, 96)


# ------------------------------------------------------------- batched versus per-frame
def test_relaxation_and_integrate_out_v_equal_per_frame_loops(hip_device, monkeypatch):
    sim = _einstein_4x3()
    torch.manual_seed(1234)
    model = nfm.NormalizingFlowModel(sim, [nff.NSF_AR(dim=12, K=8, B=3, hidden_dim=16) for _ in range(2)]).to(DEV)
    cfg = app.get_cfg_defaults()
    cfg.device, cfg.dataset.kT, cfg.dataset.dim, cfg.dataset.nparticles = DEV, 0.7, 3, 4
    torch.manual_seed(4)
    traj = sim.sample(8)
    draws = [0.05 * torch.randn(8, 12, device=DEV), 0.05 * torch.randn(8 * 10, 12, device=DEV)]
    calls = []

    def fake_generate_v(self):
        v = draws[0] if self._like()[2] == 8 else draws[1]
        calls.append(v)
        return v, self.log_prob(v)

    monkeypatch.setattr(HMC, "generate_v", fake_generate_v)
    new, q_learned, q_fe = app.relaxation_step(cfg, model, sim, traj, path_len=12, npoints=10)
    assert new.shape == (8, 12) and q_learned.shape == (8,) and q_fe.shape == (8,) and new.is_cuda
    again = app.integrate_out_v(model, HMC(sim, beta=1 / 0.7, path_len=12), new, npoints=10)
    for i in range(8):  # dynamics.py:38-56 and 26-36, one frame and one velocity at a time
        run = HMC(sim, beta=1 / 0.7, path_len=12)
        sim.set_position(traj[i])
        position, potential, _ = run.run_sim(draws[0][i])
        assert torch.equal(new[i], position)
        torch.testing.assert_close(q_fe[i], -potential[0] / 0.7, rtol=RTOL, atol=ATOL)
        rows = []
        for v in draws[1][10 * i:10 * i + 10]:
            sim.set_position(position)
            rows.append(run.run_sim(v)[0].flatten())
        q_nf = model.evaluate(torch.stack(rows))
        want = torch.logsumexp(q_nf, 0) - math.log(10)
        torch.testing.assert_close(q_learned[i], want, rtol=RTOL, atol=ATOL)
        torch.testing.assert_close(again[i], want, rtol=RTOL, atol=ATOL)
