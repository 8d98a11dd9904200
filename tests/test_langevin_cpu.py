"""CPU checks of ``langevin`` (systems.py), the per-step path: the noise is keyed
by (seed, absolute step, particle, row), so runs repeat, chunks and row blocks
join exactly, and records are the states a shorter run stops at."""
import math

import pytest
import torch

import eam_tables as et
from normalizingflow_amd import app, rng, systems

DT = 0.002


def lj_state(rows=3, n=8, seed=3, dtype=torch.float32):
    """n = 8 particles on a 2 x 2 x 2 simple-cubic lattice of spacing 1.1 plus 0.03 noise."""
    g = torch.Generator().manual_seed(seed)
    grid = torch.stack(torch.meshgrid(*[torch.arange(2, dtype=torch.float64)] * 3, indexing="ij"), -1)
    lat = grid.reshape(-1, 3)[:n] * 1.1 - 0.55
    x = lat + 0.03 * torch.randn(rows, n, 3, generator=g, dtype=torch.float64)
    return systems.LJ(boxlength=2.2, cutoff=1.05), x.to(dtype)


def einstein_state(rows=4, natoms=5, dim=3):
    g = torch.Generator().manual_seed(11)
    centers = torch.rand(natoms, dim, generator=g) - 0.5
    sim = systems.EinsteinCrystal(centers, dim, boxlength=None, alpha=50)
    return sim, centers.flatten() + 0.1 * torch.randn(rows, natoms * dim, generator=g)


def run(sim, x, nsteps, v=None, **kw):
    sim.set_velocity(v)
    out = sim.langevin(nsteps, dt=DT, init_pos=x, **kw)
    return out, sim.get_velocity()


@pytest.mark.parametrize("make", [lj_state, einstein_state])
def test_reproducible_by_seed(make):
    sim, x = make()
    (xc, _), _ = run(sim, x, 5, seed=8)
    (xa, pa), va = run(sim, x, 5, seed=7)
    (xb, pb), vb = run(sim, x, 5, seed=7)
    assert torch.equal(xa, xb) and torch.equal(va, vb) and torch.equal(pa, pb)
    assert not torch.equal(xa, xc)
    assert xa.shape == x.shape and va.shape == x.shape and pa.shape == (x.shape[0],)
    assert torch.isfinite(xa).all() and not xa.requires_grad and not pa.requires_grad
    assert torch.equal(sim.get_position(), xa)
    assert torch.allclose(pa, sim.potential(xa).reshape(-1))


@pytest.mark.parametrize("make", [lj_state, einstein_state])
def test_chunks_join_exactly(make):
    sim, x = make()
    (x11, p11), v11 = run(sim, x, 11, seed=5)
    (x4, _), v4 = run(sim, x, 4, seed=5)
    sim.set_velocity(v4)
    x7, p7 = sim.langevin(7, dt=DT, init_pos=x4, seed=5, step0=4)
    assert torch.equal(x7, x11) and torch.equal(sim.get_velocity(), v11) and torch.equal(p7, p11)


@pytest.mark.parametrize("make", [lj_state, einstein_state])
def test_a_row_alone_with_its_row_base(make):
    sim, x = make()
    (xa, pa), va = run(sim, x, 6, seed=2, row_base=10)
    for r in range(x.shape[0]):
        (xr, pr), vr = run(sim, x[r:r + 1], 6, seed=2, row_base=10 + r)
        assert torch.equal(xr[0], xa[r]) and torch.equal(vr[0], va[r]) and torch.equal(pr[0], pa[r])


def test_records_are_the_states_a_shorter_run_stops_at():
    sim, x = lj_state()
    (xe, pe, frames, pots), _ = run(sim, x, 10, seed=4, record_every=3)
    assert frames.shape == (3,) + x.shape and pots.shape == (3, x.shape[0])
    for i, stop in enumerate((3, 6, 9)):
        (xs, ps), _ = run(sim, x, stop, seed=4)
        assert torch.equal(frames[i], xs) and torch.equal(pots[i], ps)
    (x10, p10), _ = run(sim, x, 10, seed=4)
    assert torch.equal(xe, x10) and torch.equal(pe, p10)
    (_, _, none, nopots), _ = run(sim, x, 2, seed=4, record_every=3)
    assert none.shape == (0,) + x.shape and nopots.shape == (0, x.shape[0])


def test_zero_momentum_keeps_the_total_momentum():
    sim, x = lj_state(dtype=torch.float64)
    (_, _), v = run(sim, x, 40, seed=1, kT=1.0)
    assert float(v.abs().max()) > 0.1
    assert float(v.sum(1).abs().max()) < 1e-12  # the drawn velocities and every kick sum to zero
    (_, _), vf = run(sim, x, 40, seed=1, kT=1.0, zero_momentum=False)
    assert float(vf.sum(1).abs().max()) > 1e-3
    sim32, x32 = lj_state()
    (_, _), v32 = run(sim32, x32, 40, seed=1)
    assert float(v32.sum(1).abs().max()) < 40 * 8 * 1e-6
    # the defaults: momentum-free for the particle systems, plain for the priors
    assert systems.LJ._zero_momentum_default and systems.EAM._zero_momentum_default
    assert not systems.EinsteinCrystal._zero_momentum_default
    assert not systems.GaussianMixture._zero_momentum_default


def test_the_steps_are_baoab_on_the_noise_of_rng():
    sim, x = einstein_state()
    x = x.double()
    sim.centers = sim.centers.double()
    gamma, kT, mass, seed = 10.0, 0.7, 2.0, 9
    v0 = torch.randn(x.shape, generator=torch.Generator().manual_seed(1), dtype=torch.float64)
    (xo, _), vo = run(sim, x, 3, v=v0, gamma=gamma, kT=kT, mass=mass, seed=seed, step0=5, row_base=2)
    c1 = math.exp(-gamma * DT)
    c2 = math.sqrt(kT / mass * (1 - c1 * c1))
    xs, vs = x.clone(), v0.clone()
    force = lambda y: -50 * (y - sim.centers.flatten())  # noqa: E731
    for k in range(3):
        xi = rng.philox_normal(seed, x.shape[0], 5, 3, 5 + k, row_base=2, dtype=torch.float64).reshape(x.shape)
        vs = vs + 0.5 * DT / mass * force(xs)
        xs = xs + 0.5 * DT * vs
        vs = c1 * vs + c2 * xi
        xs = xs + 0.5 * DT * vs
        vs = vs + 0.5 * DT / mass * force(xs)
    torch.testing.assert_close(xo, xs, rtol=1e-12, atol=1e-12)
    torch.testing.assert_close(vo, vs, rtol=1e-12, atol=1e-12)


def test_bad_arguments():
    sim, x = lj_state()
    sim.set_position(x)
    for kw in (dict(nsteps=-1), dict(nsteps=1, record_every=-1), dict(nsteps=1, step0=-1), dict(nsteps=1, dt=0.0),
               dict(nsteps=1, seed=1 << 63)):
        sim.set_velocity(None)
        with pytest.raises(ValueError):
            sim.langevin(**kw)


def test_sample_md(tmp_path):
    cfg, _, frames = et.fe_config(tmp_path)
    potential = app.build_potential(cfg)
    out = app.sample_md(cfg, potential, 5, chains=2, burnin=3, stride=2, dt=0.01, seed=3)
    assert out.shape == (5, 16, 3) and out.dtype == torch.float32 and torch.isfinite(out).all()
    again = app.sample_md(cfg, potential, 5, chains=2, burnin=3, stride=2, dt=0.01, seed=3)
    assert torch.equal(out, again)
    centers = torch.tensor(cfg.prior.centers)
    assert 0 < float((out - centers).abs().max()) < 0.5  # cold iron stays on its lattice
    potential.update_data(out)
    assert potential.sample(4).shape == (4, 48) and potential.sample(3, flatten=False).shape == (3, 16, 3)
    potential.update_data(out[:2], append=True)
    assert len(potential.traj) == 7
    cfg.prior.type = "Normal"
    with pytest.raises(ValueError, match="x0"):
        app.sample_md(cfg, potential, 2)
    given = app.sample_md(cfg, potential, 2, x0=centers, chains=1, burnin=0, stride=1, dt=0.01)
    assert given.shape == (2, 16, 3)
