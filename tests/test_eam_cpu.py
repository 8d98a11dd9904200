"""CPU checks of systems.EAM's plain-torch path and of read_setfl: closed forms
on cubic-polynomial tables (on which the piecewise-cubic interpolant is exact
away from the first and last two intervals), invariances, an orthorhombic box
against a brute-force image scan, the Fe-style config path, and the per-step
dynamics and HMC on the EAM force."""
import itertools

import numpy as np
import pytest
import torch

import eam_tables as et
import nf.hmc
from normalizingflow_amd import app, systems

F64 = torch.float64
REL = 1e-10


def rel_err(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-300))


def brute(pos, box, rc, S=3):
    """U and dU/dx of the cubic-polynomial model by a scan over the shifts
    -S..S per axis of the unwrapped pair vectors (fp64 numpy).  Also returns
    the counted distances and the densities."""
    pos, box = np.asarray(pos, dtype=np.float64), np.asarray(box, dtype=np.float64)
    n = len(pos)
    rho, pair, dists = np.zeros(n), 0.0, []
    terms = []
    for s in itertools.product(range(-S, S + 1), repeat=3):
        d = pos[:, None, :] - pos[None, :, :] + np.asarray(s) * box
        r = np.sqrt((d * d).sum(-1))
        ok = (r > 0) & (r <= rc)
        i, j = np.nonzero(ok)
        if len(i):
            terms.append((i, j, d[ok], r[ok]))
    for i, j, d, r in terms:
        np.add.at(rho, i, et.poly(et.CUBIC_f, r))
        pair += (et.poly(et.CUBIC_z, r) / r).sum()
        dists.append(r)
    U = et.poly(et.CUBIC_F, rho).sum() + 0.5 * pair
    dF = et.dpoly(et.CUBIC_F, rho)
    grad = np.zeros((n, 3))
    for i, j, d, r in terms:
        phi = et.poly(et.CUBIC_z, r) / r
        dphi = (et.dpoly(et.CUBIC_z, r) - phi) / r
        w = (dphi + (dF[i] + dF[j]) * et.dpoly(et.CUBIC_f, r)) / r
        np.add.at(grad, i, w[:, None] * d)
    return U, grad, np.concatenate(dists) if dists else np.zeros(0), rho


def interior(tab, dists, rho):
    """Every counted distance and density between node 2 and node n - 3."""
    return (len(dists) > 0 and dists.min() >= 2 * tab["dr"] and dists.max() <= (tab["nr"] - 3) * tab["dr"]
            and rho.min() >= 2 * tab["drho"] and rho.max() <= (tab["nrho"] - 3) * tab["drho"])


def config(tab, box, n, seed):
    """n atoms in the box, redrawn until the cubic tables are exact on them: no
    distance (over all images) within 1e-4 rc above rc or in the last two
    intervals below it, nor in the first two; the same for the densities."""
    rng = np.random.default_rng(seed)
    box = np.asarray(box, dtype=np.float64)
    for _ in range(2000):
        pos = rng.random((n, 3)) * box
        wide = image_distances(pos, box, tab["rc"] * (1 + 1e-4))
        U, grad, dists, rho = brute(pos, box, tab["rc"])
        if len(wide) == len(dists) and interior(tab, dists, rho):
            return pos, U, grad
    raise AssertionError("no admissible configuration found")


def image_distances(pos, box, rc):
    """Every distance 0 < r <= rc over the shifts -3..3."""
    d = [pos[:, None, :] - pos[None, :, :] + np.asarray(s) * box for s in itertools.product(range(-3, 4), repeat=3)]
    r = np.sqrt((np.stack(d) ** 2).sum(-1))
    return r[(r > 0) & (r <= rc)]


def energy_and_grad(eam, pos, dtype=F64):
    x = torch.as_tensor(pos, dtype=dtype).clone().requires_grad_()
    u = eam.potential(x)
    g, = torch.autograd.grad(u.sum(), x)
    return u.detach(), g


# ---------------------------------------------------------------------------
@pytest.mark.parametrize("per_line", [5, 1])
def test_read_setfl_round_trip(tmp_path, per_line):
    tab = et.fs(nr=57, nrho=43)
    got = systems.read_setfl(et.write_setfl(tmp_path / "t.eam.alloy", tab, per_line=per_line))
    assert (got["nrho"], got["nr"], got["element"]) == (43, 57, "Xx")
    assert got["element_line"] == tab["element_line"]
    for k in ("drho", "dr", "rc"):
        assert got[k] == tab[k]
    for k in ("F", "f", "z"):
        assert got[k].dtype == np.float64 and np.array_equal(got[k], tab[k])


def test_read_setfl_two_elements_raises(tmp_path):
    path = et.write_setfl(tmp_path / "t.eam.alloy", et.fs(nr=20, nrho=20))
    lines = open(path).read().splitlines()
    lines[3] = "2 Fe Cr"
    open(path, "w").write("\n".join(lines) + "\n")
    with pytest.raises(NotImplementedError):
        systems.read_setfl(path)


@pytest.mark.parametrize("n,L,seed", [(6, 3.0, 1), (9, 3.4, 2), (3, 2.2, 3)])
def test_cubic_tables_reproduce_the_analytic_energy_and_gradient(n, L, seed):
    tab = et.cubic()
    pos, U, grad = config(tab, (L, L, L), n, seed)
    eam = systems.EAM(tab, L)
    u, g = energy_and_grad(eam, pos)
    assert rel_err(u, U) <= REL, rel_err(u, U)
    assert rel_err(g, grad) <= REL, rel_err(g, grad)
    assert rel_err(eam.force(torch.as_tensor(pos)), -grad) <= REL


def test_hand_case_two_atoms_two_images():
    """(a) N = 2 at (0,0,0) and (1.2,0,0), L = 3, rc = 2: the neighbour counts at
    1.2 and, through the next image, at 1.8."""
    tab = et.cubic()
    f, F = (lambda r: et.poly(et.CUBIC_f, r)), (lambda x: et.poly(et.CUBIC_F, x))
    phi = lambda r: et.poly(et.CUBIC_z, r) / r  # noqa: E731
    U = 2 * F(f(1.2) + f(1.8)) + phi(1.2) + phi(1.8)
    u, _ = energy_and_grad(systems.EAM(tab, 3.0), [[0.0, 0.0, 0.0], [1.2, 0.0, 0.0]])
    assert rel_err(u, U) <= REL, (float(u), U)


def test_hand_case_one_atom_six_self_images():
    """(b) N = 1, rc = 1.2 L: U = F(6 f(L)) + 3 phi(L), force exactly 0."""
    tab = et.cubic()
    L = tab["rc"] / 1.2
    U = et.poly(et.CUBIC_F, 6 * et.poly(et.CUBIC_f, L)) + 3 * et.poly(et.CUBIC_z, L) / L
    eam = systems.EAM(tab, L)
    u, g = energy_and_grad(eam, [[0.3, 0.1, 0.7]])
    assert rel_err(u, U) <= REL, (float(u), U)
    assert torch.equal(g, torch.zeros_like(g))
    assert torch.equal(eam.force(torch.tensor([[0.3, 0.1, 0.7]], dtype=F64)), torch.zeros(1, 3, dtype=F64))


def test_hand_case_short_cutoff_equals_minimum_image():
    """(c) rc < L/2: one image per pair, the nearest."""
    tab = et.cubic()
    L = 4.5
    pos, U, _ = config(tab, (L, L, L), 7, 11)
    d = pos[:, None, :] - pos[None, :, :]
    d = d - L * np.round(d / L)
    r = np.sqrt((d * d).sum(-1))
    ok = (r > 0) & (r <= tab["rc"])
    rho = np.where(ok, et.poly(et.CUBIC_f, np.where(ok, r, 1.0)), 0.0).sum(1)
    Umin = et.poly(et.CUBIC_F, rho).sum() + 0.5 * np.where(ok, et.poly(et.CUBIC_z, r) / np.where(ok, r, 1.0), 0).sum()
    eam = systems.EAM(tab, L)
    assert eam.nshift == (0, 0, 0)
    u, _ = energy_and_grad(eam, pos)
    assert rel_err(u, Umin) <= REL and rel_err(U, Umin) <= REL


def test_hand_case_density_beyond_the_table_continues_linearly():
    """(d) hand case (a) with a rho table that ends at 1.0 < rho = 1.88:
    F = F(rho_max) + F'(rho_max) (rho - rho_max), F' the table's end slope."""
    tab = et.cubic(rho_max=1.0)
    f = lambda r: et.poly(et.CUBIC_f, r)  # noqa: E731
    phi = lambda r: et.poly(et.CUBIC_z, r) / r  # noqa: E731
    rho = f(1.2) + f(1.8)
    assert rho > 1.5
    slope = (tab["F"][-1] - tab["F"][-2]) / tab["drho"]
    U = 2 * (tab["F"][-1] + slope * (rho - 1.0)) + phi(1.2) + phi(1.8)
    u, g = energy_and_grad(systems.EAM(tab, 3.0), [[0.0, 0.0, 0.0], [1.2, 0.0, 0.0]])
    assert rel_err(u, U) <= REL, (float(u), U)
    df = lambda r: et.dpoly(et.CUBIC_f, r)  # noqa: E731
    dphi = lambda r: (et.dpoly(et.CUBIC_z, r) - phi(r)) / r  # noqa: E731
    # dU/dx_0 along x: the image at -1.2 (d = -1.2) and the one at +1.8
    gx = -(dphi(1.2) + 2 * slope * df(1.2)) + (dphi(1.8) + 2 * slope * df(1.8))
    assert rel_err(g[0, 0], gx) <= REL and rel_err(g[1, 0], -gx) <= REL


def test_translation_permutation_and_box_vector_invariance():
    tab = et.fs(nr=400, nrho=400)
    L = 0.61 ** -1 * tab["rc"]
    eam = systems.EAM(tab, L)
    pos = et.bcc(2, L / 2, jitter=0.08, seed=5)
    u, g = energy_and_grad(eam, pos)
    u_t, g_t = energy_and_grad(eam, pos + np.array([0.37, -1.9, 12.3]))
    perm = np.random.default_rng(0).permutation(len(pos))
    u_p, g_p = energy_and_grad(eam, pos[perm])
    moved = pos.copy()
    moved[3] += np.array([L, -2 * L, 0.0])
    u_m, g_m = energy_and_grad(eam, moved)
    for what, (uu, gg, ref) in dict(translate=(u_t, g_t, g), permute=(u_p, g_p, g[perm]),
                                    box_vector=(u_m, g_m, g)).items():
        assert rel_err(uu, u) <= REL, (what, rel_err(uu, u))
        assert rel_err(gg, ref) <= REL, (what, rel_err(gg, ref))


@pytest.mark.parametrize("n,L,nshift", [(5, 3.2, (1, 0, 1)), (2, 1.5, (1, 1, 2))])
def test_orthorhombic_box_against_a_brute_force_scan(n, L, nshift):
    tab = et.cubic()
    box = (L, 1.3 * L, 0.8 * L)
    eam = systems.EAM(tab, box)
    assert eam.nshift == nshift
    pos, U, grad = config(tab, box, n, 21 + n)  # brute(): shifts -3..3
    u, g = energy_and_grad(eam, pos)
    assert rel_err(u, U) <= REL, rel_err(u, U)
    assert rel_err(g, grad) <= REL, rel_err(g, grad)


def test_batched_rows_and_fp32_follow_fp64():
    tab = et.fs(nr=500, nrho=500)
    L = tab["rc"] / 0.61
    eam = systems.EAM(tab, L)
    pos = torch.as_tensor(et.bcc(2, L / 2, jitter=0.05, seed=2, batch=3))
    u = eam.potential(pos)
    assert u.shape == (3,) and u.dtype == F64
    for b in range(3):
        assert rel_err(eam.potential(pos[b]), u[b]) <= 1e-13
    eam._CHUNK_ELEMS = 16 * 16  # one row per chunk
    assert torch.equal(eam.potential(pos), u)
    u32 = eam.potential(pos.float())
    assert u32.dtype == torch.float32 and rel_err(u32, u) <= 1e-5


# ---------------------------------------------------------------------------
def test_build_potential_from_an_fe_config(tmp_path):
    cfg, tab, frames = et.fe_config(tmp_path)
    pot = app.build_potential(cfg)
    assert isinstance(pot, systems.EAM)
    assert pot.box == (2 * 2.8841,) * 3 and pot.nparticles == 16 and pot.rc == tab["rc"]
    assert np.array_equal(pot.table["f"], tab["f"])
    x = pot.sample(5)
    assert x.shape == (5, 48)
    first = pot.sample(4, flatten=False, random=False)
    assert torch.equal(first, torch.from_numpy(frames[:4]))
    assert pot.potential(first).shape == (4,)
    np.save(tmp_path / "more.npy", frames[:3] + 1.0)
    pot.update_data(str(tmp_path / "more.npy"), append=True)
    assert pot.traj.shape == (15, 16, 3)
    pot.update_data(str(tmp_path / "more.npy"))
    assert torch.equal(pot.traj, torch.from_numpy(frames[:3] + 1.0))


def test_fe_without_eam_file_raises(tmp_path):
    cfg, _, _ = et.fe_config(tmp_path, with_eam=False)
    with pytest.raises(NotImplementedError, match="eam_file"):
        app.build_potential(cfg)


def small_system(dtype=torch.float32):
    tab = et.fs(nr=600, nrho=600)
    L = tab["rc"] / 0.61
    eam = systems.EAM(tab, L, nparticles=16)
    pos = torch.as_tensor(et.bcc(2, L / 2, jitter=0.04, seed=4, batch=3), dtype=dtype)
    return eam, pos


def test_integration_step_verlet_equals_the_written_out_steps():
    eam, x0 = small_system()
    v0 = 0.3 * torch.randn(x0.shape, generator=torch.Generator().manual_seed(1))
    dt = 0.01
    x, pot = eam.integration_step(path_len=3, dt=dt, init_pos=x0, init_velocity=v0, scheme="verlet")
    xe, ve, G = x0, v0, eam.force(x0)
    for _ in range(3):
        xn = (xe + ve * dt) + (G * 0.5) * dt ** 2
        Gn = eam.force(xn)
        ve = ve + (dt * (G + Gn)) * 0.5
        xe, G = xn, Gn
    assert torch.equal(x, xe) and torch.equal(eam.get_velocity(), ve)
    assert torch.equal(pot, eam.potential(xe)) and torch.equal(eam.last_force, G)
    assert not torch.equal(x, x0)


def test_hmc_records_the_potential_of_the_recorded_position():
    eam, x0 = small_system()
    torch.manual_seed(3)
    run = nf.hmc.HMC(eam, init_pos=x0, path_len=2, dt=0.01, beta=1.0 / 0.05, scheme="verlet")
    positions, potentials, _, rate = run.hmc(epochs=4)
    assert positions.shape == (4, 3, 48) and potentials.shape == (4, 3) and 0.0 <= rate <= 1.0
    for i in range(4):
        assert torch.equal(potentials[i], eam.potential(positions[i].reshape(3, 16, 3)))
    assert not torch.equal(positions[0], positions[3]) or rate == 0.0
