"""CPU checks of the EAM dynamics entry points: the symbols and their ctypes
signatures, the host-side validation of nfk_eam_trajectory / nfk_eam_hmc_run
(which never touches a device), ``hmc(one_launch=True)`` on CPU tensors against
the docstring's recipe, and that ``fused_dynamics`` changes nothing on the CPU.
"""
import ctypes

import torch

import eam_tables as et
from nf.hmc import HMC
from normalizingflow_amd import _lib, systems
from test_gpu_eam import lattice
from test_hmc_run_cpu import segments

NEW = ["nfk_eam_trajectory", "nfk_eam_hmc_supported", "nfk_eam_hmc_run"]
CHAINS, EPOCHS = 5, 4


def test_the_new_symbols_are_exported_and_in_the_ctypes_table():
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in NEW:
        assert hasattr(lib, name) and name in _lib.SIGNATURES, name
    # trajectory (14) / run (18) arguments, n, nfk_eam_potential's 12 table and box arguments, the stream
    assert len(_lib.SIGNATURES["nfk_eam_trajectory"][1]) == 14 + 1 + 12 + 1
    assert len(_lib.SIGNATURES["nfk_eam_hmc_run"][1]) == 18 + 1 + 12 + 1
    lib = _lib.load()
    for n, want in ((1, 1), (54, 1), (256, 1), (257, 0), (0, 0), (-3, 0)):
        assert lib.nfk_eam_hmc_supported(n) == want == lib.nfk_eam_supported(n)


# tables: 16 stands for an aligned device pointer that is never read
def _tables(rtab=16, ftab=16, nr=100, nrho=100, lx=6.0, rc=3.7):
    return [rtab, nr, 0.04, ftab, nrho, 0.6, -10.0, -0.1, lx, 6.0, 6.0, rc]


def _traj(lib, ptr=None, ld=48, batch=2, path_len=1, scheme=0, n=16, **tab):
    return lib.nfk_eam_trajectory(ptr, ld, ptr, ld, ptr, ld, ptr, ld, ptr, batch, path_len, 0.01, 1e-4, scheme, n,
                                  *_tables(**tab), None)


def _run(lib, ptr=None, ld=48, chains=2, epochs=3, path_len=1, scheme=0, n=16, pos_rec=None, **tab):
    return lib.nfk_eam_hmc_run(ptr, ld, ptr, None, ptr, ptr, None, ld, pos_rec, None, chains, epochs, path_len,
                               0.01, 1e-4, scheme, 1.0, 0, n, *_tables(**tab), None)


def test_refusals_never_reach_the_device():
    """Every refusal is decided on the host before anything is enqueued: the data
    pointers are null or placeholders that are never read."""
    lib = _lib.load()
    refusals = [
        (dict(n=257, ld=771), b"shape not supported"),
        (dict(n=0), b"shape not supported"),
        (dict(path_len=-1), b"path_len below zero"),
        (dict(scheme=2), b"scheme must be 0"),
        (dict(scheme=-1), b"scheme must be 0"),
        (dict(), b"null pointer"),
        (dict(ptr=1, ld=47), b"leading dimension"),
        (dict(ptr=1, rc=-1.0), b"bad tables, box or cutoff"),
        (dict(ptr=1, lx=0.0), b"bad tables, box or cutoff"),
        (dict(ptr=1, rc=49.0), b"bad tables, box or cutoff"),  # rc / L above 8
        (dict(ptr=1, nr=1), b"bad tables, box or cutoff"),
        (dict(ptr=1, rtab=20), b"tables need 16-byte alignment"),
        (dict(ptr=1, ftab=8), b"tables need 16-byte alignment"),
        (dict(ptr=1, rtab=None), b"null pointer"),
    ]
    for call, who in ((_traj, b"nfk_eam_trajectory: "), (_run, b"nfk_eam_hmc_run: ")):
        for kw, msg in refusals:
            assert call(lib, **kw) == _lib.NFK_EINVAL, (who, kw)
            err = lib.nfk_last_error()
            assert err.startswith(who) and msg in err, (kw, err)
    assert _traj(lib, batch=-1) == _lib.NFK_EINVAL and b"bad batch" in lib.nfk_last_error()
    assert _run(lib, chains=-1) == _lib.NFK_EINVAL and b"bad chains" in lib.nfk_last_error()
    assert _run(lib, epochs=-1) == _lib.NFK_EINVAL and b"epochs below zero" in lib.nfk_last_error()
    assert _run(lib, ptr=1, pos_rec=1) == _lib.NFK_EINVAL and b"come together" in lib.nfk_last_error()
    # nothing to do: 0 without a launch, but the tables are still looked at
    assert _traj(lib, batch=0) == 0 and _run(lib, chains=0) == 0 and _run(lib, epochs=0) == 0
    assert _traj(lib, batch=0, rc=-1.0) == _lib.NFK_EINVAL and b"bad tables" in lib.nfk_last_error()
    assert _run(lib, epochs=0, rc=-1.0) == _lib.NFK_EINVAL and b"bad tables" in lib.nfk_last_error()


def _chains():
    tab = et.fs(rho_max=400.0)
    L = tab["rc"] / 0.61
    return systems.EAM(tab, L), torch.as_tensor(lattice(16, CHAINS, L, 1016), dtype=torch.float32)


def recipe_loop(sim, run, x0, epochs, draw_bytes=1 << 28):
    """``hmc(epochs, x0, one_launch=True)`` restated for [C, n, 3] positions: the
    recipe's draws, then ``integration_step`` and the torch accept expression."""
    chains, W = x0.shape[0], x0[0].numel()
    x_cur, u_cur = x0.reshape(chains, W).clone(), sim.potential(x0).detach().clone()
    nacc = torch.zeros(chains, dtype=torch.int32)
    pos, pot = [], []
    sd = run._var(x0.device, x0.dtype).sqrt()
    for e in segments(epochs, chains, W, draw_bytes):
        v = torch.randn(e, chains, W, dtype=x0.dtype) * sd
        r = torch.rand(e, chains, dtype=x0.dtype)
        for i in range(e):
            pos.append(x_cur.clone())
            pot.append(u_cur.clone())
            x_new, u_new = sim.integration_step(run.path_len, run.dt, x_cur.view(x0.shape).clone(),
                                                v[i].view(x0.shape), scheme=run.scheme)
            d = u_cur - u_new
            if run.hamiltonian:
                vn = sim.get_velocity().reshape(chains, W)
                d = (d + 0.5 * (v[i] * v[i]).sum(1)) - 0.5 * (vn * vn).sum(1)
            acc = r[i] < torch.exp(d * run.beta)
            x_cur = torch.where(acc.unsqueeze(1), x_new.reshape(chains, W), x_cur)
            u_cur = torch.where(acc, u_new, u_cur)
            nacc += acc.to(torch.int32)
    return torch.stack(pos), torch.stack(pot), x_cur, u_cur, nacc, sim.get_velocity(), run.log_prob(v[-1])


def test_one_launch_equals_the_recipe_loop_on_cpu():
    sim, x0 = _chains()
    assert sim.fused_dynamics is True
    for scheme, hamiltonian, dt in (("reference", False, 0.02), ("verlet", True, 0.3)):
        run = HMC(sim, path_len=3, dt=dt, dim=3, beta=20.0, scheme=scheme, hamiltonian=hamiltonian)
        torch.manual_seed(77)
        pos, pot, lp, rate = run.hmc(EPOCHS, x0, one_launch=True)
        got_v, fin, ufin, nacc = sim.get_velocity(), run.position.clone(), run.potential.clone(), run.naccept.clone()
        torch.manual_seed(77)
        wpos, wpot, wx, wu, wn, wv, wlp = recipe_loop(sim, run, x0, EPOCHS)
        assert pos.shape == (EPOCHS, CHAINS, 48) and torch.equal(pos, wpos) and torch.equal(pot, wpot)
        assert torch.equal(fin, wx) and torch.equal(ufin, wu) and torch.equal(nacc, wn)
        assert torch.equal(got_v, wv) and torch.equal(lp, wlp)
        assert rate == float(wn.double().mean()) / EPOCHS and int(wn.sum()) > 0


def test_fused_dynamics_changes_nothing_on_the_cpu():
    assert systems.EAM.fused_dynamics is True
    sim, x0 = _chains()
    v0 = 0.3 * torch.randn(x0.shape, generator=torch.Generator().manual_seed(1))
    out = []
    for fused in (True, False):
        sim.fused_dynamics = fused
        x, pot = sim.integration_step(3, 0.01, x0, v0, scheme="verlet")
        out.append((x, sim.get_velocity(), pot, sim.last_force))
        assert not sim._hmc_run(x0.reshape(CHAINS, 48), pot, None, v0.reshape(1, CHAINS, 48), pot.reshape(1, -1),
                                shape=x0.shape, path_len=1, dt=0.01, sch=1, beta=1.0, hamiltonian=False)
    for a, b in zip(*out):
        assert torch.equal(a, b)
    # the written-out steps on the autograd force
    x, v, G = x0, v0, sim.force(x0)
    for _ in range(3):
        xn = (x + v * 0.01) + (G * 0.5) * 0.01 ** 2
        Gn = sim.force(xn)
        v = v + (0.01 * (G + Gn)) * 0.5
        x, G = xn, Gn
    assert torch.equal(out[0][0], x) and torch.equal(out[0][1], v) and torch.equal(out[0][3], G)
    assert torch.equal(out[0][2], sim.potential(x))
