"""Generate the ``dyn_*`` golden vectors from the REFERENCE's integrators
(applications/src/systems.py:297-338 and 382-401) and its HMC velocity
distribution (nf/hmc.py).

Run in the build container (where /root/reference exists):

    python tests/golden/make_dynamics_golden.py

The reference is imported as make_systems_golden.py imports it: module objects
stand in for lammps and MDAnalysis, nothing of the reference is altered and no
bytecode is written.  Outputs ``tests/golden/dyn_<case>.npz`` in
golden_io.load's format, arrays only: ``x0`` / ``v0`` [37, W], and per
path_len P in (1, 12) at dt 0.005 the reference's final position ``xP``, its
``self.velocity`` ``vP`` and potential ``potP`` from ONE flattened-batch
``integration_step`` call (the reference flattens what set_position gets, so
the 37 rows go through as one vector), plus the fp64 companions ``xP_64`` /
``vP_64`` / ``potP_64``: the same call on the reference objects rebuilt in
double.  ``dyn_hmc_vdist`` holds velocities and HMC's ``v_dist.log_prob`` for
mass [55.845], init_beta = beta / 1000 (dynamics.py:49).

The generator asserts that no Einstein deviation comes within 1e-4 L of L/2 at
any step of the fp64 run, so no wrap tie decides a test.
"""
from __future__ import annotations

import json
import math
import os
import sys
import types

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
REF = "/root/reference"

sys.dont_write_bytecode = True
sys.path[:] = [p for p in sys.path if os.path.abspath(p or ".") not in (REPO, HERE)]
_lammps = types.ModuleType("lammps")
for _n in ("lammps", "PyLammps", "LMP_STYLE_ATOM", "LMP_TYPE_ARRAY"):
    setattr(_lammps, _n, None)
sys.modules.setdefault("lammps", _lammps)
sys.modules.setdefault("MDAnalysis", types.ModuleType("MDAnalysis"))
sys.path.insert(0, REF + "/applications")
sys.path.insert(1, REF)

import numpy as np  # noqa: E402
import torch  # noqa: E402
from torch.distributions import MultivariateNormal  # noqa: E402

from src import systems as rsys  # noqa: E402
from nf import hmc as rhmc  # noqa: E402

assert os.path.realpath(rsys.__file__).startswith(REF), rsys.__file__
assert os.path.realpath(rhmc.__file__).startswith(REF), rhmc.__file__

ROWS = 37
DT = 0.005
PATHS = (1, 12)
L32 = 2.92402


def _save(name, meta, arrays):
    out = {"meta": np.array(json.dumps(meta))}
    for k, v in arrays.items():
        out[k] = v.detach().cpu().numpy() if torch.is_tensor(v) else np.asarray(v)
    path = os.path.join(HERE, "dyn_" + name + ".npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


def _fcc32(L):
    basis = [(0, 0, 0), (.5, .5, 0), (.5, 0, .5), (0, .5, .5)]
    pts = [((i + b[0]) / 2, (j + b[1]) / 2, (k + b[2]) / 2)
           for i in range(2) for j in range(2) for k in range(2) for b in basis]
    return (torch.tensor(pts, dtype=torch.float64) * L - L / 2 + L / 8).float()


def _trajectories(make, x0, v0, arrays, watch=None):
    """One flattened-batch integration_step per path length, fp32 and fp64."""
    for P in PATHS:
        for tag, dt_ in (("", torch.float32), ("_64", torch.float64)):
            sim = make(dt_)
            pos, pot = sim.integration_step(P, DT, x0.to(dt_).clone(), v0.to(dt_).clone())
            assert pos.dtype == dt_ and pos.shape == (x0.numel(),) and pot.shape == (ROWS,)
            assert torch.isfinite(pos).all() and torch.isfinite(pot).all()
            arrays["x%d%s" % (P, tag)] = pos.detach().reshape(x0.shape)
            arrays["v%d%s" % (P, tag)] = sim.velocity.detach().reshape(x0.shape)
            arrays["pot%d%s" % (P, tag)] = pot.detach()
    if watch is not None:  # every position the fp64 run of the longest path passes through
        sim = make(torch.float64)
        sim.set_position(x0.double().clone())
        sim.set_velocity(v0.double().clone())
        watch(sim.position.detach())
        for _ in range(max(PATHS)):
            sim.integration_step(1, DT)
            watch(sim.position.detach())


def case_einstein(name, centers, dim, boxlength, alpha, seed):
    g = torch.Generator().manual_seed(seed)
    natoms = centers.shape[0]
    x0 = (centers + torch.randn(ROWS, natoms, dim, generator=g) / math.sqrt(alpha)).reshape(ROWS, -1)
    if boxlength:  # ~5 % of the coordinates one box away, so the wrap fires
        push = torch.rand(ROWS, natoms * dim, generator=g) < 0.05
        sgn = torch.where(torch.rand(ROWS, natoms * dim, generator=g) < 0.5, -1.0, 1.0)
        x0 = x0 + push * sgn * boxlength
    x0 = x0.contiguous()
    v0 = torch.randn(ROWS, natoms * dim, generator=g)

    def make(dt_):
        sim = rsys.EinsteinCrystal(centers.numpy(), dim, boxlength=boxlength, alpha=alpha)
        if dt_ == torch.float64:
            sim.centers = sim.centers.double()
            sim.noise = MultivariateNormal(torch.zeros(dim).double(), 1 / alpha * torch.eye(dim).double())
        return sim

    wrapped = [0]

    def watch(pos):
        if boxlength:
            dev = (pos.reshape(ROWS, natoms, dim) - centers.double()).abs()
            assert ((dev - 0.5 * boxlength).abs() > 1e-4 * boxlength).all(), "a wrap tie"
            wrapped[0] += int((dev > 0.5 * boxlength).sum())

    arrays = dict(centers=centers, x0=x0, v0=v0)
    _trajectories(make, x0, v0, arrays, watch)
    if boxlength:
        assert wrapped[0] >= 2
    _save(name, dict(kind="einstein", natoms=natoms, dim=dim, boxlength=boxlength, alpha=alpha, seed=seed,
                     dt=DT, paths=list(PATHS)), arrays)


def case_gmix(name, centers, vars_, npart, dim, seed):
    g = torch.Generator().manual_seed(seed)
    c = torch.tensor(centers).float()
    M = len(c)
    vv = torch.tensor(vars_).float()
    vv = vv.expand(M) if vv.dim() == 0 else vv
    which = torch.randint(M, (ROWS * npart,), generator=g)
    x0 = c[which] + torch.randn(ROWS * npart, dim, generator=g) * vv[which].sqrt().unsqueeze(1)
    x0 = x0.reshape(ROWS, npart * dim).contiguous()
    v0 = torch.randn(ROWS, npart * dim, generator=g)

    def make(dt_):
        sim = rsys.GaussianMixture(centers, vars_, npart, dim)
        if dt_ == torch.float64:
            sim.centers = sim.centers.double()
            sim.vars = sim.vars.double()
            sim.dist = [MultivariateNormal(sim.centers[i], sim.vars[i] * torch.eye(dim).double())
                        for i in range(M)]
        return sim

    arrays = dict(x0=x0, v0=v0)
    _trajectories(make, x0, v0, arrays)
    _save(name, dict(kind="gmix", centers=centers, vars=vars_, npart=npart, dim=dim, seed=seed, dt=DT,
                     paths=list(PATHS)), arrays)


def case_vdist(name, nparticles, dim, mass, beta, seed):
    class _Sim:  # what HMC's constructor reads
        def get_position(self):
            return None

        def get_potential(self):
            return None

    _Sim.nparticles = nparticles
    run = rhmc.HMC(_Sim(), beta=beta, mass=torch.tensor(mass), dim=dim, init_beta=beta / 1000)
    g = torch.Generator().manual_seed(seed)
    std = math.sqrt(1 / (mass[0] * beta / 1000))
    v = torch.randn(ROWS, nparticles * dim, generator=g) * std
    lp = run.v_dist.log_prob(v)
    cov64 = run.v_dist.covariance_matrix.double()
    lp64 = MultivariateNormal(torch.zeros(nparticles * dim).double(), cov64).log_prob(v.double())
    _save(name, dict(kind="vdist", nparticles=nparticles, dim=dim, mass=mass, beta=beta, init_beta=beta / 1000,
                     seed=seed), dict(v=v, log_prob=lp, log_prob_64=lp64))


def main():
    g = torch.Generator().manual_seed(7)
    c52 = (torch.rand(5, 2, generator=g) - 0.5) * L32
    gm = torch.Generator().manual_seed(9)
    c3 = (torch.rand(3, 3, generator=gm) * 2 - 1).tolist()
    v3 = (0.05 + 0.25 * torch.rand(3, generator=gm)).tolist()
    case_gmix("gmix_m2_20x2", [[-1, -1], [1, 1]], [0.1, 0.05], 20, 2, 401)
    case_gmix("gmix_m3_5x3", c3, v3, 5, 3, 402)
    case_einstein("einstein_32x3_box_a600", _fcc32(L32), 3, L32, 600, 403)
    case_einstein("einstein_5x2_nobox_a600", c52, 2, None, 600, 404)
    case_vdist("hmc_vdist", 32, 3, [55.845], 1 / 0.05, 405)


if __name__ == "__main__":
    main()
