"""Generate the ``sys_*`` golden vectors from the REFERENCE's
applications/src/systems.py (EinsteinCrystal, GaussianMixture, LJ).

Run in the build container (where /root/reference exists):

    python tests/golden/make_systems_golden.py

The reference module imports lammps and MDAnalysis at the top, neither of
which its three classes use: module objects carrying the imported names stand
in for them.  Nothing else of the reference is altered and no bytecode is
written.  Outputs ``tests/golden/sys_<case>.npz`` in golden_io.load's format
(a JSON ``meta`` string plus arrays): the inputs, the reference's fp32 output,
the gradient of sum_b w_b out_b w.r.t. the input from the reference's own
autograd (``w`` stored), and the fp64 companions of both -- the same formula
on ``.double()`` inputs.  For EinsteinCrystal and GaussianMixture the fp64 run
is the reference class with its tensors and component distributions rebuilt
in double; LJ.potential casts to float inside (systems.py:170), so its fp64
companion is the formula restated here (``lj_f64``).

The generator asserts that no tie can decide a test: no deviation or pair
component within 1e-4 L of L/2, no pair distance within 1e-4 of the cutoff,
and (outside the "far" fixture) every particle's mixture density >= 1e-30.
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

import numpy as np  # noqa: E402
import torch  # noqa: E402
from torch.distributions import MultivariateNormal  # noqa: E402

from src import systems as rsys  # noqa: E402

assert os.path.realpath(rsys.__file__).startswith(REF), rsys.__file__

ROWS = 37
RHO = 1.28


def _save(name, meta, arrays):
    out = {"meta": np.array(json.dumps(meta))}
    for k, v in arrays.items():
        out[k] = v.detach().cpu().numpy() if torch.is_tensor(v) else np.asarray(v)
    path = os.path.join(HERE, "sys_" + name + ".npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


def _run(fn, x, w):
    """(out, d sum_b w_b out_b / dx) of fn at x."""
    xr = x.detach().clone().requires_grad_()
    out = fn(xr)
    g, = torch.autograd.grad((out * w.to(out.dtype)).sum(), xr)
    return out.detach(), g


def _lattice(kind, cells, L):
    """fcc / bcc / sc lattice of ``cells`` per side in [-L/2, L/2)."""
    cx, cy, cz = cells if isinstance(cells, tuple) else (cells,) * 3
    basis = {"fcc": [(0, 0, 0), (.5, .5, 0), (.5, 0, .5), (0, .5, .5)],
             "bcc": [(0, 0, 0), (.5, .5, .5)], "sc": [(0, 0, 0)]}[kind]
    pts = [((i + b[0]) / cx, (j + b[1]) / cy, (k + b[2]) / cz)
           for i in range(cx) for j in range(cy) for k in range(cz) for b in basis]
    return (torch.tensor(pts, dtype=torch.float64) * L - L / 2 + L / (4 * max(cx, cy, cz))).float()


def _box_wrap(x, L):
    return x - L * torch.floor(x / L + 0.5)


# ------------------------------------------------------------------ Einstein
def case_einstein(name, centers, dim, boxlength, alpha, seed):
    g = torch.Generator().manual_seed(seed)
    natoms = centers.shape[0]
    x = centers + torch.randn(ROWS, natoms, dim, generator=g) / math.sqrt(alpha)
    if boxlength:  # ~5 % of the coordinates one box away, so the wrap fires
        push = torch.rand(ROWS, natoms, dim, generator=g) < 0.05
        sgn = torch.where(torch.rand(ROWS, natoms, dim, generator=g) < 0.5, -1.0, 1.0)
        x = x + push * sgn * boxlength
        dev = (x - centers).abs()
        assert ((dev - 0.5 * boxlength).abs() > 1e-4 * boxlength).all()
        assert (dev > 0.5 * boxlength).sum() >= 2
    x = x.reshape(ROWS, -1).contiguous()
    w = torch.randn(ROWS, generator=g)
    ref = rsys.EinsteinCrystal(centers.numpy(), dim, boxlength=boxlength, alpha=alpha)
    out, grad = _run(ref.log_prob, x, w)
    ref64 = rsys.EinsteinCrystal(centers.numpy(), dim, boxlength=boxlength, alpha=alpha)
    ref64.centers = ref64.centers.double()
    ref64.noise = MultivariateNormal(torch.zeros(dim).double(), 1 / alpha * torch.eye(dim).double())
    out64, grad64 = _run(ref64.log_prob, x.double(), w)
    assert torch.isfinite(out).all() and torch.isfinite(grad).all()
    _save(name, dict(kind="einstein", natoms=natoms, dim=dim, boxlength=boxlength, alpha=alpha, seed=seed),
          dict(centers=centers, x=x, w=w, out=out, grad=grad, out64=out64, grad64=grad64))


# ------------------------------------------------------------------- mixture
def case_gmix(name, centers, vars_, npart, dim, seed, far=False):
    g = torch.Generator().manual_seed(seed)
    c = torch.tensor(centers).float()
    M = len(c)
    v = torch.tensor(vars_).float()
    vv = v.expand(M) if v.dim() == 0 else v
    which = torch.randint(M, (ROWS * npart,), generator=g)
    x = c[which] + torch.randn(ROWS * npart, dim, generator=g) * vv[which].sqrt().unsqueeze(1)
    x = x.reshape(ROWS, npart * dim).contiguous()
    if far:  # one particle of every third row where exp underflows to exactly 0 in fp32
        for b in range(0, ROWS, 3):
            p = b % npart
            x[b, p * dim:(p + 1) * dim] = 9.0
            d2 = ((x[b, p * dim:(p + 1) * dim].double() - c.double()) ** 2).sum(1) / (2 * vv.double())
            assert (d2 > 110).all()
    w = torch.randn(ROWS, generator=g)
    ref = rsys.GaussianMixture(centers, vars_, npart, dim)
    out, grad = _run(ref.log_prob, x, w)
    ref64 = rsys.GaussianMixture(centers, vars_, npart, dim)
    ref64.centers = ref64.centers.double()
    ref64.vars = ref64.vars.double()
    ref64.dist = [MultivariateNormal(ref64.centers[i], ref64.vars[i] * torch.eye(dim).double())
                  for i in range(M)]
    out64, grad64 = _run(ref64.log_prob, x.double(), w)
    if far:
        assert torch.isinf(out[0::3]).all() and (out[0::3] < 0).all()
        keep = torch.ones(ROWS, dtype=torch.bool)
        keep[0::3] = False
        assert torch.isfinite(out[keep]).all()
    else:
        # every particle's density is a normal number: no subnormal decides anything
        dens = sum(1 / M * torch.exp(d.log_prob(x.double().reshape(-1, dim))) for d in ref64.dist)
        assert (dens >= 1e-30).all(), float(dens.min())
        assert torch.isfinite(out).all() and torch.isfinite(grad).all()
    _save(name, dict(kind="gmix", centers=centers, vars=vars_, npart=npart, dim=dim, seed=seed, far=far),
          dict(x=x, w=w, out=out, grad=grad, out64=out64, grad64=grad64))


# ------------------------------------------------------------------------ LJ
def lj_f64(pos, L, sigma, epsilon, cutoff, shift):
    """LJ.potential (systems.py:166-189) without its cast to float."""
    pd = pos.unsqueeze(-2) - pos.unsqueeze(-3)
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
    return torch.sum(u, axis=(-1, -2)) / 2


def _lj_ties(pos, L, cutoff, skip=None):
    """[B, N] mask of particles in a pair with a component within 1e-4 L of L/2
    or (with a cutoff) a distance within 1e-4 of it."""
    pd = pos.unsqueeze(-2) - pos.unsqueeze(-3)
    bad = ((pd.abs() - 0.5 * L).abs() <= 1e-4 * L).any(-1)
    pd = pd - (pd.abs() > 0.5 * L) * torch.sign(pd) * L
    d = torch.linalg.norm(pd, axis=-1)
    if cutoff is not None:
        bad |= (d - cutoff).abs() <= 1e-4
    return bad.any(-1)


def case_lj(name, lattice, L, seed, sigma=1.0, epsilon=1.0, cutoff=1.6, shift=True, coincident=False):
    g = torch.Generator().manual_seed(seed)
    n, dim = lattice.shape
    pos = _box_wrap(lattice + 0.05 * torch.randn(ROWS, n, dim, generator=g), L)
    for _ in range(500):  # move particles off the wrap's and the cutoff's ties
        bad = _lj_ties(pos, L, cutoff)
        if not bad.any():
            break
        pos = _box_wrap(pos + bad.unsqueeze(-1) * 2e-3 * L * torch.randn(ROWS, n, dim, generator=g), L)
    if coincident:  # d == 0 off the diagonal: zero energy for the pair
        pos[:5, 1] = pos[:5, 0]
    assert not _lj_ties(pos, L, cutoff).any()
    w = torch.randn(ROWS, generator=g)
    ref = rsys.LJ(boxlength=L, sigma=sigma, epsilon=epsilon, cutoff=cutoff, shift=shift)
    out, grad = _run(ref.potential, pos, w)
    out64, grad64 = _run(lambda p: lj_f64(p, L, sigma, epsilon, cutoff, shift), pos.double(), w)
    assert torch.isfinite(out).all() and torch.isfinite(grad).all()
    pd = pos.unsqueeze(-2) - pos.unsqueeze(-3)
    pd = pd - (pd.abs() > 0.5 * L) * torch.sign(pd) * L
    d = torch.linalg.norm(pd, axis=-1) + 1e3 * torch.eye(n)
    print("  %s: energies %.3g .. %.3g, closest pair %.3g, reference fp32 error %.3g abs"
          % (name, out.min(), out.max(), d[5:].min(), (out.double() - out64).abs().max()))
    _save(name, dict(kind="lj", n=n, dim=dim, boxlength=L, sigma=sigma, epsilon=epsilon, cutoff=cutoff,
                     shift=shift, coincident=coincident, seed=seed),
          dict(x=pos, w=w, out=out, grad=grad, out64=out64, grad64=grad64))


def main():
    L32 = round((32 / RHO) ** (1 / 3), 5)   # LJ.yaml's box, 2.92402
    L54 = round((54 / RHO) ** (1 / 3), 5)
    fcc32 = _lattice("fcc", 2, L32)
    bcc54 = _lattice("bcc", 3, L54)
    g = torch.Generator().manual_seed(7)
    c52 = (torch.rand(5, 2, generator=g) - 0.5) * L32
    c13 = (torch.rand(1, 3, generator=g) - 0.5) * L32
    seed = 100
    for box, tag in ((None, "nobox"), (L32, "box"), (0, "box0")):
        for alpha in (600, 70):
            seed += 1
            case_einstein("einstein_32x3_%s_a%d" % (tag, alpha), fcc32, 3, box, alpha, seed)
    case_einstein("einstein_54x3_box_a70", bcc54, 3, L54, 70, 111)
    case_einstein("einstein_54x3_nobox_a600", bcc54, 3, None, 600, 112)
    case_einstein("einstein_5x2_box_a600", c52, 2, L32, 600, 113)
    case_einstein("einstein_5x2_box0_a70", c52, 2, 0, 70, 114)
    case_einstein("einstein_1x3_box_a70", c13, 3, L32, 70, 115)
    case_einstein("einstein_1x3_nobox_a600", c13, 3, None, 600, 116)

    case_gmix("gmix_yaml", [[-1, -1], [1, 1]], [0.1, 0.05], 20, 2, 201)
    case_gmix("gmix_rnvp", [[-0.5, -0.5]], 0.25, 20, 2, 202)
    gm = torch.Generator().manual_seed(9)
    c5 = (torch.rand(5, 3, generator=gm) * 2 - 1).tolist()
    v5 = (0.05 + 0.25 * torch.rand(5, generator=gm)).tolist()
    case_gmix("gmix_m5d3", c5, v5, 7, 3, 203)
    case_gmix("gmix_far", [[-1, -1], [1, 1]], [0.1, 0.05], 20, 2, 204, far=True)

    case_lj("lj_n32_cut_shift", fcc32, L32, 301)
    case_lj("lj_n32_cut_noshift", fcc32, L32, 302, shift=False)
    case_lj("lj_n32_nocut", fcc32, L32, 303, cutoff=None)
    case_lj("lj_n32_sigma", fcc32, L32, 304, sigma=0.9, epsilon=1.7)
    case_lj("lj_n32_coincident", fcc32, L32, 305, coincident=True)
    case_lj("lj_n54_cut_shift", bcc54, L54, 306)
    case_lj("lj_n5_cut_noshift", _lattice("sc", 2, 2.2)[:5], 2.2, 307, shift=False)
    case_lj("lj_n100_cut_shift", _lattice("sc", (5, 5, 4), 5.0), 5.0, 308)
    case_lj("lj_n6d2_nocut", _lattice("sc", (3, 2, 1), 3.3)[:, :2].contiguous(), 3.3, 309, cutoff=None)


if __name__ == "__main__":
    main()
