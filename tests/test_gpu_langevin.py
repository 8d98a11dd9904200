"""Langevin dynamics on the device (nfk_rng.h, nfk_langevin.hip, systems.*.langevin):
the Philox words against the CPU restatement, the normals against the fp64
Box-Muller of the same words, one launch against the per-step path bit for bit
(x, v, potential and records) for every system and mapping, chunking and row
blocks, fp64 restatements, and the sampled distributions."""
import math

import numpy as np
import pytest
import torch

import eam_tables as et
from normalizingflow_amd import config, rng, systems
from normalizingflow_amd import kernels as K_
from test_dynamics_cpu import L32, fcc32_state, lj_f64
from test_gpu_dynamics import fused_only
from test_gpu_eam import A_FE, lattice
from test_gpu_eam import close_or_on_par as eam_close_or_on_par
from test_gpu_systems import close_or_on_par, counts_of

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
ULP_MAX = 2.0 ** -21  # the fp32 spacing at the largest normal, 5.89


# ------------------------------------------------------------------------ the words
@pytest.mark.parametrize("tag", [0, 1])
def test_words_equal_the_cpu_restatement(tag, hip_device):
    for seed in (0, 1, 0xdeadbeef, (1 << 62) + 99, (1 << 63) - 1):
        for step in (0, 1, (1 << 32) + 5):
            for row_base, rows, n in ((0, 3, 70), (7, 37, 5), ((1 << 32) - 4, 4, 300)):
                dev = rng.philox_words(seed, rows, n, step, row_base, tag, device=DEV)
                cpu = rng.philox_words(seed, rows, n, step, row_base, tag)
                assert dev.dtype == torch.int32 and dev.shape == (rows, n, 4)
                assert torch.equal(dev.cpu(), cpu), (seed, step, row_base, tag)
    zero = rng.philox_words(0, 1, 1, 0, device=DEV)[0, 0].cpu().to(torch.int64) & 0xffffffff
    assert zero.tolist() == [0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8]


# ---------------------------------------------------------------------- the normals
def test_normals_against_the_fp64_box_muller_of_the_same_words(hip_device):
    rows, n = 1024, 256  # 2^20 values
    z = rng.philox_normal(5, rows, n, 4, step=3, row_base=11, device=DEV)
    want = rng.normals_from_words(rng.philox_words(5, rows, n, 3, 11, device=DEV), 4, dtype=torch.float64)
    err = float((z.double() - want).abs().max())
    print("normals: max |device fp32 - fp64 Box-Muller| = %.3g over 2^20 values, max |z| = %.4f"
          % (err, float(z.abs().max())))
    assert err < 1e-5
    N = z.numel()
    assert N == 1 << 20
    zz = z.double().flatten()
    assert abs(float(zz.mean())) < 5 / math.sqrt(N)
    assert abs(float(zz.var()) - 1) < 5 * math.sqrt(2 / N)
    assert float(z.abs().max()) <= 5.89
    for dim in (1, 2, 3):
        assert torch.equal(rng.philox_normal(5, 8, n, dim, step=3, row_base=11, device=DEV), z[:8, :, :dim])


@pytest.mark.parametrize("n", [1, 5, 64, 70, 256, 300])
def test_zero_mean_rows_sum_to_zero(n, hip_device):
    for dim in (2, 3, 4):
        z = rng.philox_normal(8, 37, n, dim, step=2, zero_mean=True, device=DEV)
        raw = rng.philox_normal(8, 37, n, dim, step=2, device=DEV)
        sums = z.double().sum(1).abs().max()
        print("zero_mean n %d dim %d: max |row sum| = %.3g (bound %.3g)" % (n, dim, float(sums), n * 4 * ULP_MAX))
        assert float(sums) <= n * 4 * ULP_MAX
        torch.testing.assert_close(z.double(), raw.double() - raw.double().mean(1, keepdim=True), rtol=0,
                                   atol=4 * ULP_MAX)


# ------------------------------------------------- one launch against the per-step path
def _tile(t, rows):
    return t[torch.arange(rows) % t.shape[0]]


def _einstein_case(natoms, dim, box):
    g = torch.Generator().manual_seed(7 + natoms)
    centers = (torch.rand(natoms, dim, generator=g) - 0.5) * L32
    sim = systems.EinsteinCrystal(centers, dim, boxlength=L32 if box else None, alpha=600, device=DEV)
    x = centers.flatten() + torch.randn(37, natoms * dim, generator=g) / math.sqrt(600)
    if box:  # some coordinates one box away: the wrap fires
        x = x + (torch.rand(37, natoms * dim, generator=g) < 0.05) * L32
    return sim, x, dict(dt=0.005, kT=0.02)


def _gmix_case(npart, dim):
    centers = [[-1., 0., 1.][:dim], [1., 1., 0.][:dim], [0., -1., -1.][:dim]]
    sim = systems.GaussianMixture(centers, [0.1, 0.05, 0.2], npart, dim, device=DEV)
    torch.manual_seed(17 + npart)
    return sim, sim.sample(37).cpu(), dict(dt=0.005, kT=1.0)


def _lj_case(n, dim):
    m = math.ceil(n ** (1 / dim) - 1e-9)
    L = 1.1 * m
    grid = torch.stack(torch.meshgrid(*[torch.arange(m, dtype=torch.float32)] * dim, indexing="ij"), -1)
    lat = grid.reshape(-1, dim)[:n] * 1.1 - L / 2 + 0.55
    g = torch.Generator().manual_seed(100 + n)
    x = lat + 0.03 * torch.randn(37, n, dim, generator=g)
    return systems.LJ(boxlength=L, cutoff=1.6, device=DEV), x, dict(dt=0.002, kT=1.0)


def _eam_case(n):
    if n == 54:
        tab = et.fs(scale=0.61 * 3 * A_FE / 3.7, rho_max=900.0)
        box, pos = 3 * A_FE, et.bcc(3, A_FE, jitter=0.08, seed=54, batch=37)
    else:
        tab = et.fs(rho_max=400.0)
        box = tab["rc"] / 0.61
        pos = lattice(n, 37, box, 1000 + n)
    return systems.EAM(tab, box, device=DEV), torch.as_tensor(pos, dtype=torch.float32), dict(dt=0.01, kT=0.05)


CASES = {}
for _d, _box in ((3, False), (15, True), (96, False), (96, True), (130, False), (130, True), (3, True),
                 (15, False)):
    _natoms, _dim = {3: (1, 3), 15: (5, 3), 96: (32, 3), 130: (65, 2)}[_d]
    CASES["einstein_D%d_%s" % (_d, "box" if _box else "nobox")] = (_einstein_case, (_natoms, _dim, _box))
for _n in (1, 5, 70):
    for _dim in (2, 3):
        CASES["gmix_n%d_d%d" % (_n, _dim)] = (_gmix_case, (_n, _dim))
for _n in (2, 5, 32, 64, 65, 130, 256):
    for _dim in (2, 3):
        CASES["lj_n%d_d%d" % (_n, _dim)] = (_lj_case, (_n, _dim))
for _n in (2, 54, 70, 130):
    CASES["eam_n%d" % _n] = (_eam_case, (_n,))


def _padded(t):
    """t as a column slice of rows 3 floats wider, in t's shape."""
    flat = t.reshape(t.shape[0], -1)
    wide = torch.full((flat.shape[0], flat.shape[1] + 3), float("nan"), device=t.device)
    wide[:, :flat.shape[1]] = flat
    return wide[:, :flat.shape[1]].view(t.shape)


def _run(sim, x, v, nsteps, fused, monkeypatch, **kw):
    """(x, v, pot[, frames, pots]) of one langevin call on the chosen path."""
    sim.fused_dynamics = fused
    sim.set_velocity(v)
    with monkeypatch.context() as m:
        if fused:
            fused_only(sim, m)
            got = []
            n = counts_of(lambda: got.extend(sim.langevin(nsteps, init_pos=x, **kw)))
            assert sum(c for k, c in n.items() if k.endswith("_langevin")) >= 1, n
        else:
            got = list(sim.langevin(nsteps, init_pos=x, **kw))
    sim.fused_dynamics = True
    return [got[0], sim.get_velocity()] + got[1:]


@pytest.mark.parametrize("case", sorted(CASES))
def test_one_launch_equals_the_per_step_path_bitwise(case, hip_device, monkeypatch):
    make, args = CASES[case]
    sim, x37, kw = make(*args)
    combos = [(rows, nsteps, zm, rec) for rows in (1, 37) for nsteps in (0, 1, 7) for zm in (False, True)
              for rec in (0, 1, 3)] + [(500, 7, zm, 3) for zm in (False, True)]
    for rows, nsteps, zm, rec in combos:
        x = _tile(x37, rows).to(DEV)
        if rows == 37:
            x = _padded(x)  # padded row strides
        what = "%s rows %d nsteps %d zero_momentum %s record_every %d" % (case, rows, nsteps, zm, rec)
        run_kw = dict(seed=1234, zero_momentum=zm, record_every=rec, step0=2, row_base=5, **kw)
        # the velocities are drawn (tag 1) once and given to both paths, padded like x
        v = math.sqrt(kw["kT"]) * rng.philox_normal(77, rows, *sim._lv_nd(x), step=0, tag=1, zero_mean=zm,
                                                    device=DEV).reshape(x.shape)
        if rows == 37:
            v = _padded(v)
        one = _run(sim, x, v, nsteps, True, monkeypatch, **run_kw)
        per = _run(sim, x, v, nsteps, False, monkeypatch, **run_kw)
        assert len(one) == len(per) == (5 if rec else 3), what
        for a, b, name in zip(one, per, ("x", "v", "potential", "frames", "frame potentials")):
            assert a.shape == b.shape and a.dtype == torch.float32, (what, name, a.shape, b.shape)
            assert torch.isfinite(b).all(), (what, name)
            assert torch.equal(a, b), (what, name, float((a - b).abs().max()))
        assert one[0].shape == x.shape and one[2].shape == (rows,), what
        if rec:
            nf = (2 + nsteps) // rec - 2 // rec
            assert one[3].shape == (nf,) + x.shape and one[4].shape == (nf, rows), what
        if nsteps == 0:
            assert torch.equal(one[0], x) and torch.equal(one[1], v), what


def test_a_missing_velocity_is_drawn_the_same_on_both_paths(hip_device, monkeypatch):
    sim, x, kw = _lj_case(33, 3)
    x = x.to(DEV)
    for zm in (True, False):
        one = _run(sim, x, None, 3, True, monkeypatch, seed=9, zero_momentum=zm, **kw)
        per = _run(sim, x, None, 3, False, monkeypatch, seed=9, zero_momentum=zm, **kw)
        assert torch.equal(one[0], per[0]) and torch.equal(one[1], per[1])
        sim.set_velocity(None)
        sim.langevin(0, init_pos=x, seed=9, zero_momentum=zm, **kw)
        v0 = sim.get_velocity()
        want = rng.philox_normal(9, 37, 33, 3, step=0, tag=1, zero_mean=zm, device=DEV)
        assert torch.equal(v0, float(np.float32(math.sqrt(kw["kT"]))) * want)


# -------------------------------------------------------------- chunking and geometry
@pytest.mark.parametrize("case", ["einstein_D130_box", "gmix_n70_d3", "lj_n65_d3", "eam_n54"])
def test_chunks_and_row_blocks_join_bitwise(case, hip_device, monkeypatch):
    make, args = CASES[case]
    sim, x, kw = make(*args)
    x = x.to(DEV)
    n, dim = sim._lv_nd(x)
    v = rng.philox_normal(3, 37, n, dim, step=0, tag=1, device=DEV).reshape(x.shape)
    kw = dict(seed=21, zero_momentum=True, **kw)
    whole = _run(sim, x, v, 11, True, monkeypatch, record_every=2, **kw)
    # 4 + 7 with step0 carried
    first = _run(sim, x, v, 4, True, monkeypatch, **kw)
    second = _run(sim, first[0], first[1], 7, True, monkeypatch, step0=4, **kw)
    for a, b in zip(whole[:3], second):
        assert torch.equal(a, b)
    # the launch cap
    monkeypatch.setattr(config, "LANGEVIN_STEPS_PER_LAUNCH", 3)
    got = []
    sim.set_velocity(v)
    counts = counts_of(lambda: got.extend(sim.langevin(11, init_pos=x, record_every=2, **kw)))
    assert sum(c for k, c in counts.items() if k.endswith("_langevin")) == 4, counts
    for a, b in zip(whole, [got[0], sim.get_velocity()] + got[1:]):
        assert torch.equal(a, b)
    monkeypatch.undo()
    # rows over two calls with row_base
    lo = _run(sim, x[:20], v[:20], 11, True, monkeypatch, record_every=2, **kw)
    hi = _run(sim, x[20:], v[20:], 11, True, monkeypatch, record_every=2, row_base=20, **kw)
    for a, l, h in zip(whole, lo, hi):
        assert torch.equal(a, torch.cat((l, h), dim=0 if a.shape[0] == 37 else 1))


# -------------------------------------------------------------------- against fp64
def test_lj32_against_the_fp64_per_step_run(hip_device, monkeypatch):
    x0, _ = fcc32_state()
    lj = systems.LJ(boxlength=L32, cutoff=1.6, device=DEV)
    v0 = rng.philox_normal(1, 16, 32, 3, step=0, tag=1, zero_mean=True, device=DEV)
    kw = dict(dt=0.002, seed=4, kT=1.0)
    x, v, pot = _run(lj, x0.to(DEV), v0, 7, True, monkeypatch, **kw)
    x64, v64, _ = _run(lj, x0.double().to(DEV), v0.double(), 7, False, monkeypatch, **kw)
    assert x64.dtype == torch.float64
    for ours, want, what in ((x, x64, "x"), (v, v64, "v")):
        print("LJ-32 %s after 7 steps: max error against fp64 %.3g" % (what, float((ours.double() - want).abs().max())))
        torch.testing.assert_close(ours.double().cpu(), want.cpu(), rtol=1e-5, atol=1e-4)
    close_or_on_par(pot, lj_f64(x.cpu())[0], lj_f64(x.cpu().double())[0], "LJ-32 potential at x_out")


def test_fe54_against_the_fp64_per_step_run(hip_device, monkeypatch):
    eam, x0, kw = _eam_case(54)
    x0 = x0[:5].to(DEV)
    v0 = math.sqrt(0.05) * rng.philox_normal(1, 5, 54, 3, step=0, tag=1, zero_mean=True, device=DEV)
    kw = dict(seed=4, **kw)
    x, v, pot = _run(eam, x0, v0, 7, True, monkeypatch, **kw)
    cpu = systems.EAM(eam.table, eam.boxlength)
    res = {}
    for dtype in (torch.float32, torch.float64):  # the module's CPU path: the same words, from the restatement
        cpu.set_velocity(v0.cpu().to(dtype))
        xs, ps = cpu.langevin(7, init_pos=x0.cpu().to(dtype), **kw)
        res[dtype] = (xs, cpu.get_velocity(), ps)
    for ours, i, what in ((x, 0, "x"), (v, 1, "v"), (pot, 2, "potential")):
        eam_close_or_on_par(ours, res[torch.float32][i], res[torch.float64][i], "Fe-54 " + what)


# ------------------------------------------------------------------------- physics
def test_einstein_crystal_samples_its_gaussian(hip_device, monkeypatch):
    """BAOAB samples a harmonic configuration exactly: the position variance per
    coordinate is kT scale^2 = kT / alpha.  4,096 x 96 = 3.9e5 samples, each a
    chain of its own: the relative standard error of the variance is sqrt(2 / N) =
    0.23 %, and 1.1 % is 5 sigma."""
    alpha, kT, rows = 100.0, 0.8, 4096
    g = torch.Generator().manual_seed(3)
    centers = (torch.rand(32, 3, generator=g) - 0.5) * L32
    sim = systems.EinsteinCrystal(centers, 3, boxlength=None, alpha=alpha, device=DEV)
    x0 = centers.flatten().expand(rows, 96).contiguous().to(DEV)
    kw = dict(dt=0.005, kT=kT, seed=31)
    x, v, _ = _run(sim, x0, None, 600, True, monkeypatch, **kw)  # 200 of burn-in and 400
    var = float(((x - sim.centers.flatten()).double() ** 2).mean())
    print("Einstein position variance %.6g, expected %.6g (ratio %.5f)" % (var, kT / alpha, var * alpha / kT))
    assert abs(var * alpha / kT - 1) < 0.011
    # the fp64 per-step run on the same words: the dynamics contract, rounding does not grow
    sim64 = systems.EinsteinCrystal(centers.double(), 3, boxlength=None, alpha=alpha, device=DEV)
    sub = 256
    x64, v64, _ = _run(sim64, x0[:sub].double(), None, 600, False, monkeypatch, **kw)
    for ours, want, spread, what in ((x[:sub], x64, math.sqrt(kT / alpha), "x"), (v[:sub], v64, math.sqrt(kT), "v")):
        err = float((ours.double() - want).abs().max())
        print("Einstein %s after 600 steps: max error against fp64 %.3g (thermal spread %.3g)" % (what, err, spread))
        torch.testing.assert_close(ours.double(), want, rtol=1e-4, atol=1e-4 * spread)


def _lj_thermal(zero_momentum, monkeypatch):
    x16, _ = fcc32_state()
    lj = systems.LJ(boxlength=L32, cutoff=1.6, device=DEV)
    x0 = _tile(x16, 256).to(DEV)
    out = _run(lj, x0, None, 2500, True, monkeypatch, dt=0.002, kT=1.0, seed=13, zero_momentum=zero_momentum)
    assert torch.isfinite(out[0]).all()
    return out[1].double()


def test_lj_kinetic_energy_and_momentum(hip_device, monkeypatch):
    """(n - 1) dim / 2 kT with the momentum constrained.  A row's kinetic energy is
    kT / 2 times a chi-square of 93 degrees: 14.7 % relative spread, 0.92 % over 256
    rows, so 5 sigma is 4.6 %; BAOAB's O(dt^2) bias at dt 0.002 is far below that."""
    v = _lj_thermal(True, monkeypatch)
    ke = float((0.5 * v ** 2).sum((1, 2)).mean())
    want = 31 * 3 / 2
    print("LJ-32 mean kinetic energy %.4f, expected %.4f (ratio %.4f)" % (ke, want, ke / want))
    assert abs(ke / want - 1) < 0.05
    p = float(v.sum(1).abs().max())
    print("LJ-32 largest total-momentum component %.3g" % p)
    assert p < 1e-4


def test_lj_centre_of_mass_is_thermal_without_zero_momentum(hip_device, monkeypatch):
    """var(v_com) = kT / n per component; 256 x 3 samples: sqrt(2 / 768) = 5.1 %,
    5 sigma = 26 %."""
    v = _lj_thermal(False, monkeypatch)
    var = float((v.mean(1) ** 2).mean())
    print("LJ-32 centre-of-mass velocity variance %.5f, expected %.5f" % (var, 1 / 32))
    assert abs(var * 32 - 1) < 0.26


# -------------------------------------------------------------------------- errors
def test_bad_arguments_never_reach_the_device(hip_device):
    sim, x, kw = _lj_case(5, 3)
    x = x.reshape(37, -1).to(DEV)
    v = torch.zeros_like(x)
    out = torch.empty_like(x), torch.empty_like(v), torch.empty(37, device=DEV)
    ok = dict(nsteps=2, consts=(1e-3, 1e-3, 0.9, 0.1), seed=1, n=5, dim=3, **sim._kw())
    K_.lj_langevin(x, v, *out, **ok)
    rec = torch.empty(2, 37, 15, device=DEV), torch.empty(2, 37, device=DEV)
    for bad, msg in ((dict(nsteps=-1), "nsteps below zero"),
                     (dict(record_every=1, pos_rec=rec[0]), "pos_rec and pot_rec come together"),
                     (dict(record_every=1, pot_rec=rec[1]), "pos_rec and pot_rec come together"),
                     (dict(seed=1 << 63), "seed must be in"),
                     (dict(seed=(1 << 64) - 1), "seed must be in"),
                     (dict(step0=-1), "step below zero"),
                     (dict(row_base=1 << 32), "row_base \\+ rows must stay below 2\\^32"),
                     (dict(record_every=-1), "record_every below zero")):
        with pytest.raises(ValueError, match="nfk_lj_langevin: " + msg):
            K_.lj_langevin(x, v, *out, **{**ok, **bad})
    big = torch.zeros(2, 900, device=DEV)
    with pytest.raises(ValueError, match="not supported"):
        K_.lj_langevin(big, big, torch.empty_like(big), torch.empty_like(big), torch.empty(2, device=DEV),
                       **{**ok, "n": 300})
    e5 = systems.EinsteinCrystal(torch.zeros(3, 5), 5, device=DEV)
    z = torch.zeros(2, 15, device=DEV)
    with pytest.raises(ValueError, match="not supported"):
        K_.einstein_langevin(z, z, torch.empty_like(z), torch.empty_like(z), torch.empty(2, device=DEV), e5.centers,
                             nsteps=1, consts=ok["consts"], seed=1, scale=1.0, hld=0.0)
    with pytest.raises(ValueError, match="nfk_philox_fill"):
        K_.philox_fill(torch.empty(1, 1, 4, dtype=torch.int32, device=DEV), n=1, dim=4, step=0, seed=1 << 63,
                       normals=False)
    # langevin on shapes the kernels do not take runs the per-step path
    xb = (torch.rand(2, 300, 3, device=DEV) - 0.5) * 8.0
    lj = systems.LJ(boxlength=8.0, cutoff=1.6, device=DEV)
    lj.set_velocity(torch.zeros_like(xb))
    n = counts_of(lambda: lj.langevin(1, dt=1e-5, init_pos=xb, kT=1e-6))
    assert not any(k.endswith("_langevin") for k in n) and n.get("nfk_philox_fill") == 1, n
