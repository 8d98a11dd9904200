"""Hamiltonian switching on the device (nfk_switch.hip, systems.Switch): one launch
against the per-step path bit for bit (x, v, energies, work, frames and frame
energies) at every mapping, the lam = 1 and lam = 0 limits against the existing
Langevin kernels, chunks and row blocks, fp64 restatements, Crooks consistency of
the work values, and the argument checks."""
import itertools
import math

import pytest
import torch

from normalizingflow_amd import bar, config, rng, systems
from normalizingflow_amd import kernels as K_
from test_dynamics_cpu import L32, fcc32_state, lj_f64
from test_gpu_dynamics import fused_only
from test_gpu_eam import close_or_on_par as eam_close_or_on_par
from test_gpu_langevin import CASES, _eam_case, _lj_case, _padded, _tile
from test_gpu_systems import ATOL, RTOL, close_or_on_par, counts_of

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
ALPHA = 600  # the Einstein crystal of test_gpu_langevin's own Einstein case
SWITCH_CASES = sorted(c for c in CASES if c.startswith(("lj_", "eam_")))
# indexed by the absolute step; the runs below start at step0 = 2 and take up to 7 steps
RAMP = torch.linspace(0, 1, 10)
FLAT = torch.tensor([0.0, 0.1, 0.2, 0.35, 0.35, 0.35, 0.35, 0.6, 0.8, 1.0])  # steps 3-5 skip the energies


def _switch_case(case, box=False, kT=None):
    """(Switch, x37 on the CPU, dt) of a Langevin case of test_gpu_langevin: its target,
    an Einstein crystal centred on the case's first configuration (with the target's
    box when ``box``), the case's kT."""
    make, args = CASES[case]
    sim, x37, kw = make(*args)
    n, dim = x37.shape[-2:]
    L = sim.boxlength
    A = systems.EinsteinCrystal(x37[0].clone(), dim, boxlength=L if box else None, alpha=ALPHA, device=DEV)
    if box:  # some coordinates one box away: the Einstein wrap fires (LJ and EAM wrap pair vectors anyway)
        g = torch.Generator().manual_seed(3 + n)
        x37 = x37 + (torch.rand(x37.shape, generator=g) < 0.05) * L
    return systems.Switch(A, sim, kT=kw["kT"] if kT is None else kT), x37, kw["dt"]


def _run(sw, lam, x, v, nsteps, fused, monkeypatch, **kw):
    """[x, v, work, energies(, frames, frame energies)] of one switch call on the chosen path."""
    sw.fused_dynamics = fused
    sw.set_velocity(v)
    with monkeypatch.context() as m:
        if fused:
            fused_only(sw.reference, m)
            fused_only(sw.target, m)
            got = []
            n = counts_of(lambda: got.extend(sw.switch(lam, nsteps=nsteps, init_pos=x, **kw)))
            assert sum(c for k, c in n.items() if k.endswith("_switch")) >= 1, n
            assert all(k.endswith("_switch") or k == "nfk_philox_fill" for k in n), n
        else:
            got = list(sw.switch(lam, nsteps=nsteps, init_pos=x, **kw))
    sw.fused_dynamics = True
    return [got[0], sw.get_velocity()] + got[1:]


NAMES = ("x", "v", "work", "energies", "frames", "frame energies")


# ------------------------------------------------- one launch against the per-step path
@pytest.mark.parametrize("case", SWITCH_CASES)
def test_one_launch_equals_the_per_step_path_bitwise(case, hip_device, monkeypatch):
    """Every combination of rows, nsteps, record_every, Einstein box, zero_momentum and
    schedule (144 per case; the per-step side of the longest is 7 steps of 37 rows)."""
    built = {box: _switch_case(case, box) for box in (False, True)}
    for rows, nsteps, rec, box, zm, lam in itertools.product((1, 37), (0, 1, 7), (0, 1, 3), (False, True),
                                                             (False, True), (RAMP, FLAT)):
        sw, x37, dt = built[box]
        x = _tile(x37, rows).to(DEV)
        nd = x.shape[-2:]
        v = math.sqrt(sw.kT) * rng.philox_normal(77, rows, *nd, step=0, tag=1, zero_mean=zm, device=DEV)
        if rows == 37:
            x, v = _padded(x), _padded(v)  # padded row strides
        what = "%s rows %d nsteps %d record_every %d box %s zero_momentum %s %s" % (
            case, rows, nsteps, rec, box, zm, "ramp" if lam is RAMP else "flat")
        kw = dict(dt=dt, seed=1234, zero_momentum=zm, record_every=rec, step0=2, row_base=5)
        one = _run(sw, lam, x, v, nsteps, True, monkeypatch, **kw)
        per = _run(sw, lam, x, v, nsteps, False, monkeypatch, **kw)
        assert len(one) == len(per) == (6 if rec else 4), what
        for a, b, name in zip(one, per, NAMES):
            assert a.shape == b.shape and a.dtype == b.dtype, (what, name, a.shape, b.shape)
            assert torch.isfinite(b).all(), (what, name)
            assert torch.equal(a, b), (what, name, float((a - b).abs().max()))
        assert one[0].shape == x.shape and one[2].shape == (rows,) and one[2].dtype == torch.float64, what
        assert one[3].shape == (rows, 2) and one[3].dtype == torch.float32, what
        if rec:
            nf = (2 + nsteps) // rec - 2 // rec
            assert one[4].shape == (nf,) + x.shape and one[5].shape == (nf, rows, 2), what
        if nsteps == 0:
            assert torch.equal(one[0], x) and torch.equal(one[1], v) and not one[2].any(), what
        else:
            assert one[2].abs().min() > 0, what


# ------------------------------------------------------ limits against the existing kernels
@pytest.mark.parametrize("case", ["lj_n32_d3", "lj_n65_d2", "lj_n256_d3", "eam_n54", "eam_n130"])
def test_lam_one_is_the_targets_langevin(case, hip_device, monkeypatch):
    sw, x37, dt = _switch_case(case)
    x = x37.to(DEV)
    for zm in (False, True):
        v = rng.philox_normal(5, 37, *x.shape[-2:], step=0, tag=1, zero_mean=zm, device=DEV)
        kw = dict(dt=dt, seed=9, zero_momentum=zm, step0=3)
        got = _run(sw, torch.ones(12), x, v, 7, True, monkeypatch, **kw)
        sw.target.set_velocity(v)
        xt, pot = sw.target.langevin(7, init_pos=x, kT=sw.kT, **kw)
        assert torch.equal(got[0], xt) and torch.equal(got[1], sw.target.get_velocity())
        assert torch.equal(got[3][:, 1], pot) and torch.equal(pot, sw.target.potential(xt))
        assert not got[2].any()


@pytest.mark.parametrize("case", ["lj_n32_d3", "lj_n65_d2", "lj_n256_d3", "eam_n54", "eam_n130"])
@pytest.mark.parametrize("box", [False, True])
def test_lam_zero_is_the_einstein_crystals_langevin(case, box, hip_device, monkeypatch):
    sw, x37, dt = _switch_case(case, box, kT=1.0)
    x = x37.to(DEV)
    for zm in (False, True):
        v = rng.philox_normal(5, 37, *x.shape[-2:], step=0, tag=1, zero_mean=zm, device=DEV)
        kw = dict(dt=dt, seed=9, zero_momentum=zm, step0=3)
        got = _run(sw, torch.zeros(12), x, v, 7, True, monkeypatch, **kw)
        A = sw.reference
        A.set_velocity(v.reshape(37, -1))
        xa, _ = A.langevin(7, init_pos=x.reshape(37, -1), kT=1.0, **kw)
        assert torch.equal(got[0].reshape(37, -1), xa) and torch.equal(got[1].reshape(37, -1), A.get_velocity())
        assert not got[2].any()


# -------------------------------------------------------------- chunking and geometry
@pytest.mark.parametrize("case", ["lj_n65_d3", "eam_n54"])
def test_chunks_and_row_blocks_join_bitwise(case, hip_device, monkeypatch):
    sw, x, dt = _switch_case(case, box=True)
    x = x.to(DEV)
    v = math.sqrt(sw.kT) * rng.philox_normal(3, 37, *x.shape[-2:], step=0, tag=1, device=DEV)
    lam = torch.linspace(0, 1, 12)
    kw = dict(dt=dt, seed=21)
    whole = _run(sw, lam, x, v, 11, True, monkeypatch, record_every=2, **kw)
    # 4 + 7 with step0 and the work carried
    first = _run(sw, lam, x, v, 4, True, monkeypatch, **kw)
    second = _run(sw, lam, first[0], first[1], 7, True, monkeypatch, step0=4, work=first[2], **kw)
    for a, b in zip(whole[:4], second):
        assert torch.equal(a, b)
    # the launch cap
    monkeypatch.setattr(config, "LANGEVIN_STEPS_PER_LAUNCH", 3)
    got = []
    sw.set_velocity(v)
    counts = counts_of(lambda: got.extend(sw.switch(lam, init_pos=x, record_every=2, **kw)))
    assert sum(c for k, c in counts.items() if k.endswith("_switch")) == 4, counts
    for a, b in zip(whole, [got[0], sw.get_velocity()] + got[1:]):
        assert torch.equal(a, b)
    monkeypatch.undo()
    # rows over two calls with row_base
    lo = _run(sw, lam, x[:20], v[:20], 11, True, monkeypatch, record_every=2, **kw)
    hi = _run(sw, lam, x[20:], v[20:], 11, True, monkeypatch, record_every=2, row_base=20, **kw)
    for a, l, h in zip(whole, lo, hi):
        assert torch.equal(a, torch.cat((l, h), dim=0 if a.shape[0] == 37 else 1))


# -------------------------------------------------------------------- against fp64
def _work_from_frames(lam, kT, x0, frames, u_a, u_b):
    """The work of a run from its own positions: x before step k is x0 or frame k - 1;
    ``u_a`` / ``u_b`` give the energies of [..., n, dim] positions.  Returns (work, the sum
    over the steps of |dlam| times the two energies' magnitudes (U_B over kT)), fp64."""
    pos = torch.cat((x0.unsqueeze(0), frames[:-1]))
    dl = (lam[1:].double() - lam[:-1].double()).reshape(-1, 1)
    ua, ub = u_a(pos).double(), u_b(pos).double() / kT
    return (dl * (ub - ua)).sum(0), dl.abs(), ua, ub


def _work_bound(dl, ua32, ua64, ub32, ub64):
    """sum_k |dlam_k| (tol_B + tol_A): per energy the tolerance close_or_on_par grants,
    rtol 1e-5 / atol 1e-4 or twice the fp32 restatement's own largest error."""
    tol_a = torch.maximum(ATOL + RTOL * ua64.abs(), 2 * (ua32 - ua64).abs().max() + 1e-6)
    tol_b = torch.maximum(ATOL + RTOL * ub64.abs(), 2 * (ub32 - ub64).abs().max() + 1e-6)
    return (dl * (tol_a + tol_b)).sum(0)


def test_lj32_against_the_fp64_per_step_run(hip_device, monkeypatch):
    x0, _ = fcc32_state()
    lat = x0.mean(0)
    A = systems.EinsteinCrystal(lat, 3, boxlength=None, alpha=ALPHA, device=DEV)
    sw = systems.Switch(A, systems.LJ(boxlength=L32, cutoff=1.6, device=DEV), kT=1.0)
    v0 = rng.philox_normal(1, 16, 32, 3, step=0, tag=1, device=DEV)
    lam = torch.linspace(0, 1, 8)
    kw = dict(dt=0.002, seed=4, record_every=1)
    x, v, w, en, frames, _ = _run(sw, lam, x0.to(DEV), v0, 7, True, monkeypatch, **kw)
    x64, v64, w64, _, _, _ = _run(sw, lam, x0.double().to(DEV), v0.double(), 7, False, monkeypatch, **kw)
    assert x64.dtype == torch.float64
    for ours, want, what in ((x, x64, "x"), (v, v64, "v")):
        print("LJ-32 switch %s after 7 steps: max error against fp64 %.3g"
              % (what, float((ours.double() - want).abs().max())))
        torch.testing.assert_close(ours.double().cpu(), want.cpu(), rtol=1e-5, atol=1e-4)
    cpu = systems.EinsteinCrystal(lat, 3, boxlength=None, alpha=ALPHA)

    def u_a(p):
        return cpu.potential(p.reshape(-1, 96)).reshape(p.shape[:-2])

    args = (lam, 1.0, x0, frames.cpu())
    wk64, dl, ua64, ub64 = _work_from_frames(*args, lambda p: u_a(p.double()), lambda p: lj_f64(p.double())[0])
    _, _, ua32, ub32 = _work_from_frames(*args, u_a, lambda p: lj_f64(p)[0])
    bound = _work_bound(dl, ua32, ua64, ub32, ub64)
    err = (w.cpu() - wk64).abs()
    print("LJ-32 work: max error against fp64 of the kernel's own frames %.3g (bound %.3g); |w| up to %.3g; "
          "against the fp64 run %.3g" % (float(err.max()), float(bound.min()), float(w.abs().max()),
                                         float((w - w64).abs().max())))
    assert (err <= bound).all(), (err, bound)
    close_or_on_par(en[:, 0], u_a(x.cpu()), u_a(x.cpu().double()), "u_A at x_out")
    close_or_on_par(en[:, 1], lj_f64(x.cpu())[0], lj_f64(x.cpu().double())[0], "U_B at x_out")


def test_fe54_against_the_fp64_per_step_run(hip_device, monkeypatch):
    sw, x37, dt = _switch_case("eam_n54")
    x0 = x37[:5].to(DEV)
    v0 = math.sqrt(0.05) * rng.philox_normal(1, 5, 54, 3, step=0, tag=1, device=DEV)
    lam = torch.linspace(0, 1, 8)
    kw = dict(dt=dt, seed=4, record_every=1)
    x, v, w, en, frames, _ = _run(sw, lam, x0, v0, 7, True, monkeypatch, **kw)
    cpu = systems.Switch(systems.EinsteinCrystal(x37[0].clone(), 3, alpha=ALPHA),
                         systems.EAM(sw.target.table, sw.target.boxlength), kT=sw.kT)
    res = {}
    for dtype in (torch.float32, torch.float64):  # the module's CPU path: the same words, from the restatement
        cpu.set_velocity(v0.cpu().to(dtype))
        out = cpu.switch(lam, init_pos=x0.cpu().to(dtype), **kw)
        res[dtype] = (out[0], cpu.get_velocity(), out[2][:, 0], out[2][:, 1])
    for ours, i, what in ((x, 0, "x"), (v, 1, "v"), (en[:, 0], 2, "u_A"), (en[:, 1], 3, "U_B")):
        eam_close_or_on_par(ours, res[torch.float32][i], res[torch.float64][i], "Fe-54 switch " + what)

    def u_a(p):
        return cpu.reference.potential(p.reshape(-1, 162)).reshape(p.shape[:-2])

    args = (lam, sw.kT, x0.cpu(), frames.cpu())
    wk64, dl, ua64, ub64 = _work_from_frames(*args, lambda p: u_a(p.double()),
                                             lambda p: cpu.target.potential(p.double()))
    _, _, ua32, ub32 = _work_from_frames(*args, u_a, cpu.target.potential)
    bound = _work_bound(dl, ua32, ua64, ub32, ub64)
    err = (w.cpu() - wk64).abs()
    print("Fe-54 work: max error against fp64 of the kernel's own frames %.3g (bound %.3g); |w| up to %.3g"
          % (float(err.max()), float(bound.min()), float(w.abs().max())))
    assert (err <= bound).all(), (err, bound)


# ------------------------------------------------------------------------- physics
def _crooks(rows, nsteps, device, dtype, equil=200):
    """Forward and reverse work between the Einstein crystal (alpha 600) on the fcc
    lattice of 32 and LJ-32 at kT = 1, dt = 0.002 (the Langevin LJ case's): both ways
    start from samples of the crystal and take ``equil`` steps at their own end
    state first."""
    basis = [(0, 0, 0), (.5, .5, 0), (.5, 0, .5), (0, .5, .5)]
    pts = [((i + b[0]) / 2, (j + b[1]) / 2, (k + b[2]) / 2)
           for i in range(2) for j in range(2) for k in range(2) for b in basis]
    lat = (torch.tensor(pts, dtype=torch.float64) * L32 - L32 / 2 + L32 / 8).float()
    A = systems.EinsteinCrystal(lat, 3, boxlength=None, alpha=ALPHA, device=device)
    sw = systems.Switch(A, systems.LJ(boxlength=L32, cutoff=1.6, device=device), kT=1.0)
    g = torch.Generator().manual_seed(77)
    x0 = (lat + torch.randn(2, rows, 32, 3, generator=g) / math.sqrt(ALPHA)).to(device=device, dtype=dtype)
    ramp = torch.linspace(0, 1, nsteps + 1)
    out = []
    for x, lam, seed in ((x0[0], torch.cat((torch.zeros(equil), ramp)), 31),
                         (x0[1], torch.cat((torch.ones(equil), ramp.flip(0))), 32)):
        sw.set_velocity(None)
        out.append(sw.switch(lam, init_pos=x, dt=0.002, seed=seed)[1])
    return out


def test_crooks_consistency_of_the_work_values(hip_device):
    """BAR over 512 + 512 trajectories at 64 and at 512 switching steps estimates one
    free-energy difference, and slower switching dissipates less.  The same protocol on
    the fp64 CPU path at 64 rows gave BAR 151.30 +- 0.46 (64 steps) and 151.17 +- 0.46
    (512 steps), mean dissipation 48.7 and 12.7."""
    res = {}
    for nsteps in (64, 512):
        w_f, w_r = _crooks(512, nsteps, DEV, torch.float32)
        assert w_f.dtype == torch.float64 and torch.isfinite(w_f).all() and torch.isfinite(w_r).all()
        est = float(bar.bar_solve(w_f.cpu(), w_r.cpu())[0][0, 0])
        sd = float(bar.bootstrap(w_f.float(), w_r.float(), 200,
                                 generator=torch.Generator(DEV).manual_seed(1))[:, 0].std())
        res[nsteps] = (est, sd, float(w_f.mean() + w_r.mean()))
        print("Crooks LJ-32, %d steps: BAR %.3f +- %.3f, mean dissipation %.3f" % ((nsteps,) + res[nsteps]))
    assert abs(res[64][0] - res[512][0]) <= 4 * math.hypot(res[64][1], res[512][1]), res
    assert 0 < res[512][2] < res[64][2], res


# -------------------------------------------------------------------------- edges
def test_zero_steps_and_the_empty_batch(hip_device, monkeypatch):
    sw, x37, dt = _switch_case("lj_n5_d3")
    x = x37.to(DEV)
    v = torch.randn_like(x)
    got = _run(sw, [0.0, 1.0], x, v, 0, True, monkeypatch, dt=dt)
    assert torch.equal(got[0], x) and torch.equal(got[1], v) and not got[2].any()
    u_a, u_b = sw.energies(x)
    assert torch.equal(got[3], torch.stack((u_a, u_b), -1))
    assert torch.equal(u_b, sw.target.potential(x))
    close_or_on_par(u_a, sw.reference.potential(x.reshape(37, -1)),
                    sw.reference._log_prob_torch(x.double().reshape(37, -1)).neg().cpu(), "u_A")
    empty = x[:0]
    out = _run(sw, torch.linspace(0, 1, 4), empty, empty.clone(), 3, True, monkeypatch, dt=dt, record_every=1)
    assert out[0].shape == (0, 5, 3) and out[2].shape == (0,) and out[3].shape == (0, 2)
    assert out[4].shape == (3, 0, 5, 3) and out[5].shape == (3, 0, 2)


def test_bad_arguments_never_reach_the_device(hip_device):
    sim, x, kw = _lj_case(5, 3)
    x = x.reshape(37, -1).to(DEV)
    v = torch.zeros_like(x)
    A = systems.EinsteinCrystal(torch.zeros(5, 3), 3, alpha=ALPHA, device=DEV)
    out = torch.empty_like(x), torch.empty_like(v), torch.empty(37, 2, device=DEV)
    lam = torch.linspace(0, 1, 4, device=DEV)
    scale, hld = A._consts()
    ok = dict(nsteps=2, consts=(1e-3, 1e-3, 0.9, 0.1), seed=1, kT=1.0, n=5, dim=3, scale=scale, hld=hld, **sim._kw())
    work = torch.zeros(37, dtype=torch.float64, device=DEV)
    K_.lj_switch(x, v, *out, A.centers, lam, work=work, **ok)
    assert work.abs().min() > 0
    four = systems.EinsteinCrystal(torch.zeros(4, 3), 3, device=DEV).centers
    flat2 = torch.zeros(5, 2, device=DEV)
    for bad, centers, sched, msg in (
            (dict(), A.centers, None, "null schedule"),
            (dict(nsteps=4), A.centers, lam, "the schedule is too short"),
            (dict(step0=2), A.centers, lam, "the schedule is too short"),
            (dict(), four, lam, "the Einstein crystal's natoms must equal n"),
            (dict(), flat2, lam, "the Einstein crystal's dim must equal the target's"),
            (dict(nsteps=-1), A.centers, lam, "nsteps below zero"),
            (dict(seed=1 << 63), A.centers, lam, "seed must be in"),
            (dict(row_base=1 << 32), A.centers, lam, "row_base \\+ rows must stay below 2\\^32"),
            (dict(record_every=1, pos_rec=torch.empty(2, 37, 15, device=DEV)), A.centers, lam,
             "pos_rec and en_rec come together")):
        with pytest.raises(ValueError, match="nfk_lj_switch: " + msg):
            K_.lj_switch(x, v, *out, centers, sched, **{**ok, **bad})
    eam, xe, _ = _eam_case(2)
    xe = xe.reshape(37, -1).to(DEV)
    oute = torch.empty_like(xe), torch.empty_like(xe), torch.empty(37, 2, device=DEV)
    oke = dict(nsteps=2, consts=ok["consts"], seed=1, kT=1.0, n=2, scale=scale, hld=hld, **eam._kw(DEV))
    for shape, sched, msg in (((2, 3), lam[:2], "the schedule is too short"),
                              ((3, 3), lam, "the Einstein crystal's natoms must equal n"),
                              ((2, 2), lam, "the Einstein crystal's dim must equal the target's")):
        centers = torch.zeros(shape, device=DEV)
        with pytest.raises(ValueError, match="nfk_eam_switch: " + msg):
            K_.eam_switch(xe, xe, *oute, centers, sched, **oke)
    # a pair the kernels do not take runs the per-step path
    sw = systems.Switch(A, systems.EinsteinCrystal(torch.zeros(5, 3), 3, alpha=100, device=DEV))
    sw.set_velocity(None)
    cnt = counts_of(lambda: sw.switch([0.0, 1.0], init_pos=0.1 * torch.randn(4, 15, device=DEV)))
    assert not any(k.endswith("_switch") for k in cnt), cnt
