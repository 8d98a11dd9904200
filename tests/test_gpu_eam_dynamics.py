"""GPU checks of EAM dynamics in one launch (nfk_eam_trajectory of
nfk_dynamics.hip, nfk_eam_hmc_run of nfk_hmc_run.hip): bit for bit against the
per-step path on nfk_eam.hip's force and energy kernels at every mapping of
the row (lane groups of 1..64, one to four atoms per lane), against the
module's fp64 path, in strided, misaligned and aliased layouts, past the grid
cap, as whole HMC runs against the per-epoch kernels fed the same draws, and
through the application functions.

Tables and rows are those of tests/test_gpu_eam.py (``case``, ``lattice``).
"""
import numpy as np
import pytest
import torch

import eam_tables as et
from nf.hmc import HMC
from normalizingflow_amd import app, systems
from normalizingflow_amd import kernels as K_
from test_gpu_dynamics import fused_only
from test_gpu_eam import case, close_or_on_par, lattice
from test_gpu_hmc_run import assert_same, draws, one_launch, per_epoch_loop, restated_decisions, run_launches
from test_gpu_systems import counts_of

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
DT = 0.01
CHAINS, EPOCHS, PATH = 37, 6, 5
BETA, HMC_DT = 20.0, 0.02
GRID_CAP = 16384  # blocks of an nfk_eam_trajectory / nfk_eam_hmc_run launch

NAMED = ["n1_self_images", "n3_idle_lane", "n16_ragged", "n54_fe", "n64_full_wave", "n65_two_per_lane",
         "n5_orthorhombic", "n2_orthorhombic_two_shifts", "n16_rho_beyond_table"]
OWN = {"n130_three_per_lane": 130, "n200_four_per_lane": 200}


def rows_of(name):
    """(table, box, positions [B, n, 3] fp64): test_gpu_eam's case, or one of the
    two here by the same recipe, 3 rows of 130 and 200 atoms."""
    if name in OWN:
        tab = et.fs(rho_max=400.0)
        L = tab["rc"] / 0.61
        return tab, L, lattice(OWN[name], 3, L, 1000 + OWN[name])
    return case(name)


def state(name, vscale=0.3):
    tab, box, pos = rows_of(name)
    x = torch.as_tensor(pos, dtype=torch.float32)
    v = vscale * torch.randn(x.shape, generator=torch.Generator().manual_seed(x.shape[1]))
    return systems.EAM(tab, box, device=DEV), x.to(DEV), v.to(DEV)


# ------------------------------------------------- 1. bitwise against the per-step path
@pytest.mark.parametrize("scheme", ["reference", "verlet"])
@pytest.mark.parametrize("name", NAMED + sorted(OWN))
def test_fused_equals_per_step_bitwise(name, scheme, hip_device):
    eam, x, v = state(name)
    for rows in sorted({1, x.shape[0]}):
        x0, v0 = x[:rows], v[:rows]
        for P in (0, 1, 12):
            what = "%s %s rows %d path_len %d" % (name, scheme, rows, P)
            got = []
            eam.fused_dynamics = True
            n = counts_of(lambda: got.extend(eam.integration_step(P, DT, x0, v0, scheme=scheme)))
            assert n == {"nfk_eam_trajectory": 1}, (what, n)
            xf, potf = got
            vf, ff = eam.get_velocity(), eam.last_force
            assert xf is eam.get_position() and xf.shape == x0.shape and vf.shape == x0.shape
            eam.fused_dynamics = False
            xs, pots = eam.integration_step(P, DT, x0, v0, scheme=scheme)
            vs, fs = eam.get_velocity(), eam.last_force
            assert torch.isfinite(xs).all() and torch.isfinite(vs).all() and torch.isfinite(pots).all(), what
            assert torch.equal(xf, xs) and torch.equal(vf, vs), what
            assert torch.equal(ff, fs), what
            assert potf.shape == (rows,) and torch.equal(potf, pots), what
            # the closing sum is the energy kernel's own
            assert torch.equal(potf, eam.potential(xf)), what
            if x.shape[1] == 1:  # self images exert no force: x moves by v dt alone
                assert torch.equal(ff, torch.zeros_like(ff)) and torch.equal(vf, v0), what
                want = x0
                for _ in range(P):
                    want = want + v0 * DT
                assert torch.equal(xf, want), what


# ------------------------------------------------------------------ 2. against fp64
_CPU = {}


def cpu_trajectory(dt, scheme):
    """The module's CPU path on n54_fe from v0 = randn, fp32 and fp64, computed once."""
    key = (dt, scheme)
    if key not in _CPU:
        tab, box, pos = case("n54_fe")
        v0 = torch.randn(pos.shape, generator=torch.Generator().manual_seed(54), dtype=torch.float64)
        cpu = systems.EAM(tab, box)
        res = {}
        for dtype in (torch.float32, torch.float64):
            x, pot = cpu.integration_step(12, dt, torch.as_tensor(pos, dtype=dtype), v0.to(dtype), scheme=scheme)
            res[dtype] = (x, cpu.get_velocity(), pot)
        _CPU[key] = (tab, box, pos, v0, res)
    return _CPU[key]


@pytest.mark.parametrize("scheme", ["reference", "verlet"])
@pytest.mark.parametrize("dt", [0.01, 0.02])
def test_against_fp64(dt, scheme, hip_device, monkeypatch):
    """12 steps of n54_fe with the per-step path forbidden.  The fp32 CPU path is
    the reference and the fp64 CPU path the truth (close_or_on_par).  On the CPU the
    fp32 path's own error against fp64 is at most 2.6e-6 in x, 2.3e-6 in v and 1.1e-4
    in a potential of -823 while atoms move up to 0.83, so the reference sits inside
    rtol 1e-5 / atol 1e-4 with room."""
    tab, box, pos, v0, res = cpu_trajectory(dt, scheme)
    eam = systems.EAM(tab, box, device=DEV)
    fused_only(eam, monkeypatch)
    x, pot = eam.integration_step(12, dt, torch.as_tensor(pos, dtype=torch.float32, device=DEV),
                                  v0.float().to(DEV), scheme=scheme)
    for ours, i, what in ((x, 0, "x"), (eam.get_velocity(), 1, "v"), (pot, 2, "potential")):
        close_or_on_par(ours, res[torch.float32][i], res[torch.float64][i], "n54_fe dt %g %s %s" % (dt, scheme, what))


# ---------------------------------------------------------------------------- 3. layout
def test_strided_misaligned_and_aliased(hip_device):
    eam, x, v = state("n16_ragged")
    B, W = x.shape[0], 48
    x, v = x.reshape(B, W), v.reshape(B, W)
    kw = dict(path_len=12, dt=DT, scheme=1, n=16, **eam._kw(x.device))
    xo, vo, pot = torch.empty_like(x), torch.empty_like(v), torch.empty(B, device=DEV)
    K_.eam_trajectory(x, v, xo, vo, pot, **kw)
    assert not torch.equal(xo, x) and torch.isfinite(pot).all()

    def wide(t, pad):
        w = torch.full((B, W + pad), float("nan"), device=DEV)
        w[:, :W] = t
        return w

    def off(t):
        flat = torch.zeros(B * W + 1, device=DEV)
        flat[1:] = t.flatten()
        o = flat[1:].view(B, W)
        assert o.data_ptr() % 16 == 4
        return o

    holders = wide(x, 3), wide(v, 7)
    for xa, va in ((holders[0][:, :W], holders[1][:, :W]), (off(x), off(v))):
        xw, vw = wide(x, 5), wide(v, 1)
        pb = torch.empty(B, device=DEV)
        K_.eam_trajectory(xa, va, xw[:, :W], vw[:, :W], pb, **kw)
        assert torch.equal(xw[:, :W], xo) and torch.equal(vw[:, :W], vo) and torch.equal(pb, pot)
        assert torch.isnan(xw[:, W:]).all() and torch.isnan(vw[:, W:]).all()
        pc = torch.empty(B, device=DEV)
        K_.eam_trajectory(xa, va, xa, va, pc, **kw)  # x_out is x_in, v_out is v_in
        assert torch.equal(xa, xo) and torch.equal(va, vo) and torch.equal(pc, pot)
    for h in holders:  # the padding columns stay untouched
        assert h.stride(0) > W and torch.isnan(h[:, W:]).all()
    with pytest.raises(ValueError):
        K_.eam_trajectory(x, v, xo, vo[:, :-1], pot, **kw)


# -------------------------------------------------------------------- 4. the grid cap
def test_rows_are_independent_past_the_grid_cap(hip_device):
    """n = 64: 4 rows per block and at most GRID_CAP = 16,384 blocks per launch, so
    4 * GRID_CAP + 3 rows make the grid loop take a second pass over a ragged block.
    64 sampled rows, the last three among them, equal the same rows run alone, bit
    for bit: one Verlet step through nfk_eam_trajectory, two epochs through
    nfk_eam_hmc_run."""
    tab = et.fs(rho_max=400.0)
    L = tab["rc"] / 0.61
    eam = systems.EAM(tab, L, device=DEV)
    B, W = 4 * GRID_CAP + 3, 192
    base = torch.as_tensor(et.bcc(4, L / 4)[:64], dtype=torch.float32, device=DEV)
    gen = torch.Generator(device=DEV).manual_seed(12)
    x = (base + 0.02 * L * torch.randn(B, 64, 3, device=DEV, generator=gen)).reshape(B, W)
    v = 0.3 * torch.randn(B, W, device=DEV, generator=gen)
    idx = torch.cat((torch.randint(B, (61,), device=DEV, generator=gen), torch.arange(B - 3, B, device=DEV)))
    kw = dict(path_len=1, dt=DT, scheme=1, n=64, **eam._kw(x.device))

    def traj(x, v):
        out = torch.empty_like(x), torch.empty_like(v), torch.empty(x.shape[0], device=DEV)
        K_.eam_trajectory(x, v, *out, **kw)
        return out

    for a, b in zip(traj(x, v), traj(x[idx].contiguous(), v[idx].contiguous())):
        assert torch.isfinite(a).all() and torch.equal(a[idx], b)

    u0 = torch.empty(B, device=DEV)
    K_.eam_potential(x, u0, n=64, **eam._kw(x.device))
    vd = 0.3 * torch.randn(2, B, W, device=DEV, generator=gen)
    r = torch.rand(2, B, device=DEV, generator=gen)

    def run(x, u, vd, r):
        x, u = x.clone(), u.clone()
        nacc, vl = torch.zeros(x.shape[0], dtype=torch.int32, device=DEV), torch.empty_like(x)
        K_.eam_hmc_run(x, u, nacc, vd, r, beta=BETA, v_last=vl, **kw)
        return x, u, nacc, vl

    full = run(x, u0, vd, r)
    for a, b in zip(full, run(x[idx], u0[idx], vd[:, idx].contiguous(), r[:, idx].contiguous())):
        assert torch.isfinite(a.float()).all() and torch.equal(a[idx], b)
    assert 0 < int(full[2].sum()) < 2 * B


# ------------------------------------------------------------ 5. HMC in one launch
def chains16():
    tab = et.fs(rho_max=400.0)
    L = tab["rc"] / 0.61
    return (systems.EAM(tab, L, device=DEV),
            torch.as_tensor(lattice(16, CHAINS, L, 1016), dtype=torch.float32, device=DEV))


def chains65():
    tab = et.fs(rho_max=400.0)
    L = tab["rc"] / 0.61
    return (systems.EAM(tab, L, device=DEV),
            torch.as_tensor(lattice(65, CHAINS, L, 1065), dtype=torch.float32, device=DEV))


@pytest.mark.parametrize("scheme", ["reference", "verlet"])
@pytest.mark.parametrize("which,epochs", [("n16", EPOCHS), ("n65", 3)])
def test_one_launch_equals_per_epoch_kernels_bitwise(which, epochs, scheme, hip_device):
    """On the CPU path the n = 16 settings accept 202 of 222 moves under both schemes;
    the GPU's random stream differs, but a 9 % rejection rate does not vanish."""
    sim, x0 = chains16() if which == "n16" else chains65()
    run = HMC(sim, path_len=PATH, dt=HMC_DT, dim=3, beta=BETA, scheme=scheme)
    W = x0[0].numel()
    got = {}
    torch.manual_seed(41)
    n = counts_of(lambda: got.update(one_launch(sim, run, x0, epochs)))
    assert got["vel"].shape == x0.shape and sim.get_position().shape == x0.shape
    torch.manual_seed(41)
    v, r = draws(run, epochs, CHAINS, W)
    want = per_epoch_loop(sim, run, x0, v, r)
    total = int(want["nacc"].sum())
    print("%s %s: %d of %d moves accepted" % (which, scheme, total, epochs * CHAINS))
    assert_same(got, want, (which, scheme))
    assert got["pos"].shape == (epochs, CHAINS, W) and torch.equal(got["pos"][0], x0.reshape(CHAINS, W))
    assert torch.isfinite(got["pos"]).all() and torch.isfinite(got["pot"]).all()
    assert 0 < total < epochs * CHAINS, "both branches of the decision must run"
    assert n.get("nfk_eam_hmc_run") == 1 and run_launches(n) == 1, n
    assert not any(k.endswith("_trajectory") or k == "nfk_hmc_accept" for k in n), n


# ------------------------------------------------------------------------ 6. segments
def test_one_epoch_per_segment_equals_the_default_hmc(hip_device):
    sim, x0 = chains16()
    run = HMC(sim, path_len=PATH, dt=HMC_DT, dim=3, beta=BETA)
    W = x0[0].numel()
    one = 4 * CHAINS * (W + 1)
    torch.manual_seed(43)
    pos, pot, lp, rate = run.hmc(EPOCHS, x0)
    want = dict(pos=pos, pot=pot, x=run.position.clone(), u=run.potential.clone(), nacc=run.naccept.clone(),
                vel=sim.get_velocity().clone(), lp=lp)
    got = {}
    torch.manual_seed(43)
    n = counts_of(lambda: got.update(one_launch(sim, run, x0, EPOCHS, draw_bytes=one)))
    assert_same(got, want, "one epoch per segment")
    assert got["rate"] == rate and run_launches(n) == EPOCHS and n.get("nfk_eam_hmc_run") == EPOCHS, n
    # 3 epochs as 2 + 1: two launches, the second continuing from the first one's state
    torch.manual_seed(44)
    n = counts_of(lambda: got.update(one_launch(sim, run, x0, 3, draw_bytes=2 * one)))
    torch.manual_seed(44)
    v, r = draws(run, 3, CHAINS, W, draw_bytes=2 * one)
    assert v.shape[0] == 3
    assert_same(got, per_epoch_loop(sim, run, x0, v, r), "2 + 1")
    assert run_launches(n) == 2, n


# ------------------------------------------------------------------- 7. hamiltonian
def test_hamiltonian_decisions_against_fp64(hip_device):
    """The n = 16 chains under the correct sampler at dt 0.3.  The margin formula of
    restated_decisions gives about 0.15 expected unjudged chains at these values; the
    cap is 5 % of the chains, one chain: a condition, not a measurement.  On the CPU
    these settings accept 202-205 of 222 moves."""
    sim, x0 = chains16()
    D, lanes = 48, 16
    run = HMC(sim, path_len=PATH, dt=0.3, dim=3, beta=BETA, scheme="verlet", hamiltonian=True)
    got = {}
    torch.manual_seed(47)
    n = counts_of(lambda: got.update(one_launch(sim, run, x0, EPOCHS)))
    assert run_launches(n) == 1 and "nfk_hmc_accept" not in n, n
    torch.manual_seed(47)
    v, r = draws(run, EPOCHS, CHAINS, D)
    assert torch.equal(got["lp"], run.log_prob(v[-1]))
    acc, judged, x_new, u_new = restated_decisions(sim, run, x0, got["pos"], got["pot"], v, r, D, lanes)
    nxt_x = torch.cat([got["pos"][1:], got["x"].reshape(1, CHAINS, D)])
    nxt_u = torch.cat([got["pot"][1:], got["u"].reshape(1, CHAINS)])
    took = (nxt_x == x_new).all(-1)
    stay = (nxt_x == got["pos"]).all(-1)
    assert not (took & stay).any(), "a proposal equal to its start: the walk cannot tell"
    # every chain, judged or not, moved row, potential and count together
    assert (took | stay).all()
    assert torch.equal(nxt_u[took], u_new[took]) and torch.equal(nxt_u[stay], got["pot"][stay])
    assert torch.equal(got["nacc"], took.sum(0).to(torch.int32))
    chain_judged = judged.all(0)
    unjudged = int((~chain_judged).sum())
    print("%d of %d moves accepted, %d chains unjudged" % (int(took.sum()), took.numel(), unjudged))
    assert unjudged <= 0.05 * CHAINS
    assert torch.equal(took[:, chain_judged], acc[:, chain_judged])
    assert 0 < int(took.sum()) < took.numel(), "both branches of the decision must run"
    sim.integration_step(PATH, 0.3, got["pos"][-1].view(x0.shape).clone(), v[-1].view(x0.shape), scheme="verlet")
    assert torch.equal(got["vel"], sim.get_velocity())


# ------------------------------------------------------------- 8. a poisoned chain
def test_a_poisoned_chain_stays_alone(hip_device):
    sim, x0 = chains16()
    run = HMC(sim, path_len=PATH, dt=HMC_DT, dim=3, beta=BETA)
    sim.set_position(x0)
    torch.manual_seed(61)
    v, r = draws(run, EPOCHS, CHAINS, 48)
    u0 = sim.potential(x0)
    bad = v.clone()
    bad[:, 11, 5] = float("nan")

    def launch(vd):
        x, u = x0.reshape(CHAINS, 48).clone(), u0.clone()
        nacc = torch.zeros(CHAINS, dtype=torch.int32, device=DEV)
        K_.eam_hmc_run(x, u, nacc, vd, r, path_len=PATH, dt=HMC_DT, scheme=0, beta=BETA, n=16,
                       **sim._kw(x.device))
        return x, u, nacc

    clean, dirty = launch(v), launch(bad)
    assert int(dirty[2][11]) == 0 and torch.equal(dirty[0][11], x0[11].flatten()) and dirty[1][11] == u0[11]
    others = torch.arange(CHAINS, device=DEV) != 11
    for a, b in zip(clean, dirty):
        assert torch.equal(a[others], b[others])
    assert 0 < int(clean[2].sum()) < EPOCHS * CHAINS


# -------------------------------------------------------------- 9. routes and errors
def test_unsupported_inputs_take_the_per_step_path_or_raise(hip_device):
    tab = et.fs(rho_max=400.0)
    L = tab["rc"] / 0.61
    eam = systems.EAM(tab, L, device=DEV)
    assert K_.eam_hmc_supported(256) and not K_.eam_hmc_supported(257) and not K_.eam_hmc_supported(0)
    big = torch.as_tensor(lattice(257, 2, L, 1257), dtype=torch.float32, device=DEV)
    x64 = torch.as_tensor(lattice(16, 3, L, 1016), device=DEV)
    for x in (big, x64):
        v = 0.3 * torch.randn(x.shape, device=DEV, dtype=x.dtype, generator=torch.Generator(device=DEV).manual_seed(3))
        out = []
        for fused in (True, False):
            eam.fused_dynamics = fused
            n = counts_of(lambda: out.append(eam.integration_step(2, DT, x, v, scheme="verlet")))
            assert not any(k.endswith("_trajectory") for k in n), n
            out.append(eam.get_velocity())
        assert torch.equal(out[0][0], out[2][0]) and torch.equal(out[0][1], out[2][1]) and torch.equal(out[1], out[3])
        assert out[0][0].dtype == x.dtype
    eam.fused_dynamics = True
    # above the row cap of the fused route the per-step path runs, with the same bits
    cap = eam._FUSED_ROWS_MAX
    x3 = torch.as_tensor(lattice(3, 1, L, 1003), dtype=torch.float32, device=DEV).expand(cap + 1, 3, 3)
    x3 = x3 + 0.01 * torch.randn(x3.shape, device=DEV, generator=torch.Generator(device=DEV).manual_seed(4))
    v3 = torch.zeros_like(x3)
    out = []
    n = counts_of(lambda: out.append(eam.integration_step(1, DT, x3[:cap], v3[:cap], scheme="verlet")))
    assert n == {"nfk_eam_trajectory": 1}, n
    n = counts_of(lambda: out.append(eam.integration_step(1, DT, x3, v3, scheme="verlet")))
    assert "nfk_eam_trajectory" not in n and n.get("nfk_eam_potential_bwd") == 2, n
    assert torch.equal(out[0][0], out[1][0][:cap]) and torch.equal(out[0][1], out[1][1][:cap])
    # a run of fp64 chains takes the per-epoch steps
    run = HMC(eam, path_len=2, dt=HMC_DT, dim=3, beta=BETA)
    n = counts_of(lambda: run.hmc(2, x64, one_launch=True))
    assert run_launches(n) == 0, n

    kw = eam._kw(torch.device(DEV))
    z = lambda *s: torch.zeros(*s, device=DEV)  # noqa: E731
    t16 = (z(2, 48), z(2, 48), z(2, 48), z(2, 48), z(2))
    h16 = (z(2, 48), z(2), torch.zeros(2, dtype=torch.int32, device=DEV), z(3, 2, 48), z(3, 2))
    W = 257 * 3
    with pytest.raises(ValueError, match="shape not supported"):
        K_.eam_trajectory(z(2, W), z(2, W), z(2, W), z(2, W), z(2), path_len=1, dt=DT, scheme=0, n=257, **kw)
    with pytest.raises(ValueError, match="shape not supported"):
        K_.eam_hmc_run(z(2, W), z(2), None, z(3, 2, W), z(3, 2), path_len=1, dt=DT, scheme=0, beta=1.0, n=257, **kw)
    with pytest.raises(ValueError, match="bad tables, box or cutoff"):
        K_.eam_trajectory(*t16, path_len=1, dt=DT, scheme=0, n=16, **dict(kw, rc=-1.0))
    with pytest.raises(ValueError, match="bad tables, box or cutoff"):
        K_.eam_hmc_run(*h16, path_len=1, dt=DT, scheme=0, beta=1.0, n=16, **dict(kw, rc=-1.0))
    with pytest.raises(ValueError, match="path_len below zero"):
        K_.eam_trajectory(*t16, path_len=-1, dt=DT, scheme=0, n=16, **kw)
    with pytest.raises(ValueError, match="path_len below zero"):
        K_.eam_hmc_run(*h16, path_len=-1, dt=DT, scheme=0, beta=1.0, n=16, **kw)
    with pytest.raises(ValueError, match="scheme must be 0"):
        K_.eam_trajectory(*t16, path_len=1, dt=DT, scheme=2, n=16, **kw)
    with pytest.raises(ValueError, match="scheme must be 0"):
        K_.eam_hmc_run(*h16, path_len=1, dt=DT, scheme=2, beta=1.0, n=16, **kw)
    # batch 0 and epochs 0: nothing to do and nothing written
    K_.eam_trajectory(z(0, 48), z(0, 48), z(0, 48), z(0, 48), z(0), path_len=1, dt=DT, scheme=0, n=16, **kw)
    x, u = torch.full((2, 48), 7.0, device=DEV), torch.full((2,), 5.0, device=DEV)
    K_.eam_hmc_run(x, u, h16[2], z(0, 2, 48), z(0, 2), path_len=1, dt=DT, scheme=0, beta=1.0, n=16, **kw)
    torch.cuda.synchronize()
    assert bool((x == 7.0).all()) and bool((u == 5.0).all()) and int(h16[2].sum()) == 0
    n = counts_of(lambda: run.hmc(0, x64.float(), one_launch=True))
    assert run_launches(n) == 0, n


# -------------------------------------------------------------------- 10. application
def test_relaxation_step_and_collect_hmc_data(tmp_path, hip_device):
    cfg, _, frames = et.fe_config(tmp_path, device=DEV)
    torch.manual_seed(7)
    model = app.build_model(cfg)
    pot = app.build_potential(cfg, mode="testing")
    assert isinstance(pot, systems.EAM) and pot.fused_dynamics
    traj = torch.as_tensor(frames, device=DEV).reshape(len(frames), -1)
    out = []
    torch.manual_seed(8)
    n = counts_of(lambda: out.extend(app.relaxation_step(cfg, model, pot, traj, path_len=2)))
    assert n.get("nfk_eam_trajectory") == 2 and "nfk_eam_potential_bwd" not in n, n
    pot.fused_dynamics = False
    torch.manual_seed(8)
    n = counts_of(lambda: out.extend(app.relaxation_step(cfg, model, pot, traj, path_len=2)))
    assert "nfk_eam_trajectory" not in n and n.get("nfk_eam_potential_bwd", 0) > 0, n
    pot.fused_dynamics = True
    for a, b in zip(out[:3], out[3:]):
        assert a.shape == b.shape and torch.isfinite(a).all() and torch.equal(a, b)

    run = HMC(pot, path_len=2, dt=0.01, dim=3, beta=1 / cfg.dataset.kT)
    got = []
    torch.manual_seed(21)
    n = counts_of(lambda: got.extend(app.collect_hmc_data(cfg, model, run, burnin=2, epochs=8, one_launch=True)))
    hmc_traj, acc = got
    assert hmc_traj.shape == (6, 48) and hmc_traj.is_cuda and isinstance(acc, float)
    assert n.get("nfk_eam_hmc_run") == 1 and run_launches(n) == 1, n
    torch.manual_seed(21)
    init = model.sample(1)[0].detach().reshape(16, 3)
    ref, _, _, acc_ref = run.hmc(8, init, one_launch=True)
    assert torch.equal(hmc_traj, ref[2:]) and acc == acc_ref


# ---------------------------------------------------------------- 11. reproducibility
def test_two_runs_are_bitwise_equal(hip_device):
    tab, box, pos = case("n54_fe")
    eam = systems.EAM(tab, box, device=DEV)
    gen = torch.Generator(device=DEV).manual_seed(2)
    x = torch.as_tensor(np.tile(pos, (40, 1, 1)), dtype=torch.float32, device=DEV)
    x = x + 0.01 * torch.randn(x.shape, device=DEV, generator=gen)
    v = 0.3 * torch.randn(x.shape, device=DEV, generator=gen)
    assert x.shape[0] == 200
    for scheme in ("reference", "verlet"):
        runs = []
        for _ in range(2):
            xo, pot = eam.integration_step(12, DT, x, v, scheme=scheme)
            runs.append((xo, eam.get_velocity(), pot))
        for a, b in zip(*runs):
            assert torch.equal(a, b)
        run = HMC(eam, path_len=PATH, dt=HMC_DT, dim=3, beta=BETA, scheme=scheme)
        outs = []
        for _ in range(2):
            torch.manual_seed(41)
            outs.append(one_launch(eam, run, x, 3))
        for key in ("pos", "pot", "x", "u", "nacc", "vel", "lp"):
            assert torch.equal(outs[0][key], outs[1][key]), key
