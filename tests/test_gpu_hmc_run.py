"""GPU checks of whole HMC runs in one launch (nfk_hmc_run.hip,
``HMC.hmc(one_launch=True)``): bit for bit against the per-epoch kernels fed
the same draws (rebuilt here from the docstring's recipe), one epoch per
segment against the default ``hmc()``, the hamiltonian decision against an fp64
restatement, the sampler's stationarity, and the edges.

Shapes are those of test_gpu_dynamics.py's BITWISE table (every mapping of the
three kernels) at 37 chains, 6 epochs and path_len 5.
"""
import math

import pytest
import torch

from nf.hmc import HMC
from normalizingflow_amd import app, systems
from normalizingflow_amd import kernels as K_
from test_dynamics_cpu import L32
from test_gpu_dynamics import BITWISE, _einstein_4x3, _einstein_case, fused_only
from test_gpu_systems import counts_of

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
RTOL, ATOL = 1e-5, 1e-4
CHAINS, EPOCHS, PATH = 37, 6, 5

# case -> (HMC's dim, beta, dt): beta and dt put the potential-only test between
# "all accepted" and "none accepted" for both schemes (asserted below)
PARAMS = {
    "lj_n3_d2": (2, 1.0, 0.01),
    "lj_n32_d3": (3, 1.0, 0.002),
    "lj_n33_ragged": (3, 1.0, 0.002),
    "lj_n100_two_per_lane": (3, 1.0, 0.002),
    "lj_n32_noshift": (3, 1.0, 0.002),
    "lj_n32_nocut": (3, 1.0, 0.002),
    "einstein_5x2_nobox": (2, 1.0, 0.005),
    "einstein_32x3_box": (3, 1.0, 0.005),
    "gmix_m1": (2, 1.0, 0.02),
    "gmix_m3_d3": (3, 1.0, 0.02),
}


def make(case, **kw):
    """(sim, run, x0 on the device in the simulation's shape) of a BITWISE case."""
    sim, x, _, _ = BITWISE[case]()
    dim, beta, dt = PARAMS[case]
    kw.setdefault("path_len", PATH)
    return sim, HMC(sim, dt=dt, dim=dim, beta=beta, **kw), x.to(DEV)


def segments(epochs, chains, width, draw_bytes):
    out, done = [], 0
    while done < epochs:
        out.append(max(1, min(epochs - done, draw_bytes // (4 * chains * (width + 1)))))
        done += out[-1]
    return out


def draws(run, epochs, chains, width, draw_bytes=1 << 28):
    """The docstring's recipe: per segment v = randn(e, C, W) * sd, then r = rand(e, C)."""
    sd = run._var(torch.device(DEV), torch.float32).sqrt()
    vs, rs = [], []
    for e in segments(epochs, chains, width, draw_bytes):
        vs.append(torch.randn(e, chains, width, device=DEV, dtype=torch.float32) * sd)
        rs.append(torch.rand(e, chains, device=DEV, dtype=torch.float32))
    return torch.cat(vs), torch.cat(rs)


def per_epoch_loop(sim, run, x0, v, r):
    """The per-epoch kernels fed the draws: integration_step + nfk_hmc_accept."""
    shape = x0.shape
    chains = v.shape[1]
    x_cur = x0.reshape(chains, -1).clone()
    u_cur = sim.potential(x0).reshape(chains).clone()
    nacc = torch.zeros(chains, dtype=torch.int32, device=x0.device)
    pos, pot = [], []
    for i in range(v.shape[0]):
        pos.append(x_cur.clone())
        pot.append(u_cur.clone())
        x_new, u_new = sim.integration_step(run.path_len, run.dt, x_cur.view(shape).clone(), v[i].view(shape),
                                            scheme=run.scheme)
        K_.hmc_accept(x_cur, x_new.reshape(chains, -1), u_cur, u_new.reshape(chains).contiguous(), r[i], nacc,
                      beta=run.beta)
    return dict(pos=torch.stack(pos), pot=torch.stack(pot), x=x_cur, u=u_cur, nacc=nacc,
                vel=sim.get_velocity().clone(), lp=run.log_prob(v[-1]))


def one_launch(sim, run, x0, epochs, **kw):
    pos, pot, lp, rate = run.hmc(epochs, x0, one_launch=True, **kw)
    vel = sim.get_velocity()
    return dict(pos=pos, pot=pot, x=run.position.clone(), u=run.potential.clone(), nacc=run.naccept.clone(),
                vel=None if vel is None else vel.clone(), lp=lp, rate=rate)


def assert_same(got, want, what):
    for key in ("pos", "pot", "x", "u", "nacc", "lp"):
        assert got[key].shape == want[key].shape and torch.equal(got[key], want[key]), (what, key)
    assert torch.equal(got["vel"].reshape(want["x"].shape), want["vel"].reshape(want["x"].shape)), (what, "vel")
    if "rate" in got:
        assert got["rate"] == float(want["nacc"].double().mean()) / max(1, want["pos"].shape[0]), what


def run_launches(n):
    return sum(c for k, c in n.items() if k.endswith("_hmc_run"))


# ------------------------------------------- 1. bitwise against the per-epoch kernels
@pytest.mark.parametrize("scheme", ["reference", "verlet"])
@pytest.mark.parametrize("case", sorted(BITWISE))
def test_one_launch_equals_per_epoch_kernels_bitwise(case, scheme, hip_device):
    sim, run, x0 = make(case, scheme=scheme)
    W = x0[0].numel()
    got = {}
    torch.manual_seed(41)
    n = counts_of(lambda: got.update(one_launch(sim, run, x0, EPOCHS)))
    assert got["vel"].shape == x0.shape and sim.get_position().shape == x0.shape
    torch.manual_seed(41)
    v, r = draws(run, EPOCHS, CHAINS, W)
    want = per_epoch_loop(sim, run, x0, v, r)
    total = int(want["nacc"].sum())
    print("%s %s: %d of %d moves accepted" % (case, scheme, total, EPOCHS * CHAINS))
    assert_same(got, want, (case, scheme))
    assert got["pos"].shape == (EPOCHS, CHAINS, W) and torch.equal(got["pos"][0], x0.reshape(CHAINS, W))
    assert torch.isfinite(got["pos"]).all() and torch.isfinite(got["pot"]).all()
    assert 0 < total < EPOCHS * CHAINS, "both branches of the decision must run"
    assert run_launches(n) == 1, n
    assert not any(k.endswith("_trajectory") or k == "nfk_hmc_accept" for k in n), n


# ------------------------------------------------- 2. segments and the default hmc()
@pytest.mark.parametrize("case", ["lj_n33_ragged", "einstein_32x3_box", "gmix_m3_d3"])
def test_one_epoch_per_segment_equals_the_default_hmc(case, hip_device):
    sim, run, x0 = make(case)
    W = x0[0].numel()
    one = 4 * CHAINS * (W + 1)
    torch.manual_seed(43)
    pos, pot, lp, rate = run.hmc(EPOCHS, x0)
    want = dict(pos=pos, pot=pot, x=run.position.clone(), u=run.potential.clone(), nacc=run.naccept.clone(),
                vel=sim.get_velocity().clone(), lp=lp)
    got = {}
    torch.manual_seed(43)
    n = counts_of(lambda: got.update(one_launch(sim, run, x0, EPOCHS, draw_bytes=one)))
    assert_same(got, want, case)
    assert got["rate"] == rate and run_launches(n) == EPOCHS, n
    # 3 epochs as 2 + 1: two launches, each continuing from the last one's state
    assert segments(3, CHAINS, W, 2 * one) == [2, 1]
    torch.manual_seed(44)
    n = counts_of(lambda: got.update(one_launch(sim, run, x0, 3, draw_bytes=2 * one)))
    torch.manual_seed(44)
    v, r = draws(run, 3, CHAINS, W, draw_bytes=2 * one)
    assert_same(got, per_epoch_loop(sim, run, x0, v, r), case)
    assert run_launches(n) == 2, n


# ------------------------------------------------------------------- 3. hamiltonian
def _ham_einstein_4x3():
    sim = _einstein_4x3()
    torch.manual_seed(1)
    return sim, sim.sample(CHAINS), 3, 1.0, 0.04, 12, 16


def _ham_einstein_32x3():
    sim, x, _, _ = _einstein_case(32, 3, True)
    return sim, x.to(DEV), 3, 1.0, 0.03, 96, 64


def _ham_lj32():
    sim, x, _, _ = BITWISE["lj_n32_d3"]()
    return sim, x.to(DEV), 3, 1.0, 0.012, 96, 32


def _ham_gmix3():
    sim, x, _, _ = BITWISE["gmix_m3_d3"]()
    return sim, x.to(DEV), 3, 1.0, 0.2, 21, 8


# -> (sim, x0, dim, beta, dt, D = row width, lanes of a chain)
HAMILTONIAN = {"einstein_4x3": _ham_einstein_4x3, "einstein_32x3_box": _ham_einstein_32x3,
               "lj_n32_d3": _ham_lj32, "gmix_m3_d3": _ham_gmix3}


def restated_decisions(sim, run, x0, pos, pot, v, r, D, lanes):
    """Per epoch, from the kernel path's own state before the move: the proposal
    (the trajectory kernel: the bits of the run's), the fp64 exponent and the
    margin inside which fp32 may decide either way.  Returns (accept [E, C],
    judged [E, C], x_new [E, C, W], u_new [E, C])."""
    shape = x0.shape
    acc, judged, xs, us = [], [], [], []
    for e in range(v.shape[0]):
        x_new, u_new = sim.integration_step(run.path_len, run.dt, pos[e].view(shape).clone(), v[e].view(shape),
                                            scheme=run.scheme)
        v_new = sim.get_velocity().reshape(v[e].shape)
        k_cur = 0.5 * (v[e].double() ** 2).sum(1)
        k_new = 0.5 * (v_new.double() ** 2).sum(1)
        u_cur, u_new = pot[e].double(), u_new.reshape(-1).double()
        p = torch.exp(((u_cur - u_new) + k_cur - k_new) * run.beta)
        m = (p * run.beta * 2.0 ** -24 * (2 * (u_cur.abs() + u_new.abs())
                                          + (math.ceil(D / lanes) + math.log2(lanes) + 2) * (k_cur + k_new))
             + 2.0 ** -22 * p)
        acc.append(r[e].double() < p)
        judged.append((r[e].double() - p).abs() > m)
        xs.append(x_new.reshape(v[e].shape))
        us.append(u_new.float())
    return torch.stack(acc), torch.stack(judged), torch.stack(xs), torch.stack(us)


@pytest.mark.parametrize("case", sorted(HAMILTONIAN))
def test_hamiltonian_decisions_against_fp64(case, hip_device):
    sim, x0, dim, beta, dt, D, lanes = HAMILTONIAN[case]()
    run = HMC(sim, path_len=PATH, dt=dt, dim=dim, beta=beta, scheme="verlet", hamiltonian=True)
    got = {}
    torch.manual_seed(47)
    n = counts_of(lambda: got.update(one_launch(sim, run, x0, EPOCHS)))
    assert run_launches(n) == 1 and "nfk_hmc_accept" not in n, n
    torch.manual_seed(47)
    v, r = draws(run, EPOCHS, CHAINS, D)
    assert torch.equal(got["lp"], run.log_prob(v[-1]))
    acc, judged, x_new, u_new = restated_decisions(sim, run, x0, got["pos"], got["pot"], v, r, D, lanes)
    # the state after move e: the next record, or the final state
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
    print("%s: %d of %d moves accepted, %d chains unjudged" % (case, int(took.sum()), took.numel(), unjudged))
    assert unjudged <= 0.05 * CHAINS
    assert torch.equal(took[:, chain_judged], acc[:, chain_judged])
    assert 0 < int(took.sum()) < took.numel(), "both branches of the decision must run"
    # the last trajectory's final velocity, accepted or not
    sim.integration_step(PATH, dt, got["pos"][-1].view(x0.shape).clone(), v[-1].view(x0.shape), scheme="verlet")
    assert torch.equal(got["vel"], sim.get_velocity())


# ------------------------------------------------------------------------ 4. sampler
def test_sampler_is_stationary_on_the_einstein_crystal_in_one_launch(hip_device, monkeypatch):
    sim = _einstein_4x3()
    fused_only(sim, monkeypatch)
    run = HMC(sim, scheme="verlet", hamiltonian=True, dt=0.02, path_len=8)
    torch.manual_seed(1)
    x0 = sim.sample(4096)
    out = []
    n = counts_of(lambda: out.extend(run.hmc(20, x0, record=False, one_launch=True)))
    pos, pot, _, acc = out
    assert run_launches(n) == 1, n
    dev = pos - sim.centers.flatten()
    var = float(600 * dev.double().var())
    move = float(((pos - x0).double() ** 2).mean().sqrt() * math.sqrt(600))
    print("acceptance %.3f, alpha * variance %.4f, rms move * sqrt(alpha) %.3f" % (acc, var, move))
    assert acc > 0.85
    assert 0.97 <= var <= 1.03
    assert move > 0.5
    torch.testing.assert_close(pot, sim.potential(pos), rtol=RTOL, atol=ATOL)


# -------------------------------------------------------------------------- 5. edges
def test_zero_epochs_and_zero_path_len(hip_device):
    sim, run, x0 = make("gmix_m3_d3")
    W = x0[0].numel()
    got = {}
    n = counts_of(lambda: got.update(one_launch(sim, run, x0, 0)))
    assert got["pos"].shape == (0, CHAINS, W) and got["pot"].shape == (0, CHAINS) and got["lp"] is None
    assert got["rate"] == 0.0 and torch.equal(got["x"], x0) and int(got["nacc"].sum()) == 0
    assert torch.equal(got["u"], sim.potential(x0)) and run_launches(n) == 0, n
    # path_len 0: the proposal is the start, its potential the trajectory kernel's closing sum
    for case in ("gmix_m3_d3", "lj_n33_ragged", "einstein_32x3_box"):
        sim, run, x0 = make(case, path_len=0)
        torch.manual_seed(51)
        n = counts_of(lambda: got.update(one_launch(sim, run, x0, 3)))
        torch.manual_seed(51)
        v, r = draws(run, 3, CHAINS, x0[0].numel())
        want = per_epoch_loop(sim, run, x0, v, r)
        assert_same(got, want, case)
        assert torch.equal(got["x"], x0.reshape(CHAINS, -1)) and run_launches(n) == 1, n
        assert torch.equal(got["vel"].reshape(CHAINS, -1), v[-1])


@pytest.mark.parametrize("case", ["lj_n32_d3", "einstein_5x2_nobox", "gmix_m1"])
def test_one_chain_and_no_record(case, hip_device):
    sim, run, x0 = make(case)
    W = x0[0].numel()
    torch.manual_seed(53)
    full = one_launch(sim, run, x0, EPOCHS)
    torch.manual_seed(53)
    fin, ufin, lp, rate = run.hmc(EPOCHS, x0, record=False, one_launch=True)
    assert torch.equal(fin, full["x"]) and torch.equal(ufin, full["u"]) and torch.equal(lp, full["lp"])
    assert rate == full["rate"] and torch.equal(run.naccept, full["nacc"])
    # one chain: the reference's shapes
    torch.manual_seed(54)
    n = counts_of(lambda: full.update(one=run.hmc(EPOCHS, x0[5], one_launch=True)))
    pos, pot, lp, _ = full["one"]
    assert pos.shape == (EPOCHS, W) and pot.shape == (EPOCHS,) and lp.shape == (1,)
    assert run.position.shape == (W,) and sim.get_position().shape == x0[5].shape and run_launches(n) == 1
    torch.manual_seed(54)
    v, r = draws(run, EPOCHS, 1, W)
    want = per_epoch_loop(sim, run, x0[5:6], v, r)
    assert torch.equal(pos, want["pos"][:, 0]) and torch.equal(pot, want["pot"][:, 0])
    assert torch.equal(run.position, want["x"][0]) and torch.equal(run.naccept, want["nacc"])


def test_rows_with_a_leading_dimension_above_the_width(hip_device):
    sim, x, _, _ = _einstein_case(32, 3, True)
    run = HMC(sim, path_len=PATH, dt=0.005)
    x = x.to(DEV)
    C, W = x.shape
    scale, hld = sim._consts()
    torch.manual_seed(57)
    v, r = draws(run, EPOCHS, C, W)
    u0 = sim.potential(x)

    def launch(x_cur, v_last):
        u, nacc = u0.clone(), torch.zeros(C, dtype=torch.int32, device=DEV)
        pos, pot = torch.empty(EPOCHS, C, W, device=DEV), torch.empty(EPOCHS, C, device=DEV)
        K_.einstein_hmc_run(x_cur, u, nacc, v, r, sim.centers, path_len=PATH, dt=0.005, scheme=1, beta=1.0,
                            scale=scale, hld=hld, boxlength=sim.boxlength, v_last=v_last, pos_rec=pos,
                            pot_rec=pot)
        return u, nacc, pos, pot

    xa, va = x.clone(), torch.empty_like(x)
    dense = launch(xa, va)
    wide_x = torch.full((C, W + 3), float("nan"), device=DEV)
    wide_v = torch.full((C, W + 5), float("nan"), device=DEV)
    wide_x[:, :W] = x
    xb, vb = wide_x[:, :W], wide_v[:, :W]
    assert xb.stride(0) == W + 3 and vb.stride(0) == W + 5
    for a, b in zip(dense, launch(xb, vb)):
        assert torch.equal(a, b)
    assert torch.equal(xa, xb) and torch.equal(va, vb) and 0 < int(dense[1].sum()) < EPOCHS * C
    assert torch.isnan(wide_x[:, W:]).all() and torch.isnan(wide_v[:, W:]).all()  # the padding is untouched
    with pytest.raises(ValueError):
        K_.einstein_hmc_run(xa, u0.clone(), None, v, r, sim.centers, path_len=PATH, dt=0.005, scheme=1,
                            beta=1.0, scale=scale, hld=hld, v_last=va[:, :-1])


def test_a_shape_beyond_the_limits_takes_the_per_epoch_steps(hip_device):
    g = torch.Generator().manual_seed(9)
    centers = (torch.rand(130, 4, generator=g) - 0.5) * L32
    sim = systems.EinsteinCrystal(centers, 4, alpha=600, device=DEV)
    assert not K_.einstein_hmc_supported(130, 4) and K_.einstein_hmc_supported(128, 4)
    x0 = (centers.flatten() + torch.randn(CHAINS, 520, generator=g) / math.sqrt(600)).to(DEV)
    run = HMC(sim, path_len=PATH, dt=0.001, dim=4)
    got = {}
    torch.manual_seed(59)
    n = counts_of(lambda: got.update(one_launch(sim, run, x0, 3)))
    torch.manual_seed(59)
    v, r = draws(run, 3, CHAINS, 520)
    assert_same(got, per_epoch_loop(sim, run, x0, v, r), "einstein 130 x 4")
    assert run_launches(n) == 0 and n.get("nfk_einstein_trajectory") == 3 and n.get("nfk_hmc_accept") == 3, n


class _Model:
    """Stand-in flow model: a seeded sampler around the mixture's first centre."""

    def __init__(self, width):
        self.width = width

    def sample(self, n):
        x = 0.1 * torch.randn(n, self.width, device=DEV) - 1.0
        return x, x.sum(1), x


def test_collect_hmc_data_in_one_launch(hip_device):
    sim = systems.GaussianMixture([[-1., -1.], [1., 1.]], [0.1, 0.05], 20, 2, device=DEV)
    run = HMC(sim, path_len=2, dt=0.01, dim=2)
    cfg = app.get_cfg_defaults()
    out = []
    torch.manual_seed(21)
    n = counts_of(lambda: out.extend(app.collect_hmc_data(cfg, _Model(40), run, burnin=3, epochs=8,
                                                          one_launch=True)))
    traj, acc = out
    assert traj.shape == (5, 40) and traj.is_cuda and isinstance(acc, float) and run_launches(n) == 1, n
    torch.manual_seed(21)
    init = _Model(40).sample(1)[0]
    ref, _, _, acc_ref = run.hmc(8, init.flatten(), one_launch=True)
    assert torch.equal(traj, ref[3:]) and acc == acc_ref
