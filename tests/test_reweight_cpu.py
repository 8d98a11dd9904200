"""CPU checks of ``normalizingflow_amd.reweight`` and ``app.metropolize``: the
torch restatement of the Metropolis chain against a scalar loop written here
from applications/src/utils.py:86-99, chains continued with ``carry``, the
NaN / inf rules, the statistics of the independence sampler against the
reference's energy-only rule, ``ess`` / ``reweighted_mean`` against closed
forms, and the host-side validation of nfk_metropolize, which never touches a
device.
"""
import math

import pytest
import torch

from normalizingflow_amd import _lib, app, systems
from normalizingflow_amd import reweight as R

PIECES = (1, 63, 64, 65, 130)


def scalar_chain(e, r, lq=None, burnin=0):
    """utils.py:86-99 on precomputed reduced energies, one 0-d tensor operation
    at a time: (accept flags, index, energy_list).  With ``lq`` the test is the
    independence sampler's."""
    n = len(e)
    index = [False for _ in range(n)]
    accept = [False for _ in range(n)]
    energy, q = e[0], None if lq is None else lq[0]
    energy_list = []
    for i in range(n):
        d = energy - e[i]
        if lq is not None:
            d = (d + q) - lq[i]
        if r[i] < torch.exp(d):
            energy = e[i]
            if lq is not None:
                q = lq[i]
            accept[i] = True
            if i > burnin:
                index[i] = True
            energy_list.append(energy)
    return accept, index, energy_list


def crystal():
    g = torch.Generator().manual_seed(3)
    centers = (torch.rand(4, 3, generator=g) - 0.5) * 2
    cfg = app.get_cfg_defaults()
    cfg.device, cfg.dataset.kT, cfg.dataset.dim, cfg.dataset.nparticles = "cpu", 0.7, 3, 4
    return systems.EinsteinCrystal(centers, 3, alpha=40), centers, cfg


def frames_of(centers, n, seed):
    """n frames around the lattice whose spread varies, so that energies rise and fall."""
    g = torch.Generator().manual_seed(seed)
    width = 0.05 + 0.1 * torch.rand(n, 1, 1, generator=g)
    return centers + width * torch.randn(n, 4, 3, generator=g)


@pytest.mark.parametrize("with_q", [False, True])
@pytest.mark.parametrize("burnin", [0, 20])
def test_metropolize_equals_the_reference_loop(burnin, with_q):
    sim, centers, cfg = crystal()
    x = frames_of(centers, 150, 11)
    lq = -0.3 * sim.potential(x) if with_q else None  # any fixed log density serves
    torch.manual_seed(5)
    kept, energies = app.metropolize(cfg, sim, x.reshape(150, 12), burnin, log_q=lq)
    torch.manual_seed(5)
    r = torch.rand(150)
    e = torch.stack([sim.potential(x[i:i + 1])[0] / cfg.dataset.kT for i in range(150)])  # frame by frame
    accept, index, energy_list = scalar_chain(e, r, lq, burnin)
    assert 10 < sum(accept) < 140, "both branches of the test must run"
    assert kept.shape == (sum(index), 4, 3) and torch.equal(kept, x[torch.tensor(index)])
    assert energies.shape == (sum(accept),) and torch.equal(energies, torch.stack(energy_list))
    state, accepted, naccept, carry = R.metropolis_chain(e, r, lq)
    assert state.dtype == torch.int32 and accepted.dtype == torch.bool and naccept.dtype == torch.int32
    assert accepted.tolist() == accept and int(naccept) == sum(accept)
    last = [max(j for j in range(i + 1) if accept[j]) for i in range(150)]  # step 0 always accepts
    assert state.tolist() == last
    assert float(carry[0]) == float(e[last[-1]]) and int(carry[2]) == last[-1]
    assert (carry[1] is None) == (lq is None)
    # return_chain: the state after every step past the burn-in, fixed shapes
    torch.manual_seed(5)
    xs, es, rate = app.metropolize(cfg, sim, x, burnin, log_q=lq, return_chain=True)
    want = torch.tensor(last[burnin + 1:])
    assert xs.shape == (149 - burnin, 4, 3) and torch.equal(xs, x[want]) and torch.equal(es, e[want])
    assert float(rate) == sum(accept) / 150


@pytest.mark.parametrize("with_q", [False, True])
def test_a_chain_in_pieces_equals_the_chain_in_one(with_q):
    g = torch.Generator().manual_seed(8)
    C, N = 3, sum(PIECES)
    e, r = 2.0 * torch.randn(C, N, generator=g), torch.rand(C, N, generator=g)
    lq = torch.randn(C, N, generator=g) if with_q else None
    state, accepted, naccept, carry = R.metropolis_chain(e, r, lq)
    assert 0 < int(naccept.min()) and int(naccept.max()) < N
    parts, o, c, total = [], 0, None, torch.zeros(C, dtype=torch.int32)
    for n in PIECES:
        given = c
        copy = None if c is None else tuple(None if t is None else t.clone() for t in c)
        s, a, k, c = R.metropolis_chain(e[:, o:o + n], r[:, o:o + n], None if lq is None else lq[:, o:o + n],
                                        carry=c, base=o)
        if given is not None:  # the caller's carry is not written to
            assert all(t is None or torch.equal(t, u) for t, u in zip(given, copy))
        parts.append((s, a))
        total += k
        o += n
    assert torch.equal(torch.cat([p[0] for p in parts], 1), state)
    assert torch.equal(torch.cat([p[1] for p in parts], 1), accepted)
    assert torch.equal(total, naccept)
    assert torch.equal(c[0], carry[0]) and torch.equal(c[2], carry[2])
    assert (c[1] is None and carry[1] is None) or torch.equal(c[1], carry[1])
    # one chain as a vector
    s1, a1, k1, c1 = R.metropolis_chain(e[1], r[1], None if lq is None else lq[1])
    assert torch.equal(s1, state[1]) and torch.equal(a1, accepted[1]) and k1.dim() == 0 and int(k1) == int(naccept[1])
    assert c1[0].dim() == 0 and float(c1[0]) == float(carry[0][1])


def test_nan_and_inf_rules():
    nan, inf = float("nan"), float("inf")
    r = torch.full((8,), 0.999)
    # a NaN and a +inf proposal reject; an equal energy accepts whatever r < 1 is
    e = torch.tensor([1.0, nan, 1.0, inf, 1.0, 5.0, 1.0, 0.5])
    state, accepted, naccept, carry = R.metropolis_chain(e, r)
    assert accepted.tolist() == [True, False, True, False, True, False, True, True]
    assert state.tolist() == [0, 0, 2, 2, 4, 4, 6, 7] and int(naccept) == 5 and float(carry[0]) == 0.5
    # after an accepted -inf nothing finite (nor another -inf, whose d is NaN) is accepted
    e = torch.tensor([1.0, -inf, -5.0, -1e30, -inf, 0.0, nan, inf])
    state, accepted, _, carry = R.metropolis_chain(e, torch.zeros(8))
    assert accepted.tolist() == [True, True] + [False] * 6 and state.tolist() == [0] + [1] * 7
    assert float(carry[0]) == -inf and int(carry[2]) == 1
    # the same through log_q: a NaN density rejects, d = (d + lq_cur) - lq[i] in that order
    e = torch.tensor([1.0, 0.0, 0.0, 3.0])
    lq = torch.tensor([0.0, nan, 0.0, -5.0])
    _, accepted, _, _ = R.metropolis_chain(e, torch.full((4,), 0.5), lq)
    assert accepted.tolist() == [True, False, True, True]
    # a chain that starts at a NaN never moves
    state, accepted, _, _ = R.metropolis_chain(torch.tensor([nan, 0.0, 1.0]), torch.zeros(3), base=7)
    assert accepted.tolist() == [False] * 3 and state.tolist() == [7] * 3


def test_argument_errors():
    e, r = torch.zeros(2, 5), torch.zeros(2, 5)
    with pytest.raises(ValueError, match="one shape"):
        R.metropolis_chain(e, r[:, :4])
    with pytest.raises(ValueError, match="fit int32"):
        R.metropolis_chain(e, r, base=2 ** 31 - 5)
    with pytest.raises(ValueError, match="fit int32"):
        R.metropolis_chain(e, r, base=-1)
    _, _, _, carry = R.metropolis_chain(e, r)
    with pytest.raises(ValueError, match="lq_cur exactly when"):
        R.metropolis_chain(e, r, torch.zeros(2, 5), carry=carry)
    with pytest.raises(ValueError, match="one state per chain"):
        R.metropolis_chain(e[:1], r[:1], carry=carry)
    with pytest.raises(ValueError, match="at least one proposal"):
        R.metropolis_chain(e[:, :0], r[:, :0])
    s, a, k, c = R.metropolis_chain(e[:, :0], r[:, :0], carry=carry)
    assert s.shape == (2, 0) and a.shape == (2, 0) and k.tolist() == [0, 0] and torch.equal(c[2], carry[2])


def test_the_correct_rule_samples_the_target_and_the_energy_rule_does_not():
    """Proposals N(0, 1.5^2), target N(0.5, 1): 64 chains of 4096 proposals, the
    first 256 states dropped.  The standard errors come from the spread between
    the chains."""
    C, N, DROP = 64, 4096, 256
    g = torch.Generator().manual_seed(0)
    x = 1.5 * torch.randn(C, N, generator=g)
    r = torch.rand(C, N, generator=g)
    e = 0.5 * (x - 0.5) ** 2
    lq = -0.5 * (x / 1.5) ** 2 - math.log(1.5)

    def moments(log_q):
        state, _, naccept, _ = R.metropolis_chain(e, r, log_q)
        xs = torch.gather(x, 1, state[:, DROP:].long()).double()
        means = xs.mean(1)
        mean, mean_se = float(means.mean()), float(means.std()) / math.sqrt(C)
        sq = ((xs - mean) ** 2).mean(1)
        return mean, mean_se, float(sq.mean()), float(sq.std()) / math.sqrt(C), float(naccept.double().mean()) / N

    mean, se, var, var_se, rate = moments(lq)
    print("independence sampler: mean %.4f se %.4f var %.4f se %.4f acceptance %.3f" % (mean, se, var, var_se, rate))
    assert 0.0 < se < 0.01 and 0.0 < var_se < 0.02
    assert abs(mean - 0.5) < 5 * se
    assert abs(var - 1.0) < 5 * var_se
    mean0, se0, var0, _, rate0 = moments(None)
    print("energy-only rule: mean %.4f se %.4f var %.4f acceptance %.3f" % (mean0, se0, var0, rate0))
    assert abs(mean0 - 0.5) > 5 * se0


def test_ess_and_reweighted_mean_closed_forms():
    N = 1000
    assert float(R.ess(torch.full((N,), -3.25))) == pytest.approx(N, rel=1e-12)
    lw = torch.zeros(N, dtype=torch.float64)
    lw[17] = 60.0  # the others weigh e^-60 of it
    assert float(R.ess(lw)) == pytest.approx(1.0, rel=1e-12)
    # m weights of a and N - m of 1: (m a + N - m)^2 / (m a^2 + N - m), shifted by a constant
    m, a = 100, 7.0
    lw = torch.cat((torch.full((m,), math.log(a), dtype=torch.float64),
                    torch.zeros(N - m, dtype=torch.float64))) + 123.0
    want = (m * a + N - m) ** 2 / (m * a * a + N - m)
    assert float(R.ess(lw)) == pytest.approx(want, rel=1e-12)
    assert R.ess(torch.stack((lw, lw * 0))).shape == (2,)
    assert float(R.ess(torch.stack((lw, lw * 0)))[1]) == pytest.approx(N, rel=1e-12)
    # fp32 weights far outside exp's range: evaluated in fp64 from the logs
    big = torch.tensor([-500.0, -500.0, -501.0])
    w = torch.tensor([1.0, 1.0, math.exp(-1.0)], dtype=torch.float64)
    assert float(R.ess(big)) == pytest.approx(float(w.sum() ** 2 / (w * w).sum()), rel=1e-12)
    v = torch.tensor([2.0, 4.0, -1.0])
    assert float(R.reweighted_mean(v, big)) == pytest.approx(float((w * v.double()).sum() / w.sum()), rel=1e-12)
    vv = torch.stack((v, 2 * v), dim=1)  # [N, W]
    got = R.reweighted_mean(vv, big)
    assert got.shape == (2,) and float(got[1]) == pytest.approx(2 * float(got[0]), rel=1e-12)
    with pytest.raises(ValueError):
        R.reweighted_mean(torch.zeros(3, 2, 2), big)
    # log_weights and a reweighting that is exact: proposals N(0, 1.5^2), target N(0.5, 1), E[x] = 0.5
    g = torch.Generator().manual_seed(1)
    x = 1.5 * torch.randn(200000, generator=g, dtype=torch.float64)
    e, lq = 0.5 * (x - 0.5) ** 2, -0.5 * (x / 1.5) ** 2 - math.log(1.5)
    logw = R.log_weights(lq, e)
    assert torch.equal(logw, -e - lq)
    assert float(R.reweighted_mean(x, logw)) == pytest.approx(0.5, abs=0.02)
    # ESS / N -> 1 / E_q[w^2] = sqrt(2 s^2 - 1) / s^2 exp(-mu^2 / (2 s^2 - 1)) for these Gaussians (0.774)
    s2 = 1.5 ** 2
    ratio = math.sqrt(2 * s2 - 1) / s2 * math.exp(-0.25 / (2 * s2 - 1))
    assert float(R.ess(logw)) / 200000 == pytest.approx(ratio, rel=0.02)


# --------------------------------------------------------------- host-only ABI checks
def _call(lib, e=1, lde=64, lq=None, ldq=64, r=1, ldr=64, chains=2, N=64, base=0, carry_in=0, e_cur=None,
          lq_cur=None, idx_cur=None, state=None, lds=64, accepted=None, lda=64, naccept=None):
    return lib.nfk_metropolize(e, lde, lq, ldq, r, ldr, chains, N, base, carry_in, e_cur, lq_cur, idx_cur, state,
                               lds, accepted, lda, naccept, None)


REFUSALS = [
    (dict(chains=-1), b"bad sizes"),
    (dict(N=-1), b"bad sizes"),
    (dict(base=-1), b"fit int32"),
    (dict(base=2 ** 31 - 64), b"fit int32"),
    (dict(e=None), b"null pointer"),
    (dict(r=None), b"null pointer"),
    (dict(e_cur=1), b"e_cur and idx_cur come together"),
    (dict(idx_cur=1), b"e_cur and idx_cur come together"),
    (dict(lq_cur=1), b"lq and lq_cur come together"),
    (dict(lq=1, lq_cur=1), b"lq and lq_cur come together"),
    (dict(lq=1, e_cur=1, idx_cur=1), b"lq and lq_cur come together"),
    (dict(e_cur=1, idx_cur=1, lq_cur=1), b"lq and lq_cur come together"),
    (dict(carry_in=1), b"carry_in needs"),
    (dict(lde=63), b"leading dimension"),
    (dict(ldr=63), b"leading dimension"),
    (dict(lq=1, ldq=63), b"leading dimension"),
    (dict(state=1, lds=63), b"leading dimension"),
    (dict(accepted=1, lda=63), b"leading dimension"),
]


def test_refusals_never_reach_the_device():
    """Every refusal is decided on the host before anything is enqueued; the
    non-null pointers are placeholders that are never read."""
    lib = _lib.load()
    for kw, msg in REFUSALS:
        assert _call(lib, **kw) == _lib.NFK_EINVAL, kw
        err = lib.nfk_last_error()
        assert msg in err and err.startswith(b"nfk_metropolize"), (kw, err)
    assert _call(lib, chains=0) == 0
    assert _call(lib, N=0) == 0
    assert _call(lib, N=0, e=None, r=None, carry_in=1) == 0
    assert _call(lib, chains=0, N=2 ** 31 - 1, lde=0) == 0
    # the size and base rules come first
    assert _call(lib, chains=0, N=2 ** 31) == _lib.NFK_EINVAL
