"""GPU checks of the nfk_metropolize kernel (nfk_metropolize.hip) and of the
layers over it (``reweight.metropolis_chain``, ``app.metropolize``,
``app.metropolized_samples``).

The kernel is compared with the CPU restatement of the same fp32 arithmetic
and must equal it exactly in ``state``, ``accepted``, ``naccept`` and the carry.
``expf`` on the device and ``torch.exp`` on the host may differ in the last
bit, so every case first asserts, on the CPU chain alone, that no decision is
near its threshold: min_i |r_i - exp(d_i)| / exp(d_i) > 1e-6, with exp taken in
fp64 of the fp32 d_i (``margin``).  That is a condition on the inputs, not a
tolerance on the result.  Steps whose d is exactly 0 (exp is exactly 1 on both
sides: step 0 of a chain without carry), NaN, or beyond exp's fp64 range (the
result is 0 or inf on both sides) are decided alike by any exp and are left
out of the minimum.
"""
import pytest
import torch

import nf.flows as nff
import nf.models as nfm
from normalizingflow_amd import app, config, systems
from normalizingflow_amd import kernels as K_
from normalizingflow_amd import reweight as R
from test_gpu_systems import counts_of

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SIZES_N = (1, 2, 63, 64, 65, 128, 130, 321)
SIZES_C = (1, 3, 4, 5, 9)  # below, at and above one workgroup's four waves
PIECES = (1, 63, 64, 65, 130)
MARGIN = 1e-6


def margin(e, r, lq, accepted, start=None):
    """min_i |r_i - exp(d_i)| / exp(d_i) of a CPU chain, d_i in fp32 in the
    kernel's order from the state before step i (see the module docstring)."""
    C, N = e.shape
    pos = torch.where(accepted, torch.arange(N).expand(C, N), torch.full((C, N), -1))
    before = torch.cat((torch.full((C, 1), -1), torch.cummax(pos, 1).values[:, :-1]), 1)
    took = before >= 0
    e0 = e[:, :1] if start is None else start[0].reshape(C, 1)
    d = torch.where(took, e.gather(1, before.clamp_min(0)), e0.expand(C, N)) - e
    if lq is not None:
        q0 = lq[:, :1] if start is None else start[1].reshape(C, 1)
        d = (d + torch.where(took, lq.gather(1, before.clamp_min(0)), q0.expand(C, N))) - lq
    assert d.dtype == torch.float32
    p = torch.exp(d.double())
    near = (d != 0) & torch.isfinite(p) & (p > 0)
    if not bool(near.any()):
        return float("inf")
    return float(((r.double() - p).abs() / p)[near].min())


def cpu_chain(e, r, lq=None, carry=None, base=0):
    """The CPU restatement on fp32 CPU tensors, with the margin condition asserted."""
    state, accepted, naccept, out = R.metropolis_chain(e, r, lq, carry=carry, base=base)
    m = margin(e, r, lq, accepted, carry)
    assert m > MARGIN, "a decision within %.3g of its threshold: choose another seed" % m
    return state, accepted, naccept, out


def dev(t):
    return None if t is None else t.to(DEV)


def run_kernel(e, r, lq=None, carry=None, base=0):
    """``metropolis_chain`` on device copies in one nfk_metropolize launch; results on the host."""
    out = {}

    def go():
        out["r"] = R.metropolis_chain(dev(e), dev(r), dev(lq), base=base,
                                      carry=None if carry is None else tuple(dev(t) for t in carry))

    n = counts_of(go)
    assert n == {"nfk_metropolize": 1}, n
    state, accepted, naccept, c = out["r"]
    assert state.is_cuda and state.dtype == torch.int32 and accepted.dtype == torch.bool
    assert naccept.dtype == torch.int32 and c[2].dtype == torch.int32
    return state.cpu(), accepted.cpu(), naccept.cpu(), tuple(None if t is None else t.cpu() for t in c)


def same(got, want):
    assert torch.equal(got[0], want[0]), "state"
    assert torch.equal(got[1], want[1]), "accepted"
    assert torch.equal(got[2], want[2]), "naccept"
    for g, w in zip(got[3], want[3]):
        assert (g is None and w is None) or torch.equal(g, w), "carry"


def draws(C, N, seed, with_q):
    g = torch.Generator().manual_seed(seed)
    e, r = 1.5 * torch.randn(C, N, generator=g), torch.rand(C, N, generator=g)
    return e, r, (torch.randn(C, N, generator=g) if with_q else None)


@pytest.mark.parametrize("with_q", [False, True], ids=["energy", "lq"])
@pytest.mark.parametrize("N", SIZES_N)
def test_every_shape_equals_the_cpu_chain(N, with_q, hip_device):
    """One CPU reference of 9 chains per N; chains are independent, so its
    first C rows are the reference of every smaller C."""
    e, r, lq = draws(max(SIZES_C), N, 100 + N, with_q)
    want = cpu_chain(e, r, lq)
    if N > 2:
        assert 0 < int(want[2].min()) and int(want[2].max()) < N
    for C in SIZES_C:
        got = run_kernel(e[:C], r[:C], None if lq is None else lq[:C])
        same(got, (want[0][:C], want[1][:C], want[2][:C], tuple(None if t is None else t[:C] for t in want[3])))


@pytest.mark.parametrize("with_q", [False, True], ids=["energy", "lq"])
@pytest.mark.parametrize("N", [128, 130], ids=["aligned", "ragged"])
def test_acceptance_regimes(N, with_q, hip_device):
    C = 5
    g = torch.Generator().manual_seed(N)
    r = torch.rand(C, N, generator=g)
    steps = torch.arange(N, dtype=torch.float32).expand(C, N)
    # every step accepts: strictly decreasing e (with lq = e / 4 the exponent is 1.25 times the drop)
    e = -0.5 * steps - torch.rand(C, N, generator=g).cumsum(1)
    want = cpu_chain(e, r, 0.25 * e if with_q else None)
    assert bool(want[1].all()) and want[0].tolist() == [list(range(N))] * C
    same(run_kernel(e, r, 0.25 * e if with_q else None), want)
    # nothing accepts after step 0: e[0] lowest by a wide gap
    e = torch.randn(C, N, generator=g)
    e[:, 0] = -50.0
    lq = 0.5 * torch.randn(C, N, generator=g) if with_q else None
    want = cpu_chain(e, r, lq)
    assert want[2].tolist() == [1] * C and not bool(want[0].any())
    same(run_kernel(e, r, lq), want)
    # random, at a low and a high acceptance rate
    for spread in (4.0, 0.3):
        e = spread * torch.randn(C, N, generator=g)
        lq = 0.5 * torch.randn(C, N, generator=g) if with_q else None
        want = cpu_chain(e, r, lq)
        assert 1 < int(want[2].min()) and int(want[2].max()) < N
        same(run_kernel(e, r, lq), want)


def test_acceptance_at_block_boundaries(hip_device):
    """Exactly lane 0 and lane 63 of every 64-block accept."""
    C, N = 2, 192
    accept_at = [0, 63, 64, 127, 128, 191]
    g = torch.Generator().manual_seed(64)
    r = torch.rand(C, N, generator=g)
    e = torch.full((C, N), 100.0)
    for k, i in enumerate(accept_at):
        e[:, i] = -float(k)
    for lq in (None, 0.5 * e):
        want = cpu_chain(e, r, lq)
        assert [i for i in range(N) if want[1][0, i]] == accept_at and want[2].tolist() == [6, 6]
        same(run_kernel(e, r, lq), want)


def test_row_strides_and_untouched_padding(hip_device):
    C, N, LEFT, WIDE = 5, 130, 3, 141
    e, r, lq = draws(C, N, 7, True)
    want = cpu_chain(e, r, lq)

    def wide(t, fill, dtype):
        w = torch.full((C, WIDE), fill, dtype=dtype, device=DEV)
        if t is not None:
            w[:, LEFT:LEFT + N] = t.to(DEV)
        return w

    we, wr, wq = (wide(t, float("nan"), torch.float32) for t in (e, r, lq))
    ws, wa = wide(None, -7, torch.int32), wide(None, 9, torch.uint8)
    naccept = torch.zeros(C, dtype=torch.int32, device=DEV)
    cut = slice(LEFT, LEFT + N)
    K_.metropolize(we[:, cut], wr[:, cut], lq=wq[:, cut], state=ws[:, cut], accepted=wa[:, cut], naccept=naccept)
    assert torch.equal(ws[:, cut].cpu(), want[0]) and torch.equal(wa[:, cut].cpu().bool(), want[1])
    assert torch.equal(naccept.cpu(), want[2])
    pad = torch.ones(WIDE, dtype=torch.bool)
    pad[cut] = False
    assert bool((ws.cpu()[:, pad] == -7).all()) and bool((wa.cpu()[:, pad] == 9).all())
    # through metropolis_chain, which passes the strides on
    got = R.metropolis_chain(we[:, cut], wr[:, cut], wq[:, cut])
    same((got[0].cpu(), got[1].cpu(), got[2].cpu(), tuple(t.cpu() for t in got[3])), want)
    with pytest.raises(ValueError, match="unit column stride"):
        K_.metropolize(we[:, 0:120:2], wr[:, 0:60])


@pytest.mark.parametrize("with_q", [False, True], ids=["energy", "lq"])
def test_a_chain_in_pieces_with_carry_and_base(with_q, hip_device):
    C, N, BASE = 5, sum(PIECES), 1000
    e, r, lq = draws(C, N, 21, with_q)
    want = cpu_chain(e, r, lq, base=BASE)
    assert int(want[0].min()) >= BASE
    # the kernel entry: one set of carry arrays and one naccept through every call
    de, dr, dq = dev(e), dev(r), dev(lq)
    state = torch.empty(C, N, dtype=torch.int32, device=DEV)
    accepted = torch.empty(C, N, dtype=torch.uint8, device=DEV)
    naccept = torch.zeros(C, dtype=torch.int32, device=DEV)
    e_cur = torch.empty(C, device=DEV)
    q_cur = torch.empty(C, device=DEV) if with_q else None
    i_cur = torch.empty(C, dtype=torch.int32, device=DEV)
    o = 0
    for n in PIECES:
        cut = slice(o, o + n)
        K_.metropolize(de[:, cut], dr[:, cut], lq=dq[:, cut] if with_q else None, state=state[:, cut],
                       accepted=accepted[:, cut], naccept=naccept, e_cur=e_cur, lq_cur=q_cur, idx_cur=i_cur,
                       carry_in=o > 0, base=BASE + o)
        o += n
    same((state.cpu(), accepted.cpu().bool(), naccept.cpu(),
          (e_cur.cpu(), None if q_cur is None else q_cur.cpu(), i_cur.cpu())), want)
    # metropolis_chain, piece by piece against the CPU chain of the same piece
    o, carry, ccarry = 0, None, None
    for n in PIECES:
        cut = slice(o, o + n)
        ql = None if lq is None else lq[:, cut]
        wantp = cpu_chain(e[:, cut], r[:, cut], ql, carry=ccarry, base=BASE + o)
        gotp = run_kernel(e[:, cut], r[:, cut], ql, carry=carry, base=BASE + o)
        same(gotp, wantp)
        carry, ccarry = gotp[3], wantp[3]
        o += n
    assert torch.equal(carry[0], want[3][0]) and torch.equal(carry[2], want[3][2])


def test_each_output_absent_in_turn(hip_device):
    C, N = 5, 130
    e, r, lq = draws(C, N, 33, True)
    want = cpu_chain(e, r, lq)
    de, dr, dq = dev(e), dev(r), dev(lq)
    for absent in ("state", "accepted", "naccept", "carry"):
        out = dict(state=torch.full((C, N), -7, dtype=torch.int32, device=DEV),
                   accepted=torch.full((C, N), 9, dtype=torch.uint8, device=DEV),
                   naccept=torch.full((C,), 5, dtype=torch.int32, device=DEV))
        cur = dict(e_cur=torch.empty(C, device=DEV), lq_cur=torch.empty(C, device=DEV),
                   idx_cur=torch.empty(C, dtype=torch.int32, device=DEV))
        if absent == "carry":
            cur = {}
        else:
            del out[absent]
        K_.metropolize(de, dr, lq=dq, **out, **cur)
        if "state" in out:
            assert torch.equal(out["state"].cpu(), want[0])
        if "accepted" in out:
            assert torch.equal(out["accepted"].cpu().bool(), want[1])
        if "naccept" in out:
            assert torch.equal(out["naccept"].cpu(), want[2] + 5)  # added to
        if cur:
            assert torch.equal(cur["e_cur"].cpu(), want[3][0]) and torch.equal(cur["lq_cur"].cpu(), want[3][1])
            assert torch.equal(cur["idx_cur"].cpu(), want[3][2])


def test_nan_and_inf_rules(hip_device):
    """tests/test_reweight_cpu.py's cases: the expected flags are written out, no exp is near a threshold."""
    nan, inf = float("nan"), float("inf")

    def flags(e, r, lq=None, base=0):
        s, a, k, c = R.metropolis_chain(dev(torch.tensor(e)), dev(r), None if lq is None else dev(torch.tensor(lq)),
                                        base=base)
        assert int(k) == int(a.sum())
        return a.tolist(), s.tolist(), float(c[0]), int(c[2])

    a, s, ec, ic = flags([1.0, nan, 1.0, inf, 1.0, 5.0, 1.0, 0.5], torch.full((8,), 0.999))
    assert a == [True, False, True, False, True, False, True, True]
    assert s == [0, 0, 2, 2, 4, 4, 6, 7] and ec == 0.5 and ic == 7
    a, s, ec, ic = flags([1.0, -inf, -5.0, -1e30, -inf, 0.0, nan, inf], torch.zeros(8))
    assert a == [True, True] + [False] * 6 and s == [0] + [1] * 7 and ec == -inf and ic == 1
    a, _, _, _ = flags([1.0, 0.0, 0.0, 3.0], torch.full((4,), 0.5), [0.0, nan, 0.0, -5.0])
    assert a == [True, False, True, True]
    a, s, _, _ = flags([nan, 0.0, 1.0], torch.zeros(3), base=7)
    assert a == [False] * 3 and s == [7] * 3
    # the same rules past a block boundary and in its tail
    e = torch.zeros(2, 70)
    e[0, 64], e[0, 66], e[1, 65], e[1, 67] = nan, inf, -inf, -1.0
    r = torch.full((2, 70), 0.999)
    got = R.metropolis_chain(dev(e), dev(r))
    want = R.metropolis_chain(e, r)
    assert want[1][0].tolist() == [i not in (64, 66) for i in range(70)]
    assert want[1][1].tolist() == [i <= 65 for i in range(70)]
    same((got[0].cpu(), got[1].cpu(), got[2].cpu(), (got[3][0].cpu(), None, got[3][2].cpu())), want)


def test_argument_errors(hip_device):
    e, r = torch.zeros(2, 8, device=DEV), torch.zeros(2, 8, device=DEV)
    with pytest.raises(ValueError, match="lq and lq_cur come together"):
        K_.metropolize(e, r, lq_cur=torch.zeros(2, device=DEV))
    with pytest.raises(ValueError, match="e_cur and idx_cur come together"):
        K_.metropolize(e, r, e_cur=torch.zeros(2, device=DEV))
    with pytest.raises(ValueError, match="carry_in needs"):
        K_.metropolize(e, r, carry_in=True)
    with pytest.raises(ValueError, match="fit int32"):
        K_.metropolize(e, r, base=2 ** 31 - 8)
    with pytest.raises(ValueError, match="state must be"):
        K_.metropolize(e, r, state=torch.zeros(2, 8, device=DEV))
    with pytest.raises(RuntimeError, match="ROCm device only"):
        K_.metropolize(e.cpu(), r)


# ------------------------------------------------------------- applications
def crystal_and_model():
    """An Einstein crystal of 4 atoms x 3 as the target and a 2-layer NSF_AR
    flow over a wider crystal on the same sites."""
    centers = torch.tensor([[-0.75, -0.75, -0.75], [0.75, 0.75, -0.75], [0.75, -0.75, 0.75], [-0.75, 0.75, 0.75]])
    target = systems.EinsteinCrystal(centers, 3, alpha=28, device=DEV)  # alpha / kT = the prior's 40
    prior = systems.EinsteinCrystal(centers, 3, alpha=40, device=DEV)
    torch.manual_seed(1234)
    model = nfm.NormalizingFlowModel(prior, [nff.NSF_AR(dim=12, K=8, B=3, hidden_dim=16) for _ in range(2)]).to(DEV)
    cfg = app.get_cfg_defaults()
    cfg.device, cfg.dataset.kT, cfg.dataset.dim, cfg.dataset.nparticles = DEV, 0.7, 3, 4
    return cfg, target, model


def both_paths(fn):
    """fn() on the kernel path (one launch) and on the torch path."""
    out = {}
    n = counts_of(lambda: out.update(kernel=fn()))
    assert n.get("nfk_metropolize") == 1, n
    R.use_kernels = False
    try:
        n = counts_of(lambda: out.update(torch=fn()))
    finally:
        R.use_kernels = True
    assert "nfk_metropolize" not in n, n
    return out["kernel"], out["torch"]


def test_app_metropolize_on_both_paths_and_under_capture(hip_device, monkeypatch):
    cfg, target, model = crystal_and_model()
    N, BURNIN = 130, 20
    torch.manual_seed(77)
    with torch.no_grad():
        x, lq = app.generate_from_nf(model, N, batchsize=N)
    e = (target.potential(x.reshape(-1, 4, 3)) / cfg.dataset.kT).detach()  # once, on the device
    for log_q in (None, lq):
        r = torch.rand(N, generator=torch.Generator(DEV).manual_seed(3), device=DEV)
        want = cpu_chain(e.cpu()[None], r.cpu()[None], None if log_q is None else log_q.cpu()[None])
        print("app.metropolize %s: %d of %d accepted" % ("energy" if log_q is None else "lq", int(want[2]), N))
        assert 1 <= int(want[2]) <= N

        def default():
            return app.metropolize(cfg, target, x, BURNIN, log_q=log_q, generator=torch.Generator(DEV).manual_seed(3))

        def chain():
            return app.metropolize(cfg, target, x, BURNIN, log_q=log_q, return_chain=True,
                                   generator=torch.Generator(DEV).manual_seed(3))

        (kx, ke), (tx, te) = both_paths(default)
        index = want[1][0].clone()
        index[:BURNIN + 1] = False
        assert kx.is_cuda and kx.shape == (int(index.sum()), 4, 3) and torch.equal(kx, tx) and torch.equal(ke, te)
        assert torch.equal(kx.cpu(), x.cpu().reshape(N, 4, 3)[index]) and torch.equal(ke.cpu(), e.cpu()[want[1][0]])
        (kx, ke, ka), (tx, te, ta) = both_paths(chain)
        kept = want[0][0, BURNIN + 1:].long()
        assert kx.shape == (N - BURNIN - 1, 4, 3) and torch.equal(kx, tx) and torch.equal(ke, te)
        assert torch.equal(kx.cpu(), x.cpu().reshape(N, 4, 3)[kept]) and torch.equal(ke.cpu(), e.cpu()[kept])
        assert ka.dim() == 0 and float(ka) == float(ta) == int(want[2]) / N

    # return_chain=True under capture: nothing synchronises once the potential's NaN check is off
    monkeypatch.setattr(config, "STRICT_CHECKS", False)

    def captured():
        return app.metropolize(cfg, target, x, BURNIN, log_q=lq, return_chain=True)

    side = torch.cuda.Stream(DEV)
    side.wait_stream(torch.cuda.current_stream(DEV))
    with torch.cuda.stream(side):
        captured()
    torch.cuda.current_stream(DEV).wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = captured()
    torch.manual_seed(9)
    eager = [t.clone() for t in captured()]
    for _ in range(2):  # the uniforms come from the default generator: the same seed, the same output
        torch.manual_seed(9)
        graph.replay()
        torch.cuda.synchronize()
        assert all(torch.equal(a, b) for a, b in zip(out, eager))
    torch.manual_seed(10)
    graph.replay()
    torch.cuda.synchronize()
    torch.manual_seed(10)
    assert all(torch.equal(a, b) for a, b in zip(out, captured()))


def test_app_metropolized_samples_on_both_paths(hip_device):
    cfg, target, model = crystal_and_model()
    N, CHAINS, BURNIN = 130, 3, 10

    def run():
        torch.manual_seed(77)
        return app.metropolized_samples(cfg, model, target, N, batchsize=N, chains=CHAINS, burnin=BURNIN,
                                        generator=torch.Generator(DEV).manual_seed(3))

    # the same seeded draws, the energies once on the device, the CPU chain and its margin
    torch.manual_seed(77)
    with torch.no_grad():
        x, lq = app.generate_from_nf(model, CHAINS * N, batchsize=N)
    e = (target.potential(x.reshape(-1, 4, 3)) / cfg.dataset.kT).detach().reshape(CHAINS, N)
    r = torch.rand(CHAINS, N, generator=torch.Generator(DEV).manual_seed(3), device=DEV)
    want = cpu_chain(e.cpu(), r.cpu(), lq.cpu().reshape(CHAINS, N))
    print("metropolized_samples: accepted %s of %d" % (want[2].tolist(), N))
    (kx, ka, ks), (tx, ta, ts) = both_paths(run)
    assert kx.is_cuda and kx.shape == (CHAINS, N - BURNIN, 12) and ka.shape == (CHAINS,) and ks.shape == (CHAINS,)
    assert ka.dtype == torch.float64 and ks.dtype == torch.float64
    assert torch.equal(kx, tx) and torch.equal(ka, ta) and torch.equal(ks, ts)
    rows = x.cpu().reshape(CHAINS, N, 12)
    for c in range(CHAINS):
        assert torch.equal(kx[c].cpu(), rows[c][want[0][c, BURNIN:].long()])
    assert torch.equal(ka.cpu(), want[2].double() / N)
    # fp64 log-sum-exps of 130 fp32 weights on two devices: the inputs are equal, the sums' order is not
    torch.testing.assert_close(ks.cpu(), R.ess(R.log_weights(lq.cpu().reshape(CHAINS, N), e.cpu())), rtol=1e-12,
                               atol=0)
    assert bool((ks >= 1).all()) and bool((ks <= N).all())
    with pytest.raises(ValueError, match="multiple of batchsize"):
        app.metropolized_samples(cfg, model, target, N, batchsize=100, chains=CHAINS)
