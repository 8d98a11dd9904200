"""GPU checks of the multistate layer: the nfk_mbar kernel (nfk_mbar.hip) against
the ``mbar_*`` golden vectors and against the fp64 CPU path of
``normalizingflow_amd.mbar`` on the same rows, the shapes at which its mapping
changes, bitwise repeatability, its argument errors, and ``app.fe_estimates`` /
``app.fe_diff`` with ``emus=True`` on the device.

Tolerances are tests/test_mbar_cpu.py's: tol = 64 N 2^-53 max(1, max|f|)
max(1, kappa), kappa from the fixture or, for shapes no fixture holds, from the
CPU run compared with (``cpu_reference``).
"""
import math

import pytest
import torch

import nf.flows as nff
import nf.models as nfm
from normalizingflow_amd import _lib, app, systems
from normalizingflow_amd import kernels as K_
from normalizingflow_amd import mbar as M
from test_gpu_systems import counts_of
from test_mbar_cpu import MBAR_CASES, boot_rows, case_tol, check_against_fixture, cpu_reference, fixture

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
BASE = {2: "mbar_k2_n500_d37", 3: "mbar_k3_wells", 8: "mbar_k8_wells"}


def ksolve(u, n_k, idx=None, **kw):
    """mbar_solve on device copies: the kernel path."""
    out = {}

    def run():
        out["r"] = M.mbar_solve(u.to(DEV), n_k, idx=None if idx is None else idx.to(DEV), **kw)

    n = counts_of(run)
    assert n.get("nfk_mbar") == 1, n
    f, iters, gram = out["r"]
    assert f.is_cuda and f.dtype == torch.float64 and iters.is_cuda and iters.dtype == torch.int32
    assert gram.is_cuda and gram.dtype == torch.float64
    return f.cpu(), iters.cpu(), gram.cpu()


def tiled(K, N):
    """N samples of K states by tiling a fixture's, state by state, in the
    fixture's proportions (every state keeps at least one): (u, n_k)."""
    _, data = fixture(BASE[K])
    base = data["n_k"]
    n_k = [max(1, N * b // sum(base)) for b in base]
    n_k[n_k.index(max(n_k))] += N - sum(n_k)
    assert sum(n_k) == N and min(n_k) >= 1
    rows, o = [], 0
    for b, n in zip(base, n_k):
        rows.append(o + torch.arange(n) % b)
        o += b
    return data["u"][torch.cat(rows)].clone(), n_k


def compare(u, n_k, idx=None, **kw):
    ref_f, ref_iters, ref_gram, tol = cpu_reference(u, n_k, idx, **kw)
    f, iters, gram = ksolve(u, n_k, idx, **kw)
    for p in range(f.shape[0]):
        err, gerr = float((f[p] - ref_f[p]).abs().max()), float((gram[p] - ref_gram[p]).abs().max())
        print("K %d N %d %s problem %d: err %.3g gram err %.3g tol %.3g iters %d" % (
            len(n_k), sum(n_k), kw, p, err, gerr, tol[p], int(iters[p])))
        assert int(iters[p]) == int(ref_iters[p])
        assert err <= tol[p] and gerr <= tol[p]
    return f, iters, gram


# ---------------------------------------------------------------- fixtures
@pytest.mark.parametrize("name", MBAR_CASES)
def test_kernel_against_fixture(name, hip_device):
    _, data = fixture(name)
    check_against_fixture(lambda **kw: ksolve(data["u"], data["n_k"], **kw), data, "kernel " + name)
    f, iters, _ = ksolve(data["u"], data["n_k"], f0=data["f_root"] + 3.0)  # a start at the root, gauge taken out
    assert int(iters[0]) == 1 and float((f[0] - data["f_root"]).abs().max()) <= case_tol(data)


def test_one_launch_device_results_and_the_torch_path(hip_device):
    _, data = fixture("mbar_k3_wells")
    u, n_k = data["u"].to(DEV), data["n_k"]
    n = counts_of(lambda: M.bootstrap(u, n_k, 200, generator=torch.Generator(DEV).manual_seed(1)))
    assert n.get("nfk_mbar") == 1, n
    f, iters, gram = M.bootstrap(u, n_k, 200, generator=torch.Generator(DEV).manual_seed(1))
    assert f.shape == (200, 3) and f.is_cuda and iters.shape == (200,) and gram.shape == (200, 3, 3)
    sd = M.mbar_std(M.mbar_solve(u, n_k)[2], n_k, 0, 2)
    assert sd.is_cuda and sd.shape == (1,)
    assert float(f[:, 2].std()) / 1.5 <= float(sd[0]) <= float(f[:, 2].std()) * 1.5
    M.use_kernels = False
    try:  # the torch path on the device
        assert counts_of(lambda: M.mbar_solve(u, n_k)).get("nfk_mbar") is None
        o, i, g = M.mbar_solve(u, n_k)
    finally:
        M.use_kernels = True
    assert o.is_cuda and i.is_cuda and g.is_cuda
    assert float((o[0].cpu() - data["hist_64"][-1]).abs().max()) <= case_tol(data)
    assert int(i[0]) == int(data["iters_64"])
    # fp64 energies are the torch path's as well
    assert counts_of(lambda: M.mbar_solve(u.double(), n_k)).get("nfk_mbar") is None


def test_results_without_a_host_sync(hip_device):
    meta, d = fixture("mbar_k3_wells")
    u, n_k = d["u"].to(DEV), d["n_k"]
    idx = boot_rows(4, n_k, 5).to(DEV)
    import golden_io as gio
    qmeta, qdata, _ = gio.load("fe_q_lj")
    cfg = app.get_cfg_defaults()
    cfg.dataset.nparticles, cfg.dataset.kT = qmeta["nparticles"], qmeta["kT"]
    Q = qdata["Q"].to(DEV)
    M.mbar_solve(u, n_k)  # the library is loaded and the kernel's attributes are set
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        f, iters, gram = M.mbar_solve(u, n_k)
        fb, _, _ = M.mbar_solve(u, n_k, idx=idx)
        sd = M.mbar_std(gram, n_k, 0, 1)
        four = app.fe_estimates(cfg, Q, emus=True)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert all(t.is_cuda for t in (f, iters, gram, fb, sd) + four)
    assert float((f[0].cpu() - d["hist_64"][-1]).abs().max()) <= case_tol(d)
    want = app.fe_estimates(cfg, qdata["Q"], emus=True)
    Qs = qdata["Q"] - torch.stack((qdata["Q"][1][:, 0].min(), qdata["Q"][1][:, 1].min()))
    tol = cpu_reference((-Qs).reshape(-1, 2), [64, 64])[3][0] / qmeta["nparticles"] * qmeta["kT"]
    assert abs(float(four[3]) - float(want[3])) <= tol and four[3].dim() == 0


# ------------------------------------------------ kernel against the CPU path
@pytest.mark.parametrize("name", ["mbar_k2_n37_d07", "mbar_k2_n500_d300", "mbar_k3_wells", "mbar_k8_wells"])
def test_kernel_equals_cpu_path_on_the_same_rows(name, hip_device):
    _, data = fixture(name)
    compare(data["u"], data["n_k"], boot_rows(3, data["n_k"], 17))


def _shapes():
    cap = 32768  # asserted against mbar_stage_cap() in the test
    out = []
    for K in (2, 3, 8):
        small, mid = 2048 // K, 65536 // K
        out += [(K, n) for n in (
            K, 65,                       # one sample per state (N = 2 at K = 2); a wave + 1
            257, 1025,                   # a workgroup + 1 at 256 threads (K = 8: within 512) and at 512
            small, small + 1,            # N K at the 256 / 512 threshold and past it
            cap // K, cap // K + 1,      # the LDS cap (staged) and one sample past it (streamed)
            mid, mid + 1)]               # N K at the 512 / 1,024 threshold and past it (K = 8 stays at 512)
    return list(dict.fromkeys(out))


@pytest.mark.parametrize("K,N", _shapes())
def test_shapes_where_the_mapping_changes(K, N, hip_device):
    assert K_.mbar_stage_cap() == 32768 and K_.mbar_supported(K)
    u, n_k = tiled(K, N)
    compare(u, n_k, relative_tolerance=0.0, maximum_iterations=3)
    compare(u, n_k)


# ------------------------------------------------------------- repeatability
@pytest.mark.parametrize("K,N", [(2, 900), (8, 5000), (3, 25000)])  # staged 256 threads, streamed 512, streamed 1,024
def test_bitwise_repeatable_and_index_forms(K, N, hip_device):
    u, n_k = tiled(K, N)
    idx = boot_rows(3, n_k, 23)
    a = ksolve(u, n_k, idx)
    b = ksolve(u, n_k, idx)
    assert all(torch.equal(x, y) for x, y in zip(a, b))
    plain = ksolve(u, n_k)
    ident = ksolve(u, n_k, torch.arange(N, dtype=torch.int32).reshape(1, -1))
    assert all(torch.equal(x, y) for x, y in zip(plain, ident))
    four = ksolve(u, n_k, idx[1:2].expand(4, -1))
    assert all(torch.equal(four[j][p], a[j][1]) for p in range(4) for j in range(3))
    # a problem on gathered rows is the plain problem on the gathered matrix, padded rows or not
    g = ksolve(u[idx[2].long()], n_k)
    assert all(torch.equal(g[j][0], a[j][2]) for j in range(3))
    wide = torch.full((N, K + 3), float("nan"))
    wide[:, :K] = u
    w = M.mbar_solve(wide.to(DEV)[:, :K], n_k)  # row stride K + 3
    assert all(torch.equal(x.cpu(), y) for x, y in zip(w, plain))


def test_more_problems_than_the_grid_holds(hip_device):
    u, n_k = tiled(3, 30)
    P = 4096 + 5  # the kernel's grid cap is 4096 workgroups
    idx = boot_rows(8, n_k, 31)
    rows = torch.arange(P) % 8
    out = ksolve(u, n_k, idx[rows])
    base = ksolve(u, n_k, idx)
    assert all(torch.equal(o, b[rows]) for o, b in zip(out, base))


def test_nan_energy_ends_the_loop(hip_device):
    for K, N in ((3, 445), (8, 5000)):
        u, n_k = tiled(K, N)
        u[17, 1] = float("nan")
        f, iters, gram = ksolve(u, n_k, maximum_iterations=50)
        assert bool(torch.isnan(f[0, 1:]).all()) and int(iters[0]) == 1
        assert bool(torch.isnan(gram).any())


# ------------------------------------------------------------ argument errors
def test_argument_errors_launch_nothing(hip_device):
    import ctypes
    lib = _lib.load()
    u = torch.zeros(14, 3, device=DEV)
    jx = torch.zeros(2, 14, dtype=torch.int32, device=DEV)
    f = torch.full((2, 3), 7.0, dtype=torch.float64, device=DEV)
    it = torch.full((2,), 7, dtype=torch.int32, device=DEV)
    gram = torch.full((2, 3, 3), 7.0, dtype=torch.float64, device=DEV)

    def counts(*v):
        return (ctypes.c_int64 * len(v))(*v)

    ok = dict(u=u.data_ptr(), ldu=3, N=14, K=3, n_k=counts(8, 4, 2), idx=jx.data_ptr(), ldi=14, problems=2,
              f0=None, max_iterations=10, rtol=1e-8, f=f.data_ptr(), iters=it.data_ptr(), gram=gram.data_ptr(),
              stream=None)
    bad = [(dict(K=1), b"K must be"), (dict(K=9), b"K must be"), (dict(n_k=counts(8, 6, 0)), b"at least 1"),
           (dict(n_k=counts(8, 4, 3)), b"sum to N"), (dict(n_k=None), b"n_k given"), (dict(N=0), b"N must be"),
           (dict(problems=0), b"problems"), (dict(max_iterations=0), b"max_iterations"),
           (dict(rtol=-1e-9), b"rtol"), (dict(rtol=float("nan")), b"rtol"),
           (dict(ldu=2), b"leading dimension"), (dict(ldi=13), b"leading dimension"),
           (dict(u=None), b"null energies"), (dict(f=None), b"null f"), (dict(iters=None), b"null f"),
           (dict(gram=None), b"null f"), (dict(idx=None), b"needs idx")]
    for change, msg in bad:
        assert lib.nfk_mbar(*{**ok, **change}.values()) == _lib.NFK_EINVAL, change
        assert msg in lib.nfk_last_error(), (change, lib.nfk_last_error())
    torch.cuda.synchronize()
    assert bool((f == 7.0).all()) and bool((it == 7).all()) and bool((gram == 7.0).all())
    assert not K_.mbar_supported(1) and not K_.mbar_supported(9) and K_.mbar_supported(2) and K_.mbar_supported(8)
    with pytest.raises(ValueError, match="int32"):
        K_.mbar(u, [8, 4, 2], f, it, gram, idx=jx.long())
    with pytest.raises(ValueError, match="at least 1"):
        K_.mbar(u, [10, 4, 0], f, it, gram, idx=jx)
    with pytest.raises(ValueError, match="columns"):
        K_.mbar(u, [10, 4], f, it, gram, idx=jx)
    with pytest.raises(ValueError, match="2 <= K <= 8"):
        K_.mbar(torch.zeros(14, 9, device=DEV), [6] + [1] * 8, torch.zeros(1, 9, dtype=torch.float64, device=DEV),
                it[:1], torch.zeros(1, 9, 9, dtype=torch.float64, device=DEV))
    with pytest.raises(ValueError, match="one problem"):
        K_.mbar(u, [8, 4, 2], f, it, gram)
    with pytest.raises(RuntimeError, match="ROCm device only"):
        K_.mbar(u.cpu(), [8, 4, 2], f, it, gram, idx=jx)
    with pytest.raises(ValueError, match="at least 1"):
        M.mbar_solve(u, [12, 2, 0])


# ------------------------------------------------------------- applications
def test_fe_diff_with_emus_on_a_small_model(hip_device):
    """2 x NSF_AR over an Einstein-crystal prior on 4 atoms x 3, a Lennard-Jones
    target holding a 4-frame trajectory (tests/test_gpu_fe.py's model):
    ``fe_diff(..., emus=True, return_err=True)`` is ``fe_estimates`` of the Q
    that the same seeded calls produce, its first three estimates and errors
    are those of the call without ``emus``, and ``emus`` / ``emus_err`` are the
    fp64 CPU path's on the same Q."""
    L = 6.0
    centers = torch.tensor([[-0.75, -0.75, -0.75], [0.75, 0.75, -0.75], [0.75, -0.75, 0.75], [-0.75, 0.75, 0.75]])
    prior = systems.EinsteinCrystal(centers, 3, boxlength=L, alpha=600, device=DEV)
    torch.manual_seed(1234)
    model = nfm.NormalizingFlowModel(prior, [nff.NSF_AR(dim=12, K=8, B=3, hidden_dim=16) for _ in range(2)]).to(DEV)
    frames = centers + 0.02 * torch.randn(4, 4, 3, generator=torch.Generator().manual_seed(6))
    lj = systems.LJ(pos_dir=frames, boxlength=L, device=DEV, cutoff=1.6, shift=True)
    cfg = app.get_cfg_defaults()
    cfg.device, cfg.dataset.kT, cfg.dataset.dim, cfg.dataset.nparticles = DEV, 0.7, 3, 4
    torch.manual_seed(77)
    eight = app.fe_diff(cfg, model, lj, 500, return_err=True, nboot=20, batchsize=500, emus=True,
                        generator=torch.Generator(DEV).manual_seed(3))
    torch.manual_seed(77)
    six = app.fe_diff(cfg, model, lj, 500, return_err=True, nboot=20, batchsize=500,
                      generator=torch.Generator(DEV).manual_seed(3))
    torch.manual_seed(77)
    Q = app.q_matrix(cfg, model, lj, 500, batchsize=500)
    assert len(eight) == 8 and len(six) == 6
    assert all(t.is_cuda and t.dim() == 0 and t.dtype == torch.float64 for t in eight)
    assert all(math.isfinite(float(t)) for t in eight[:7])
    assert all(float(a) == float(b) for a, b in zip(eight[:3] + eight[4:7], six))
    four = app.fe_estimates(cfg, Q, emus=True)
    assert len(four) == 4 and all(float(a) == float(b) for a, b in zip(four, eight[:4]))
    # emus against the fp64 CPU path on the same Q
    ref = app.fe_estimates(cfg, Q.cpu(), emus=True, nboot=2, generator=torch.Generator().manual_seed(1))
    Qs = Q.cpu() - torch.stack((Q[1][:, 0].min(), Q[1][:, 1].min())).cpu()
    f, _, gram, tol = cpu_reference((-Qs).reshape(-1, 2), [500, 500])
    scale = cfg.dataset.kT / cfg.dataset.nparticles
    print("emus %.12g cpu %.12g err %.3g tol %.3g; emus_err %.4g cpu %.4g" % (
        float(eight[3]), float(ref[3]), abs(float(eight[3]) - float(ref[3])), tol[0] * scale, float(eight[7]),
        float(ref[7])))
    assert abs(float(eight[3]) - float(ref[3])) <= tol[0] * scale
    # The untrained flow and this target do not overlap (G_01 ~ 1e-54, so H_r = N_1 - G_11 is 0 in fp64):
    # the asymptotic error of such an estimate is inf, on both paths; a Q with overlap is
    # test_fe_estimates_emus_on_the_device's
    _check_emus_err(float(eight[7]) / scale, float(ref[7]) / scale, gram, 500, tol[0])
    assert float(eight[7]) == float("inf")


def _check_emus_err(sd, ref_sd, gram, n, tol):
    """Theta_00 + Theta_11 - 2 Theta_01 = 1 / H_r - 2 / n for two states of n samples, H_r = n - G_11:
    an error tol of G_11 moves the variance by tol / H_r^2."""
    h = n - float(gram[0, 1, 1])
    if h == 0.0:
        assert sd == ref_sd == float("inf")
    else:
        assert sd > 0.0 and abs(sd ** 2 - ref_sd ** 2) <= 2 * tol / h ** 2 + 1e-12 * ref_sd ** 2


def test_fe_estimates_emus_on_the_device(hip_device):
    import golden_io as gio
    meta, data, _ = gio.load("fe_q_lj")
    cfg = app.get_cfg_defaults()
    cfg.dataset.nparticles, cfg.dataset.kT = meta["nparticles"], meta["kT"]
    Q = data["Q"].to(DEV)
    eight = app.fe_estimates(cfg, Q, emus=True, nboot=50, generator=torch.Generator(DEV).manual_seed(5))
    six = app.fe_estimates(cfg, Q, nboot=50, generator=torch.Generator(DEV).manual_seed(5))
    assert torch.equal(Q.cpu(), data["Q"])
    assert len(eight) == 8 and all(t.is_cuda and t.dim() == 0 and t.dtype == torch.float64 for t in eight)
    assert all(float(a) == float(b) for a, b in zip(eight[:3] + eight[4:7], six))
    ref = app.fe_estimates(cfg, data["Q"], emus=True, nboot=2, generator=torch.Generator().manual_seed(1))
    Qs = data["Q"] - torch.stack((data["Q"][1][:, 0].min(), data["Q"][1][:, 1].min()))
    _, _, gram, tol = cpu_reference((-Qs).reshape(-1, 2), [64, 64])
    scale = meta["kT"] / meta["nparticles"]
    print("emus %.12g cpu %.12g tol %.3g; emus_err %.6g cpu %.6g bar_err %.6g" % (
        float(eight[3]), float(ref[3]), tol[0] * scale, float(eight[7]), float(ref[7]), float(eight[4])))
    assert abs(float(eight[3]) - float(ref[3])) <= tol[0] * scale
    assert 0.0 < float(eight[7]) < 1.0
    _check_emus_err(float(eight[7]) / scale, float(ref[7]) / scale, gram, 64, tol[0])
