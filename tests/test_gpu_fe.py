"""GPU checks of the free-energy layer: the nfk_bar kernel (nfk_bar.hip) against
the ``fe_bar_*`` golden vectors and against the fp64 CPU path of
``normalizingflow_amd.bar`` on the same index rows, the shapes at which its
mapping changes, bitwise repeatability, its argument errors, and
``app.fe_estimates`` / ``app.fe_diff`` on the device.

Tolerances are tests/test_fe_cpu.py's: tol = 64 (n_f + n_r) 2^-53 max(1, |Delta|).
"""
import math

import pytest
import torch

import nf.flows as nff
import nf.models as nfm
from normalizingflow_amd import _lib, app, systems
from normalizingflow_amd import bar as B
from normalizingflow_amd import kernels as K_
from test_fe_cpu import BAR_CASES, boot_indices, case_tol, check_against_fixture, fixture, tol_of
from test_gpu_systems import counts_of

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def ksolve(wf, wr, idx_f=None, idx_r=None, **kw):
    """bar_solve on device copies: the kernel path."""
    out, iters = B.bar_solve(wf.to(DEV), wr.to(DEV), idx_f=None if idx_f is None else idx_f.to(DEV),
                             idx_r=None if idx_r is None else idx_r.to(DEV), **kw)
    assert out.is_cuda and out.dtype == torch.float64 and iters.is_cuda and iters.dtype == torch.int32
    return out.cpu(), iters.cpu()


def tiled(n_f, n_r):
    """n_f / n_r work values by tiling the 500 / 400 fixture's."""
    _, data = fixture("fe_bar_n500_d37")
    return data["w_f"][torch.arange(n_f) % 500].clone(), data["w_r"][torch.arange(n_r) % 400].clone()


# ---------------------------------------------------------------- fixtures
@pytest.mark.parametrize("name", BAR_CASES)
def test_kernel_against_fixture(name, hip_device):
    _, data = fixture(name)
    check_against_fixture(lambda **kw: ksolve(data["w_f"], data["w_r"], **kw), data, "kernel " + name)
    first, iters = ksolve(data["w_f"], data["w_r"], maximum_iterations=1)
    assert int(iters[0]) == 1 and abs(float(first[0, 0]) - float(data["hist_64"][0])) <= case_tol(data)


def test_one_launch_and_device_results(hip_device):
    _, data = fixture("fe_bar_n500_d37")
    wf, wr = data["w_f"].to(DEV), data["w_r"].to(DEV)
    n = counts_of(lambda: B.bootstrap(wf, wr, 200, generator=torch.Generator(DEV).manual_seed(1)))
    assert n.get("nfk_bar") == 1, n
    v = B.BAR(wf, wr)
    assert torch.is_tensor(v) and v.is_cuda and v.dim() == 0 and v.dtype == torch.float64
    assert abs(float(v) - float(data["bar_64"])) <= case_tol(data)
    B.use_kernels = False
    try:  # the torch path on the device
        assert counts_of(lambda: B.bar_solve(wf, wr)).get("nfk_bar") is None
        o, i = B.bar_solve(wf, wr)
    finally:
        B.use_kernels = True
    assert o.is_cuda and abs(float(o[0, 0]) - float(data["bar_64"])) <= case_tol(data)
    assert int(i[0]) == int(data["iters_64"])


# ------------------------------------------------ kernel against the CPU path
@pytest.mark.parametrize("name", ["fe_bar_n37_d07", "fe_bar_n500_d37", "fe_bar_n500_dm3", "fe_bar_n500_d300"])
def test_kernel_equals_cpu_path_on_the_same_indices(name, hip_device):
    _, data = fixture(name)
    wf, wr = data["w_f"], data["w_r"]
    idx_f, idx_r = boot_indices(3, wf.numel(), wr.numel(), 17)
    ref, ref_iters = B.bar_solve(wf, wr, idx_f=idx_f, idx_r=idx_r)
    out, iters = ksolve(wf, wr, idx_f, idx_r)
    tol = case_tol(data)
    print(name, "max err", float((out - ref).abs().max()), "tol", tol, "iters", iters.tolist())
    assert torch.equal(iters, ref_iters)
    assert float((out - ref).abs().max()) <= tol


def _shapes():
    cap = 32768  # asserted against bar_stage_cap() in the test
    return [(1, 1), (1, 65), (64, 64), (65, 64), (64, 65),
            (257, 200), (513, 1600), (1025, 70000),          # a side of blockDim + 1 at 256, 512 and 1024 threads
            (1024, 1024), (1025, 1024),                      # 2048 values: 256 threads; 2049: 512
            (cap // 2, cap - cap // 2), (cap // 2 + 1, cap - cap // 2),  # the LDS cap (staged), cap + 1 (streamed)
            (32768, 32768), (32769, 32768)]                  # 65536 values: 512 threads; 65537: 1024


@pytest.mark.parametrize("n_f,n_r", _shapes())
def test_shapes_where_the_mapping_changes(n_f, n_r, hip_device):
    """One value, one side of one value, a wave, a wave + 1, a workgroup + 1 at
    each of the kernel's three workgroup sizes, the two sizes at which the
    workgroup size changes, the LDS cap exactly (staged form) and the cap + 1
    (streamed form)."""
    cap = K_.bar_stage_cap()
    assert cap == 32768
    wf, wr = tiled(n_f, n_r)
    for kw in (dict(relative_tolerance=0.0, maximum_iterations=6), dict()):
        ref, ref_iters = B.bar_solve(wf, wr, **kw)
        out, iters = ksolve(wf, wr, **kw)
        tol = tol_of(n_f, n_r, ref[0, 0])
        print((n_f, n_r), kw, "err", (out - ref).abs().max().item(), "tol", tol, "iters", int(iters[0]))
        assert torch.equal(iters, ref_iters)
        assert float((out - ref).abs().max()) <= tol


def test_staged_and_streamed_forms_agree(hip_device):
    """The form is chosen by n_f + n_r alone, so the public ABI cannot run one
    problem in both forms, and a value added or removed changes n, M and every
    sum.  What can be checked: the cap-sized problem (staged) and the same
    problem with one forward value repeated (streamed) differ by what the fp64
    CPU path says they differ by, within the two tolerances."""
    cap = K_.bar_stage_cap()
    wf, wr = tiled(cap // 2 + 1, cap - cap // 2)
    kw = dict(relative_tolerance=0.0, maximum_iterations=5)
    staged, streamed = ksolve(wf[:-1], wr, **kw)[0], ksolve(wf, wr, **kw)[0]
    ref_a, ref_b = B.bar_solve(wf[:-1], wr, **kw)[0], B.bar_solve(wf, wr, **kw)[0]
    tol = tol_of(cap // 2 + 1, cap - cap // 2, ref_b[0, 0])
    assert float(((staged - streamed) - (ref_a - ref_b)).abs().max()) <= 2 * tol


# ------------------------------------------------------------- repeatability
@pytest.mark.parametrize("n_f,n_r", [(500, 400), (20000, 12769), (40000, 30000)])
def test_bitwise_repeatable_and_index_forms(n_f, n_r, hip_device):
    wf, wr = tiled(n_f, n_r)
    idx_f, idx_r = boot_indices(3, n_f, n_r, 23)
    a, ia = ksolve(wf, wr, idx_f, idx_r)
    b, ib = ksolve(wf, wr, idx_f, idx_r)
    assert torch.equal(a, b) and torch.equal(ia, ib)
    plain, ip = ksolve(wf, wr)
    ident_f = torch.arange(n_f, dtype=torch.int32).reshape(1, -1)
    ident_r = torch.arange(n_r, dtype=torch.int32).reshape(1, -1)
    ident, ii = ksolve(wf, wr, ident_f, ident_r)
    assert torch.equal(plain, ident) and torch.equal(ip, ii)
    four, i4 = ksolve(wf, wr, idx_f[1:2].expand(4, -1), idx_r[1:2].expand(4, -1))
    assert all(torch.equal(four[p], a[1]) for p in range(4)) and i4.tolist() == [int(ia[1])] * 4
    # a problem on gathered rows is the plain problem on the gathered vectors
    g, ig = ksolve(wf[idx_f[2].long()], wr[idx_r[2].long()])
    assert torch.equal(g[0], a[2]) and int(ig[0]) == int(ia[2])


def test_more_problems_than_the_grid_holds(hip_device):
    wf, wr = tiled(37, 29)
    P = 4096 + 5  # the kernel's grid cap is 4096 workgroups
    idx_f, idx_r = boot_indices(8, 37, 29, 31)
    rows = torch.arange(P) % 8
    out, iters = ksolve(wf, wr, idx_f[rows], idx_r[rows])
    base, ib = ksolve(wf, wr, idx_f, idx_r)
    assert torch.equal(out, base[rows]) and torch.equal(iters, ib[rows])


def test_non_finite_and_large_exponents(hip_device):
    inf = float("inf")
    wf, wr = tiled(37, 29)
    for f, r in ((torch.full((3,), inf), wr), (wf, torch.cat((wr, torch.tensor([-inf]))))):
        out, iters = ksolve(f, r, maximum_iterations=50)
        assert math.isnan(float(out[0, 0])) and int(iters[0]) == 1
    for w in (900.0, -900.0):  # tests/test_fe_cpu.py derives these values
        out, iters = ksolve(torch.tensor([w]), torch.tensor([-w]), maximum_iterations=1)
        assert float(out[0, 0]) == w and int(iters[0]) == 1
        out, iters = ksolve(torch.tensor([w]), torch.tensor([-w]))
        assert abs(float(out[0, 0]) - w) <= 2 * 2.0 ** -43 and int(iters[0]) == 2


# ------------------------------------------------------------ argument errors
def test_argument_errors_launch_nothing(hip_device):
    lib = _lib.load()
    wf = torch.zeros(8, device=DEV)
    wr = torch.zeros(6, device=DEV)
    jf = torch.zeros(2, 8, dtype=torch.int32, device=DEV)
    jr = torch.zeros(2, 6, dtype=torch.int32, device=DEV)
    out = torch.full((2, 3), 7.0, dtype=torch.float64, device=DEV)
    it = torch.full((2,), 7, dtype=torch.int32, device=DEV)
    ok = dict(w_f=wf.data_ptr(), n_f=8, w_r=wr.data_ptr(), n_r=6, idx_f=jf.data_ptr(), ldif=8,
              idx_r=jr.data_ptr(), ldir=6, problems=2, delta0=0.0, max_iterations=10, rtol=1e-5,
              out=out.data_ptr(), iters=it.data_ptr(), stream=None)
    bad = [(dict(n_f=0), b"n_f and n_r"), (dict(n_r=0), b"n_f and n_r"), (dict(n_f=-3), b"n_f and n_r"),
           (dict(problems=0), b"problems"), (dict(max_iterations=0), b"max_iterations"),
           (dict(rtol=-1e-9), b"rtol"), (dict(rtol=float("nan")), b"rtol"),
           (dict(ldif=7), b"leading dimension"), (dict(ldir=5), b"leading dimension"),
           (dict(out=None), b"null out or iters"), (dict(iters=None), b"null out or iters"),
           (dict(idx_f=None), b"come together"), (dict(idx_r=None), b"come together")]
    for change, msg in bad:
        assert lib.nfk_bar(*{**ok, **change}.values()) == _lib.NFK_EINVAL, change
        assert msg in lib.nfk_last_error(), (change, lib.nfk_last_error())
    torch.cuda.synchronize()
    assert bool((out == 7.0).all()) and bool((it == 7).all())
    with pytest.raises(ValueError, match="come together"):
        K_.bar(wf, wr, out, it, idx_f=jf)
    with pytest.raises(ValueError, match="int32"):
        K_.bar(wf, wr, out, it, idx_f=jf.long(), idx_r=jr)
    with pytest.raises(RuntimeError, match="ROCm device only"):
        K_.bar(wf.cpu(), wr, out, it)


# ------------------------------------------------------------- applications
def test_fe_estimates_on_the_device(hip_device):
    meta, data = fixture("fe_q_lj")
    cfg = app.get_cfg_defaults()
    cfg.dataset.nparticles, cfg.dataset.kT = meta["nparticles"], meta["kT"]
    Q = data["Q"].to(DEV)
    res = app.fe_estimates(cfg, Q)
    ref = app.fe_estimates(cfg, data["Q"])
    assert torch.equal(Q.cpu(), data["Q"])
    tol = tol_of(64, 64, data["delta_64"])
    for ours, want, key in zip(res, ref, ("bar", "md", "nf")):
        assert ours.is_cuda and ours.dim() == 0 and ours.dtype == torch.float64
        assert abs(float(ours) - float(want)) <= tol
        assert abs(float(ours) - float(data[key])) <= tol
    six = app.fe_estimates(cfg, Q, nboot=50, generator=torch.Generator(DEV).manual_seed(5))
    assert len(six) == 6 and all(t.is_cuda and t.dim() == 0 for t in six)
    assert all(0.0 < float(e) < 1.0 for e in six[3:])


@pytest.mark.parametrize("relaxation", [False, True])
def test_fe_diff_on_a_small_model(relaxation, hip_device):
    """2 x NSF_AR over an Einstein-crystal prior on 4 atoms x 3, a Lennard-Jones
    target holding a 4-frame trajectory: fe_diff is fe_estimates of the Q that
    the same seeded calls produce."""
    L = 6.0
    centers = torch.tensor([[-0.75, -0.75, -0.75], [0.75, 0.75, -0.75], [0.75, -0.75, 0.75], [-0.75, 0.75, 0.75]])
    prior = systems.EinsteinCrystal(centers, 3, boxlength=L, alpha=600, device=DEV)
    torch.manual_seed(1234)
    model = nfm.NormalizingFlowModel(prior, [nff.NSF_AR(dim=12, K=8, B=3, hidden_dim=16) for _ in range(2)]).to(DEV)
    frames = centers + 0.02 * torch.randn(4, 4, 3, generator=torch.Generator().manual_seed(6))
    lj = systems.LJ(pos_dir=frames, boxlength=L, device=DEV, cutoff=1.6, shift=True)
    cfg = app.get_cfg_defaults()
    cfg.device, cfg.dataset.kT, cfg.dataset.dim, cfg.dataset.nparticles = DEV, 0.7, 3, 4
    kw = dict(relaxation_kw=dict(path_len=2)) if relaxation else {}
    torch.manual_seed(77)
    res = app.fe_diff(cfg, model, lj, 500, relaxation=relaxation, batchsize=500, **kw)
    torch.manual_seed(77)
    if relaxation:
        Q = app.q_matrix_relaxed(cfg, model, lj, 500, batchsize=500, path_len=2)
    else:
        Q = app.q_matrix(cfg, model, lj, 500, batchsize=500)
    assert Q.shape == (2, 500, 2) and Q.is_cuda
    want = app.fe_estimates(cfg, Q)
    assert len(res) == 3
    for ours, ref in zip(res, want):
        assert ours.is_cuda and ours.dim() == 0 and ours.dtype == torch.float64
        assert math.isfinite(float(ours)) and float(ours) == float(ref)
    torch.manual_seed(77)
    six = app.fe_diff(cfg, model, lj, 500, relaxation=relaxation, return_err=True, nboot=20, batchsize=500,
                      generator=torch.Generator(DEV).manual_seed(3), **kw)
    assert len(six) == 6 and all(float(a) == float(b) for a, b in zip(six[:3], res))
    assert all(math.isfinite(float(e)) and float(e) >= 0.0 for e in six[3:])
