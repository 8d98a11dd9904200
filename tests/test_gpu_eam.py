"""GPU checks of systems.EAM on nfk_eam.hip: the energy and its gradient at
every lane-group width and atoms-per-lane count, on Finnis-Sinclair-shaped
setfl tables (tests/eam_tables.py; Nr = Nrho = 2,000 unless stated).

There is no LAMMPS-generated golden.  The stand-in reference is the module's
fp32 torch path on the CPU and the truth is its fp64 torch path; both are
pinned against closed forms by tests/test_eam_cpu.py.  A case passes by
tests/test_gpu_systems.py's close_or_on_par (restated here): rtol 1e-5 /
atol 1e-4 against the fp32 reference, or our max and p99 error against fp64
within 2x the reference's own.
"""
import numpy as np
import pytest
import torch

import eam_tables as et
from normalizingflow_amd import app, systems
from normalizingflow_amd import kernels as K_

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
RTOL, ATOL = 1e-5, 1e-4
A_FE = 2.8841  # the Fe configs' cell_len


def close_or_on_par(ours, ref, truth, what, rtol=RTOL, atol=ATOL, factor=2.0):
    o, r, t = ours.detach().cpu().double(), ref.detach().cpu().double(), truth.double()
    eo, er = (o - t).abs().flatten(), (r - t).abs().flatten()
    qo, qr = torch.quantile(eo, 0.99).item(), torch.quantile(er, 0.99).item()
    print("%s: max |ours - ref| %.3g; vs fp64 max ours %.3g ref %.3g (ratio %.3g), p99 ours %.3g ref %.3g (ratio %.3g)"
          % (what, (o - r).abs().max(), eo.max(), er.max(), eo.max() / max(er.max().item(), 1e-30), qo, qr,
             qo / max(qr, 1e-30)))
    try:
        torch.testing.assert_close(o, r, rtol=rtol, atol=atol)
        return
    except AssertionError:
        pass
    assert eo.max().item() <= factor * er.max().item() + 1e-6, (what, eo.max().item(), er.max().item())
    assert qo <= factor * qr + 1e-6, (what, qo, qr)


def lattice(n, B, L, seed):
    """B perturbed rows of n atoms in a cubic box L: the first n sites of the
    smallest bcc lattice that has them, 4 % of the nearest-neighbour distance
    of jitter."""
    ncell = 1
    while 2 * ncell ** 3 < n:
        ncell += 1
    a = L / ncell
    pos = et.bcc(ncell, a, jitter=0.04 * a * 0.866, seed=seed, batch=B)
    return pos[:, :n]


def case(name):
    """(table, box, positions [B, n, 3] fp64) of a named case."""
    fe_scale = 0.61 * 3 * A_FE / 3.7  # rc = 0.61 L at the Fe box
    if name == "n1_self_images":
        tab = et.fs(rho_max=200.0)
        return tab, tab["rc"] / 1.2, np.array([[[0.3, 0.1, 0.7]]])
    if name == "n2_hand_case":
        tab = et.fs(scale=2.0 / 3.7)  # rc = 2
        pos = np.array([[[0.0, 0.0, 0.0], [1.2, 0.0, 0.0]]]) + np.array([0.0, 0.4, -3.3]).reshape(3, 1, 1) * [1, 0, 0]
        return tab, 3.0, pos
    if name == "n54_fe":
        tab = et.fs(scale=fe_scale, rho_max=900.0)
        return tab, 3 * A_FE, et.bcc(3, A_FE, jitter=0.08, seed=54, batch=5)
    if name == "n16_rho_beyond_table":
        tab = et.fs(rho_max=3.0)
        return tab, tab["rc"] / 0.61, lattice(16, 4, tab["rc"] / 0.61, 160)
    if name == "n16_nr10000":
        tab = et.fs(nr=10000, nrho=10000, rho_max=200.0)
        return tab, tab["rc"] / 0.61, lattice(16, 6, tab["rc"] / 0.61, 161)
    if name == "n5_orthorhombic":
        tab = et.fs(rho_max=200.0)
        L = tab["rc"] / 0.625
        box = (L, 1.3 * L, 0.8 * L)  # n_a = (1, 0, 1)
        rng = np.random.default_rng(5)
        return tab, box, (rng.random((6, 5, 3)) + np.arange(5)[:, None] * 0.37) % 1.0 * np.asarray(box)
    if name == "n2_orthorhombic_two_shifts":
        tab = et.fs(rho_max=400.0)
        L = tab["rc"] / (2.0 / 1.5)
        box = (L, 1.3 * L, 0.8 * L)  # n_a = (1, 1, 2)
        rng = np.random.default_rng(6)
        pos = rng.random((5, 2, 3)) * np.asarray(box)
        pos[:, 1] = pos[:, 0] + 0.5 * np.asarray(box) + 0.1 * (pos[:, 1] - 0.5)
        return tab, box, pos
    n, B = {"n3_idle_lane": (3, 5), "n16_ragged": (16, 7), "n64_full_wave": (64, 4), "n65_two_per_lane": (65, 3)}[name]
    tab = et.fs(rho_max=400.0)
    L = tab["rc"] / 0.61
    return tab, L, lattice(n, B, L, 1000 + n)


_REF = {}


def reference(name):
    """The case with its CPU results, computed once: U and dU/dx weighted by w,
    by the fp32 and by the fp64 torch path."""
    if name not in _REF:
        tab, box, pos = case(name)
        B = pos.shape[0]
        w = torch.linspace(0.5, 1.7, B, dtype=torch.float64) * torch.tensor([1.0, -1.0])[torch.arange(B) % 2]
        cpu = systems.EAM(tab, box)
        res = {}
        for dt in (torch.float32, torch.float64):
            x = torch.as_tensor(pos, dtype=dt).clone().requires_grad_()
            u = cpu.potential(x)
            g, = torch.autograd.grad((u * w.to(dt)).sum(), x)
            res[dt] = (u.detach(), g)
        _REF[name] = (tab, box, pos, w, res)
    return _REF[name]


SHAPES = ["n1_self_images", "n2_hand_case", "n3_idle_lane", "n16_ragged", "n54_fe", "n64_full_wave",
          "n65_two_per_lane", "n5_orthorhombic", "n2_orthorhombic_two_shifts", "n16_nr10000",
          "n16_rho_beyond_table"]


@pytest.mark.parametrize("name", SHAPES)
def test_energy(name, hip_device):
    tab, box, pos, _, res = reference(name)
    eam = systems.EAM(tab, box, device=DEV)
    x = torch.as_tensor(pos, dtype=torch.float32, device=DEV)
    assert eam._kernel_ok(x)
    u = eam.potential(x)
    assert u.shape == (pos.shape[0],) and u.dtype == torch.float32 and u.is_cuda
    close_or_on_par(u, res[torch.float32][0], res[torch.float64][0], name + " U")


@pytest.mark.parametrize("name", SHAPES)
def test_potential_bwd_with_weights(name, hip_device):
    """The backward kernel with weights g that are not all ones (both signs),
    through autograd."""
    tab, box, pos, w, res = reference(name)
    eam = systems.EAM(tab, box, device=DEV)
    x = torch.as_tensor(pos, dtype=torch.float32, device=DEV).requires_grad_()
    u = eam.potential(x)
    g, = torch.autograd.grad((u * w.float().to(DEV)).sum(), x)
    assert g.shape == x.shape
    close_or_on_par(g, res[torch.float32][1], res[torch.float64][1], name + " dU/dx")


def test_hand_case_closed_form(hip_device):
    """Hand case (a) on the device: both images of the one neighbour count, and
    the row does not depend on where along x the pair sits."""
    tab, box, pos, _, res = reference("n2_hand_case")
    eam = systems.EAM(tab, box, device=DEV)
    F = lambda rho: -1.9 * np.sqrt(rho)  # noqa: E731
    d, c = tab["rc"], 3.4 * 2.0 / 3.7
    f = lambda r: (r - d) ** 2 - 0.9 * (r - d) ** 3 / d  # noqa: E731
    phi = lambda r: (r - c) ** 2 * (1.2 - 0.6 * r + 0.09 * r * r) if r < c else 0.0  # noqa: E731
    U = 2 * F(f(1.2) + f(1.8)) + phi(1.2) + phi(1.8)
    u = eam.potential(torch.as_tensor(pos, dtype=torch.float32, device=DEV)).cpu().double()
    # fp32 arithmetic and a 2,000-point table of smooth functions: 1e-5 relative is ample
    assert float((u - U).abs().max()) <= 1e-5 * abs(U), (u, U)


def test_self_images_have_no_force(hip_device):
    tab, box, pos, _, _ = reference("n1_self_images")
    eam = systems.EAM(tab, box, device=DEV)
    f = eam.force(torch.as_tensor(pos, dtype=torch.float32, device=DEV))
    assert torch.equal(f, torch.zeros_like(f))


def test_row_strided_input(hip_device):
    tab, box, pos, w, res = reference("n16_ragged")
    eam = systems.EAM(tab, box, device=DEV)
    B = pos.shape[0]
    wide = torch.full((B, 48 + 5), float("nan"), device=DEV)
    wide[:, :48] = torch.as_tensor(pos, dtype=torch.float32).reshape(B, 48)
    x = wide[:, :48].unflatten(1, (16, 3))
    assert not x.is_contiguous()
    dense = x.contiguous()
    assert torch.equal(eam.potential(x), eam.potential(dense))
    assert torch.equal(eam.force(x), eam.force(dense))
    gx = torch.full((B, 48 + 3), 7.0, device=DEV)
    K_.eam_potential_bwd(wide[:, :48], torch.ones(B, device=DEV), gx[:, :48], n=16, **eam._kw(x.device))
    assert torch.equal(gx[:, :48], -eam.force(dense).reshape(B, 48))
    assert torch.equal(gx[:, 48:], torch.full((B, 3), 7.0, device=DEV))


def test_autograd_equals_minus_force(hip_device):
    tab, box, pos, _, _ = reference("n54_fe")
    eam = systems.EAM(tab, box, device=DEV)
    x = torch.as_tensor(pos, dtype=torch.float32, device=DEV).requires_grad_()
    u = eam.potential(x)
    g, = torch.autograd.grad(u, x, torch.ones_like(u))
    assert torch.equal(g, -eam.force(x.detach()))
    assert torch.equal(eam.get_force(x.detach()), eam.force(x.detach()))


def test_rows_are_independent_past_the_grid_cap(hip_device):
    """n = 16: 16 rows per block and at most 65,536 blocks (grid_for_rows), so
    65,536 * 16 + 5 rows make the grid loop take a second pass over a ragged
    block.  64 sampled rows, the last five among them, equal the same rows run
    alone, bit for bit, forward and backward."""
    tab = et.fs(rho_max=400.0)
    L = tab["rc"] / 0.61
    eam = systems.EAM(tab, L, device=DEV)
    B = 65536 * (4 * (64 // 16)) + 5
    base = torch.as_tensor(et.bcc(2, L / 2), dtype=torch.float32, device=DEV)
    gen = torch.Generator(device=DEV).manual_seed(12)
    x = base + 0.05 * L * torch.randn(B, 16, 3, device=DEV, generator=gen)
    u = eam.potential(x)
    f = eam.force(x)
    idx = torch.cat((torch.randint(B, (59,), device=DEV, generator=gen), torch.arange(B - 5, B, device=DEV)))
    rows = x[idx].contiguous()
    assert torch.equal(u[idx], eam.potential(rows))
    assert torch.equal(f[idx], eam.force(rows))
    assert bool(torch.isfinite(u).all())


def test_two_runs_are_bitwise_equal(hip_device):
    tab, box, pos, _, _ = reference("n54_fe")
    eam = systems.EAM(tab, box, device=DEV)
    x = torch.as_tensor(np.tile(pos, (40, 1, 1)), dtype=torch.float32, device=DEV)
    x = x + 0.01 * torch.randn(x.shape, device=DEV, generator=torch.Generator(device=DEV).manual_seed(2))
    assert torch.equal(eam.potential(x), eam.potential(x))
    assert torch.equal(eam.force(x), eam.force(x))


def test_unsupported_inputs_take_the_torch_path_or_raise(hip_device):
    tab, box, pos, _, res = reference("n16_ragged")
    eam = systems.EAM(tab, box, device=DEV)
    assert K_.eam_supported(256) and not K_.eam_supported(257) and not K_.eam_supported(0)
    x64 = torch.as_tensor(pos, device=DEV)
    assert not eam._kernel_ok(x64)
    torch.testing.assert_close(eam.potential(x64).cpu(), res[torch.float64][0], rtol=1e-12, atol=1e-12)
    out = torch.empty(2, device=DEV)
    with pytest.raises(ValueError, match="bad tables, box or cutoff"):
        K_.eam_potential(torch.zeros(2, 48, device=DEV), out, n=16, **dict(eam._kw(out.device), rc=-1.0))
    with pytest.raises(ValueError, match="shape not supported"):
        K_.eam_potential(torch.zeros(2, 257 * 3, device=DEV), out, n=257, **eam._kw(out.device))


@pytest.mark.parametrize("relaxation", [False, True])
def test_fe_config_to_free_energy_difference(tmp_path, relaxation, hip_device):
    """read_input of an Fe-style config -> build_model / build_potential ->
    fe_diff: finite 0-d tensors on the device."""
    cfg, _, _ = et.fe_config(tmp_path, device=DEV)
    torch.manual_seed(7)
    model = app.build_model(cfg)
    pot = app.build_potential(cfg, mode="testing")
    assert isinstance(pot, systems.EAM) and pot.traj.is_cuda
    kw = dict(relaxation=True, relaxation_kw=dict(path_len=2)) if relaxation else {}
    out = app.fe_diff(cfg, model, pot, 64, batchsize=32, return_err=True, nboot=20, **kw)
    assert len(out) == 6
    for v in out:
        assert v.dim() == 0 and v.is_cuda and bool(torch.isfinite(v)), out
