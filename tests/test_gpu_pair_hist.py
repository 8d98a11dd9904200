"""GPU: nfk_pair_hist (the weighted pair-distance histogram) and what stands on
it, observables.pair_histogram / rdf and app.structure.

The kernel's distances are fp32 and the reference here is the definition in
fp64 NumPy on the same fp32 inputs, so the comparison holds under a condition on
the INPUTS, asserted on the CPU before anything runs: no pair's fp64 distance
lies within 32 * 2^-24 * max(L) of a bin edge, r_max included (without a box,
max |x| of the row stands for L).  That is the absolute error a handful of fp32
roundings at magnitude L can put on r: the wrap d - L * k rounds at ulp(L), not
at ulp(r).  ``conditioned`` redraws every row that holds an offending pair until
none is left.  Under the condition the counts are exactly equal; it is no
tolerance.  r_max is chosen per case from the expected number of offending pairs
per row (pairs * shell measure within the margin of an edge / box measure), so
that the redraws converge; nothing is chosen from what the kernel returns.
"""
import itertools
import math

import numpy as np
import pytest
import torch

import nf.flows as nff
import nf.models as nfm
from normalizingflow_amd import _lib, app, systems
from normalizingflow_amd import kernels as K_
from normalizingflow_amd import observables as O
from normalizingflow_amd import reweight as R

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
MARGIN = 32 * 2.0 ** -24
BOXES = {"cubic": (4.0, 4.0, 4.0), "ortho": (4.0, 5.5, 3.25), "none": None}


@pytest.fixture(autouse=True)
def kernel_path_only(monkeypatch):
    """A device fp32 call that reaches the torch restatement fails the test."""
    real = O._hist_torch

    def guard(flat, *a, **k):
        assert not (flat.is_cuda and flat.dtype == torch.float32 and O.use_kernels), "the torch path ran"
        return real(flat, *a, **k)
    monkeypatch.setattr(O, "_hist_torch", guard)


def np_rows(x32, box, r_max, nbins):
    """Per-row integer counts [B, nbins] by the definition in fp64, and per row the
    least distance of a pair's r to a bin edge divided by the row's scale (max L, or
    max |x| without a box)."""
    x = np.asarray(x32, dtype=np.float64)
    B, n, dim = x.shape
    counts = np.zeros((B, nbins), dtype=np.int64)
    slack = np.full(B, np.inf)
    if n < 2:
        return counts, slack
    i, j = np.triu_indices(n, 1)
    L = None if box is None else np.asarray(box[:dim], dtype=np.float64)
    step = max(1, (1 << 21) // len(i))
    for s in range(0, B, step):
        xs = x[s:s + step]
        d = xs[:, i] - xs[:, j]
        if L is not None:
            d = d - L * np.rint(d / L)
        r = np.sqrt((d * d).sum(-1))
        t = r * nbins / r_max
        edge = np.minimum(np.rint(t), nbins) * (r_max / nbins)
        scale = np.abs(xs).max(axis=(1, 2)) if L is None else np.full(len(xs), L.max())
        with np.errstate(invalid="ignore"):
            slack[s:s + step] = np.nanmin(np.abs(r - edge), axis=1) / scale
            ok = r < r_max
        k = np.where(ok, np.floor(np.where(ok, t, 0.0)), 0).astype(np.int64)
        ok &= k < nbins
        rows = np.broadcast_to(np.arange(len(xs))[:, None], k.shape)
        counts[s:s + step] = np.bincount((rows * nbins + k)[ok], minlength=len(xs) * nbins).reshape(-1, nbins)
    return counts, slack


def draw(B, n, dim, box, shifts, gen):
    if box is None:
        return (4.0 * torch.rand(B, n, dim, generator=gen) - 2.0).float()
    L = torch.tensor(box[:dim])
    x = torch.rand(B, n, dim, generator=gen) * L
    if shifts:
        x = x + L * torch.randint(-shifts, shifts + 1, (B, n, dim), generator=gen).float()
    return x.float()


def pick_r_max(n, dim, nbins, box):
    """The largest r_max (from half the shortest box length down, or 2 without a box)
    at which a row expects at most half an offending pair."""
    L = (4.0,) * dim if box is None else box[:dim]
    scale = 2.0 if box is None else max(L)
    r_max = 0.5 * min(L)
    pairs = n * (n - 1) / 2
    while True:
        edges = np.arange(1, nbins + 1) * (r_max / nbins)
        shell = (4 * math.pi * edges ** 2 if dim == 3 else 2 * math.pi * edges).sum() * 2 * MARGIN * scale
        if pairs * shell / math.prod(L) <= 0.5:
            return r_max
        r_max *= 0.8


def conditioned(B, n, dim, box_kind, nbins, shifts=0, seed=0, r_max=None):
    """fp32 rows [B, n, dim] that meet the condition, r_max, and their per-row fp64 counts."""
    box = BOXES[box_kind]
    r_max = pick_r_max(n, dim, nbins, box) if r_max is None else r_max
    gen = torch.Generator().manual_seed(seed)
    x = draw(B, n, dim, box, shifts, gen)
    counts, slack = np_rows(x.numpy(), box, r_max, nbins)
    for _ in range(200):
        bad = np.nonzero(slack < MARGIN)[0]
        if len(bad) == 0:
            break
        x[bad] = draw(len(bad), n, dim, box, shifts, gen)
        counts[bad], slack[bad] = np_rows(x[bad].numpy(), box, r_max, nbins)
    assert (slack >= MARGIN).all(), "the redraws did not converge"
    return x, (None if box is None else box[:dim]), r_max, counts


def device_hist(x, box, r_max, nbins, weights=None):
    hist, edges = O.pair_histogram(x.to(DEV), box, r_max, nbins,
                                   weights=None if weights is None else weights.to(DEV))
    assert hist.is_cuda and hist.dtype == torch.float64 and hist.shape == (nbins,)
    assert float(edges[0]) == 0.0 and float(edges[-1]) == r_max
    return hist.cpu().numpy()


NS = [1, 2, 3, 31, 32, 33, 64, 65, 256]
NBINS = [1, 7, 64, 65, 1024]
BATCHES = [1, 2, 5, 37]
GRID = [(n, dim, NBINS[(q + q // 5) % 5], BATCHES[q % 4], ["cubic", "ortho", "none"][q % 3], 3 * (q % 2))
        for q, (n, dim) in enumerate(itertools.product(NS, (2, 3)))]
# every value of a set with every kind of box at n = 32, and the largest of everything at once
GRID += [(32, 3, nb, b, kind, 3) for (nb, b), kind in zip(itertools.product(NBINS, BATCHES),
                                                         itertools.cycle(["cubic", "none", "ortho"]))]
GRID += [(256, 3, 1024, 5, "ortho", 3), (256, 2, 1024, 2, "none", 0), (256, 3, 64, 2, "cubic", 3),
         (256, 3, 65, 5, "ortho", 0)]


@pytest.mark.parametrize("n,dim,nbins,batch,box_kind,shifts", GRID)
def test_unweighted_counts_are_exact(hip_device, n, dim, nbins, batch, box_kind, shifts):
    x, box, r_max, counts = conditioned(batch, n, dim, box_kind, nbins, shifts, seed=n * 1000 + nbins + batch)
    want = counts.sum(0)
    got = device_hist(x, box, r_max, nbins)
    print("n %d dim %d nbins %d batch %d %s r_max %.4f: %d pairs counted" % (n, dim, nbins, batch, box_kind, r_max,
                                                                            want.sum()))
    assert np.array_equal(got, want.astype(np.float64))
    if n >= 31 and nbins <= 65:  # (a fine grid on many particles leaves room for a small r_max only)
        assert want.sum() > 10 * batch


def test_batches_around_the_partition_points(hip_device):
    huge = K_.pair_hist_parts(1 << 40)
    assert K_.pair_hist_parts(0) == 0 and K_.pair_hist_parts(1) == 1 and huge >= 1
    lo, hi = 1, 1 << 40  # the least batch that saturates the partials
    while lo < hi:
        mid = (lo + hi) // 2
        lo, hi = (lo, mid) if K_.pair_hist_parts(mid) == huge else (mid + 1, hi)
    saturation = lo
    per_group = 1  # the rows one workgroup takes before a second one starts
    while K_.pair_hist_parts(per_group + 1) == 1:
        per_group += 1
    assert saturation == (huge - 1) * per_group + 1 and saturation <= 1 << 16
    assert K_.pair_hist_workspace_elems(saturation + 5, 7) == 7 * huge
    sizes = sorted({b for c in (per_group, saturation, huge * per_group, 2 * huge * per_group)
                    for b in (c - 1, c, c + 1) if b >= 1})
    x, box, r_max, counts = conditioned(max(sizes), 3, 3, "ortho", 7, shifts=3, seed=41)
    cum = np.concatenate((np.zeros((1, 7), dtype=np.int64), np.cumsum(counts, 0)))
    for b in sizes:
        assert np.array_equal(device_hist(x[:b], box, r_max, 7), cum[b].astype(np.float64)), b


def test_strided_rows(hip_device):
    n, dim, nbins = 9, 3, 16
    x, box, r_max, counts = conditioned(11, n, dim, "cubic", nbins, shifts=3, seed=5)
    wide = torch.full((11, n * dim + 7), float("nan"), device=DEV)
    wide[:, 3:3 + n * dim] = x.reshape(11, -1).to(DEV)
    rows = wide[:, 3:3 + n * dim]
    assert rows.stride(0) == n * dim + 7
    hist, _ = O.pair_histogram(rows.reshape(11, n, dim), box, r_max, nbins)
    assert np.array_equal(hist.cpu().numpy(), counts.sum(0).astype(np.float64))
    # the binding itself on the slice
    out = torch.empty(nbins, dtype=torch.float64, device=DEV)
    ws = torch.empty(K_.pair_hist_workspace_elems(11, nbins), dtype=torch.float64, device=DEV)
    K_.pair_hist(rows, out, ws, n=n, dim=dim, box=box, r_max=r_max)
    assert torch.equal(out, hist)


def test_weighted(hip_device):
    n, dim, nbins, B = 33, 3, 65, 300
    x, box, r_max, counts = conditioned(B, n, dim, "ortho", nbins, shifts=2, seed=6)
    w = torch.rand(B, generator=torch.Generator().manual_seed(7), dtype=torch.float64) + 0.05
    w[::5] = 0.0
    got = device_hist(x, box, r_max, nbins, w)
    want = (w.numpy()[:, None] * counts).sum(0)
    # B * 2^-53 for B <= 1,024 rows of non-negative terms, rounded up
    np.testing.assert_allclose(got, want, rtol=1e-12, atol=0)
    unit = device_hist(x, box, r_max, nbins)
    assert np.array_equal(device_hist(x, box, r_max, nbins, torch.full((B,), 2.0, dtype=torch.float64)), 2.0 * unit)
    assert np.array_equal(device_hist(x, box, r_max, nbins, torch.ones(B)), unit)  # fp32 weights are promoted


def test_reproducible_and_capturable(hip_device):
    n, dim, nbins, B = 32, 3, 100, 5000
    gen = torch.Generator().manual_seed(8)
    x = draw(B, n, dim, BOXES["cubic"], 1, gen).to(DEV)
    w = (torch.rand(B, generator=gen, dtype=torch.float64) + 0.1).to(DEV)
    first, _ = O.pair_histogram(x, 4.0, 2.0, nbins, weights=w)
    second, _ = O.pair_histogram(x, 4.0, 2.0, nbins, weights=w)
    assert torch.equal(first, second) and float(first.sum()) > 0
    # one capture on one stream, replayed: the eager bits
    rows = x.reshape(B, -1)
    hist = torch.zeros(nbins, dtype=torch.float64, device=DEV)
    ws = torch.empty(K_.pair_hist_workspace_elems(B, nbins), dtype=torch.float64, device=DEV)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        K_.pair_hist(rows, hist, ws, n=n, dim=dim, box=(4.0, 4.0, 4.0), r_max=2.0, weights=w)
    for _ in range(2):
        hist.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(hist, first)


def test_nan_row_lands_in_no_bin(hip_device):
    n, dim, nbins = 31, 3, 7
    x, box, r_max, counts = conditioned(9, n, dim, "cubic", nbins, seed=9)
    clean = device_hist(x, box, r_max, nbins)
    bad = x.clone()
    bad[4, :, 1] = float("nan")  # every pair of row 4 has a NaN distance
    got = device_hist(bad, box, r_max, nbins)
    assert np.array_equal(got, (counts.sum(0) - counts[4]).astype(np.float64)) and counts[4].sum() > 0
    assert np.array_equal(clean, counts.sum(0).astype(np.float64))
    bad[4, :, 1] = float("inf")
    assert np.array_equal(device_hist(bad, box, r_max, nbins), got)


def test_host_validation(hip_device):
    lib = _lib.load()
    n, dim, nbins, B = 4, 3, 8, 6
    x = torch.rand(B, n * dim, device=DEV)
    hist = torch.full((nbins,), -7.0, dtype=torch.float64, device=DEV)
    ws = torch.zeros(K_.pair_hist_workspace_elems(B, nbins), dtype=torch.float64, device=DEV)
    stream = torch.cuda.current_stream().cuda_stream

    def call(x=x.data_ptr(), ldx=n * dim, w=None, batch=B, n=n, dim=dim, box=(4.0, 4.0, 4.0), r_max=2.0, nbins=nbins,
             hist=hist.data_ptr(), ws=ws.data_ptr()):
        rc = lib.nfk_pair_hist(x, ldx, w, batch, n, dim, *box, r_max, nbins, hist, ws, stream)
        return rc, lib.nfk_last_error().decode()

    refused = [
        (dict(n=0), "shape not supported"), (dict(n=257), "shape not supported"),
        (dict(dim=1), "shape not supported"), (dict(dim=4), "shape not supported"),
        (dict(nbins=0), "shape not supported"), (dict(nbins=1025), "shape not supported"),
        (dict(batch=-1), "bad batch"),
        (dict(x=None), "null x or workspace"), (dict(ws=None), "null x or workspace"), (dict(hist=None), "null hist"),
        (dict(r_max=0.0), "r_max must be"), (dict(r_max=-1.0), "r_max must be"),
        (dict(r_max=float("nan")), "r_max must be"),
        (dict(r_max=2.0 + 1e-9), "half the shortest box"), (dict(box=(4.0, 3.9, 4.0)), "half the shortest box"),
        (dict(box=(4.0, 4.0, 3.9)), "half the shortest box"),
        (dict(box=(4.0, 0.0, 4.0)), "all positive or all zero"), (dict(box=(-4.0, 4.0, 4.0)), "bad box length"),
        (dict(ldx=n * dim - 1), "ldx below the row width"),
    ]
    for kw, message in refused:
        rc, err = call(**kw)
        assert rc == _lib.NFK_EINVAL and message in err, (kw, rc, err)
    torch.cuda.synchronize()
    assert bool((hist == -7.0).all()) and bool((ws == 0.0).all())  # nothing was launched
    assert not K_.pair_hist_supported(257, 3, 8) and K_.pair_hist_supported(256, 2, 1024)
    with pytest.raises(ValueError, match="half the shortest box"):
        K_.pair_hist(x, hist, ws, n=n, dim=dim, box=(4.0, 4.0, 4.0), r_max=2.5)
    # legal edges: dim 2 ignores lz, one row ignores ldx, batch 0 writes zeros
    assert call(dim=2, ldx=8, n=4, box=(4.0, 4.0, 0.0))[0] == 0
    assert call(batch=1, ldx=0)[0] == 0
    assert call(batch=0, x=None, ws=None)[0] == 0
    torch.cuda.synchronize()
    assert bool((hist == 0.0).all())
    empty, _ = O.pair_histogram(x[:0].reshape(0, n, dim), 4.0, 2.0, nbins)
    assert empty.is_cuda and bool((empty == 0.0).all())


def test_rdf_on_the_device_against_the_cpu(hip_device):
    n, dim, nbins, B = 32, 3, 64, 200
    for box_kind in ("cubic", "ortho"):
        x, box, r_max, counts = conditioned(B, n, dim, box_kind, nbins, shifts=1, seed=10)
        lw = torch.randn(B, generator=torch.Generator().manual_seed(11))
        for kw in ({}, {"log_weights": lw}):
            hist_c, _ = O.pair_histogram(x, box, r_max, nbins)
            hist_d, _ = O.pair_histogram(x.to(DEV), box, r_max, nbins)
            assert torch.equal(hist_d.cpu(), hist_c) and np.array_equal(hist_c.numpy(), counts.sum(0))
            r_c, g_c = O.rdf(x, box, r_max=r_max, nbins=nbins, **kw)
            r_d, g_d = O.rdf(x.to(DEV), box, r_max=r_max, nbins=nbins,
                             **{k: v.to(DEV) for k, v in kw.items()})
            assert g_d.is_cuda and torch.equal(r_d.cpu(), r_c)
            torch.testing.assert_close(g_d.cpu(), g_c, rtol=1e-12, atol=0)
    # 2-D, r_max from the box
    x, box, r_max, _ = conditioned(50, 16, 2, "ortho", 20, seed=12, r_max=2.0)
    r_c, g_c = O.rdf(x, box, nbins=20)
    r_d, g_d = O.rdf(x.to(DEV), box, nbins=20)
    assert torch.equal(r_d.cpu(), r_c)
    torch.testing.assert_close(g_d.cpu(), g_c, rtol=1e-12, atol=0)


def test_use_kernels_switch_takes_the_torch_path(hip_device, monkeypatch):
    x, box, r_max, counts = conditioned(7, 9, 3, "cubic", 16, seed=13)
    monkeypatch.setattr(O, "use_kernels", False)
    hist, _ = O.pair_histogram(x.to(DEV), box, r_max, 16)
    assert hist.is_cuda and np.array_equal(hist.cpu().numpy(), counts.sum(0).astype(np.float64))


def lj_and_model():
    """Eight LJ particles on a 2 x 2 x 2 lattice of spacing 1.2 and a 2-layer NSF_AR
    flow over an Einstein crystal on the same sites."""
    L = 2.4
    sites = torch.tensor(list(itertools.product((0.6, 1.8), repeat=3)))
    torch.manual_seed(1234)
    traj = sites + 0.05 * torch.randn(200, 8, 3)
    target = systems.LJ(pos_dir=traj, boxlength=L, device=DEV, cutoff=1.2)
    prior = systems.EinsteinCrystal(sites, 3, boxlength=L, alpha=400, device=DEV)
    model = nfm.NormalizingFlowModel(prior, [nff.NSF_AR(dim=24, K=8, B=3, hidden_dim=16) for _ in range(2)]).to(DEV)
    cfg = app.get_cfg_defaults()
    cfg.device, cfg.dataset.kT, cfg.dataset.dim, cfg.dataset.nparticles = DEV, 1.0, 3, 8
    return cfg, target, model, L


def test_app_structure_on_the_device(hip_device):
    cfg, target, model, L = lj_and_model()
    torch.manual_seed(21)
    out = app.structure(cfg, model, target, 64, batchsize=32, nbins=24)
    assert sorted(out) == ["ess", "g_flow", "g_reweighted", "g_target", "r"]
    for k in ("r", "g_flow", "g_reweighted", "g_target"):
        assert out[k].is_cuda and out[k].shape == (24,) and out[k].dtype == torch.float64
        assert bool(torch.isfinite(out[k]).all())
    assert float(out["r"][-1] + out["r"][0]) == pytest.approx(0.5 * L)
    assert out["ess"].dim() == 0 and 0.999 < float(out["ess"]) <= 64.0
    # the same draws by hand
    torch.manual_seed(21)
    with torch.no_grad():
        x, lq = app.generate_from_nf(model, 64, batchsize=32)
    rows = target.sample(64).reshape(64, 8, 3)
    e = target.potential(x.reshape(-1, 8, 3)).detach() / cfg.dataset.kT
    lw = R.log_weights(lq, e)
    assert torch.equal(out["g_target"], O.rdf(rows, L, nbins=24)[1]) and float(out["g_target"].sum()) > 0
    assert torch.equal(out["g_flow"], O.rdf(x.reshape(-1, 8, 3), L, nbins=24)[1])
    assert torch.equal(out["g_reweighted"], O.rdf(x.reshape(-1, 8, 3), L, nbins=24, log_weights=lw)[1])
    assert torch.equal(out["ess"], R.ess(lw))
