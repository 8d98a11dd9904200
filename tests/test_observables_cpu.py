"""CPU: observables.py's torch restatement (pair_histogram, rdf, coordination)
against a plain NumPy fp64 double loop, and app.structure with a stub model."""
import math

import numpy as np
import pytest
import torch

from normalizingflow_amd import app, systems
from normalizingflow_amd import observables as O
from normalizingflow_amd import reweight as R


def numpy_hist(x, box, r_max, nbins, w=None):
    """The definition, pair by pair in fp64: (hist, pairs at or beyond r_max)."""
    x = np.asarray(x, dtype=np.float64)
    B, n, dim = x.shape
    L = None if box is None else np.broadcast_to(np.asarray(box, dtype=np.float64), (dim,))
    hist = np.zeros(nbins)
    beyond = 0
    scale = nbins / r_max
    for b in range(B):
        count = np.zeros(nbins, dtype=np.int64)
        for i in range(n):
            for j in range(i + 1, n):
                d = x[b, i] - x[b, j]
                if L is not None:
                    d = d - L * np.rint(d * (1.0 / L))
                r2 = d[0] * d[0] + d[1] * d[1]
                if dim == 3:
                    r2 = r2 + d[2] * d[2]
                r = math.sqrt(r2)
                k = int(math.floor(r * scale))
                if r < r_max and k < nbins:
                    count[k] += 1
                else:
                    beyond += 1
        hist += (1.0 if w is None else float(w[b])) * count
    return hist, beyond


def positions(B, n, dim, box, shifts, seed):
    """fp64 rows uniform in the box (or in [-2, 2] without one), every particle moved
    by up to +-``shifts`` whole box lengths."""
    g = torch.Generator().manual_seed(seed)
    if box is None:
        return 4.0 * torch.rand(B, n, dim, generator=g, dtype=torch.float64) - 2.0
    L = torch.tensor(box, dtype=torch.float64).expand(dim)
    x = torch.rand(B, n, dim, generator=g, dtype=torch.float64) * L
    if shifts:
        x = x + L * torch.randint(-shifts, shifts + 1, (B, n, dim), generator=g).double()
    return x


BOXES = {"cubic": lambda dim: 4.0, "ortho": lambda dim: (4.0, 5.5, 3.25)[:dim], "none": lambda dim: None}


@pytest.mark.parametrize("box_kind", ["cubic", "ortho", "none"])
@pytest.mark.parametrize("dim", [2, 3])
@pytest.mark.parametrize("n", [1, 2, 3, 9])
def test_exact_counts_and_pair_accounting(n, dim, box_kind):
    box = BOXES[box_kind](dim)
    B, nbins, r_max = 23, 13, 1.55
    for shifts in (0, 3):
        x = positions(B, n, dim, box, shifts, seed=100 * n + 10 * dim + shifts)
        hist, edges = O.pair_histogram(x, box, r_max, nbins)
        want, beyond = numpy_hist(x.numpy(), box, r_max, nbins)
        assert hist.dtype == torch.float64 and hist.shape == (nbins,) and edges.shape == (nbins + 1,)
        assert float(edges[0]) == 0.0 and float(edges[-1]) == r_max
        assert np.array_equal(hist.numpy(), want), (hist, want)
        assert float(hist.sum()) + beyond == B * n * (n - 1) // 2
        if n > 2:
            assert hist.sum() > 0 and beyond > 0


def test_batch_shape_chunks_and_fp32(monkeypatch):
    x = positions(12, 5, 3, 4.0, 2, seed=5)
    want, _ = O.pair_histogram(x, 4.0, 2.0, 16)
    got, _ = O.pair_histogram(x.reshape(3, 4, 5, 3), 4.0, 2.0, 16)
    assert torch.equal(got, want)
    monkeypatch.setattr(O, "_CHUNK_ELEMS", 25)  # two rows per chunk
    got, _ = O.pair_histogram(x, (4.0, 4.0, 4.0), 2.0, 16)
    assert torch.equal(got, want)
    h32, _ = O.pair_histogram(x.float(), 4.0, 2.0, 16)
    # fp32 distances: a pair within an ulp of an edge may move to the next bin, no more
    assert h32.dtype == torch.float64 and float((h32 - want).abs().sum()) <= 4


def test_weighted_histogram():
    B, n, nbins, r_max, box = 1024, 4, 9, 1.6, (4.0, 5.5, 3.25)
    x = positions(B, n, 3, box, 1, seed=7)
    w = torch.rand(B, generator=torch.Generator().manual_seed(8), dtype=torch.float64) + 0.1
    w[::7] = 0.0
    hist, _ = O.pair_histogram(x, box, r_max, nbins, weights=w)
    want, _ = numpy_hist(x.numpy(), box, r_max, nbins, w.numpy())
    # B * 2^-53 with B <= 1,024 rows of positive terms, rounded up
    np.testing.assert_allclose(hist.numpy(), want, rtol=1e-12, atol=0)
    twice, _ = O.pair_histogram(x, box, r_max, nbins, weights=torch.full((B,), 2.0))
    unit, _ = O.pair_histogram(x, box, r_max, nbins)
    assert torch.equal(twice, 2.0 * unit)


def test_nan_row_lands_in_no_bin():
    x = positions(6, 5, 3, 4.0, 0, seed=9)
    want, _ = O.pair_histogram(x[[0, 1, 3, 4, 5]], 4.0, 2.0, 8)
    x[2, 1, 0] = float("nan")
    hist, _ = O.pair_histogram(x, 4.0, 2.0, 8)
    # the row's pairs that avoid particle 1 still count
    keep = O.pair_histogram(x[2:3, [0, 2, 3, 4]], 4.0, 2.0, 8)[0]
    assert torch.equal(hist, want + keep) and float(want.sum()) > 0


def ideal_gas(B=4096, n=32, L=4.0, seed=11):
    return torch.rand(B, n, 3, generator=torch.Generator().manual_seed(seed), dtype=torch.float64) * L


def test_ideal_gas_rdf_is_one():
    # 50 bins: the innermost bin expects 8.5 pairs, the least at which 5 Poisson standard
    # errors are a two-sided bound (at 100 bins it expects 1, where g = 0 is 1 sigma away)
    B, n, L, nbins = 4096, 32, 4.0, 50
    x = ideal_gas(B, n, L)
    r, g = O.rdf(x, L, nbins=nbins)
    assert r.shape == g.shape == (nbins,) and g.dtype == torch.float64
    dr = 0.5 * L / nbins
    torch.testing.assert_close(r, (torch.arange(nbins, dtype=torch.float64) + 0.5) * dr, rtol=1e-14, atol=0)
    edges = torch.arange(nbins + 1, dtype=torch.float64) * dr
    expected = B * n * (n - 1) / 2 * 4.0 / 3.0 * math.pi * (edges[1:] ** 3 - edges[:-1] ** 3) / L ** 3
    stderr = 1.0 / torch.sqrt(expected)  # Poisson counts: sigma(g) = sqrt(N) / N
    dev = (g - 1.0).abs() / stderr
    print("ideal gas: max |g - 1| / stderr = %.2f, smallest expected count %.1f" % (float(dev.max()),
                                                                                    float(expected.min())))
    assert bool((dev < 5.0).all()), dev


def test_rdf_2d_and_orthorhombic_normalisation():
    box = (4.0, 6.0)
    g0 = torch.Generator().manual_seed(12)
    x = torch.rand(2048, 16, 2, generator=g0, dtype=torch.float64) * torch.tensor(box, dtype=torch.float64)
    r, g = O.rdf(x, box, nbins=20)
    assert float(r[-1] + r[0]) == pytest.approx(2.0)  # r_max = min(L) / 2
    edges = torch.arange(21, dtype=torch.float64) * 0.1
    expected = 2048 * 16 * 15 / 2 * math.pi * (edges[1:] ** 2 - edges[:-1] ** 2) / 24.0
    assert bool(((g - 1.0).abs() * torch.sqrt(expected) < 5.0).all())


def test_log_weights_against_weights():
    x = ideal_gas(64, 8)
    lw = 3.0 * torch.randn(64, generator=torch.Generator().manual_seed(13))
    r1, g1 = O.rdf(x, 4.0, nbins=10, log_weights=lw)
    r2, g2 = O.rdf(x, 4.0, nbins=10, weights=torch.softmax(lw.double(), 0))
    assert torch.equal(r1, r2) and torch.equal(g1, g2)
    # a common factor of the weights cancels
    _, g3 = O.rdf(x, 4.0, nbins=10, weights=5.0 * torch.softmax(lw.double(), 0))
    torch.testing.assert_close(g3, g1, rtol=1e-13, atol=0)
    # the weighted g(r) is the weighted mean of the rows' own
    rows = torch.stack([O.rdf(x[b], 4.0, nbins=10)[1] for b in range(64)])
    torch.testing.assert_close(g1, R.reweighted_mean(rows, lw), rtol=1e-12, atol=1e-15)


def test_coordination_of_an_ideal_gas():
    n, L = 32, 4.0
    x = ideal_gas(2048, n, L)
    r, g = O.rdf(x, L, nbins=40)
    N = O.coordination(r, g, n, L)
    assert N.shape == (41,) and float(N[0]) == 0.0 and bool((N[1:] >= N[:-1]).all())
    sphere = (n - 1) * 4.0 / 3.0 * math.pi * 2.0 ** 3 / L ** 3
    # 2 / n times the pairs within r_max per row: Poisson, relative error 1 / sqrt(pairs)
    pairs = 2048 * n / 2 * sphere
    assert abs(float(N[-1]) - sphere) < 5.0 * sphere / math.sqrt(pairs)
    # with g == 1 exactly the shells telescope to the sphere
    N1 = O.coordination(r, torch.ones_like(g), n, (L, L, L))
    assert float(N1[-1]) == pytest.approx(sphere, rel=1e-13)
    # it is exactly the mean neighbour count: 2 / n * pairs within r_max per row
    hist, _ = O.pair_histogram(x, L, 2.0, 40)
    assert float(N[-1]) == pytest.approx(2.0 / n * float(hist.sum()) / 2048, rel=1e-12)


def test_error_paths():
    x = ideal_gas(4, 5)
    with pytest.raises(ValueError, match="half the shortest box"):
        O.pair_histogram(x, 4.0, 2.0 + 1e-9, 10)
    with pytest.raises(ValueError, match="half the shortest box"):
        O.rdf(x, (4.0, 3.0, 4.0), r_max=1.6)
    with pytest.raises(ValueError, match="not both"):
        O.rdf(x, 4.0, weights=torch.ones(4), log_weights=torch.zeros(4))
    with pytest.raises(ValueError, match="needs a box"):
        O.rdf(x, None, r_max=1.0)
    with pytest.raises(ValueError, match="r_max"):
        O.pair_histogram(x, None, 0.0, 10)
    with pytest.raises(ValueError, match="nbins"):
        O.pair_histogram(x, None, 1.0, 0)
    with pytest.raises(ValueError, match="one value per configuration"):
        O.pair_histogram(x, None, 1.0, 4, weights=torch.ones(3))
    with pytest.raises(ValueError, match="box must be"):
        O.pair_histogram(x, (4.0, 4.0), 1.0, 4)
    hist, _ = O.pair_histogram(x[:0], 4.0, 1.0, 4)
    assert torch.equal(hist, torch.zeros(4, dtype=torch.float64))


class _StubModel:
    """Samples near the lattice sites with a made-up log q."""

    def __init__(self, centers):
        self.c = centers.reshape(-1)

    def sample(self, n):
        x = self.c + 0.2 * torch.randn(n, self.c.numel())
        return x, -(x - self.c).square().sum(1), x


def test_app_structure_on_cpu():
    L = 3.0
    centers = torch.tensor([[0.5, 0.5, 0.5], [2.0, 2.0, 0.5], [2.0, 0.5, 2.0], [0.5, 2.0, 2.0]])
    target = systems.EinsteinCrystal(centers, 3, boxlength=None, alpha=30)
    cfg = app.get_cfg_defaults()
    cfg.device, cfg.dataset.kT, cfg.dataset.dim, cfg.dataset.nparticles = "cpu", 0.7, 3, 4
    cfg.dataset.boxlength = L  # the potential holds none: the config's is the fallback
    torch.manual_seed(3)
    out = app.structure(cfg, _StubModel(centers), target, 60, batchsize=20, nbins=12)
    assert sorted(out) == ["ess", "g_flow", "g_reweighted", "g_target", "r"]
    for k in ("r", "g_flow", "g_reweighted", "g_target"):
        assert out[k].shape == (12,) and out[k].dtype == torch.float64 and bool(torch.isfinite(out[k]).all())
    assert out["ess"].dim() == 0 and 1.0 <= float(out["ess"]) <= 60.0
    assert float(out["r"][-1] + out["r"][0]) == pytest.approx(0.5 * L)
    assert not torch.equal(out["g_flow"], out["g_reweighted"]) and float(out["g_target"].sum()) > 0
    # the same draws by hand
    torch.manual_seed(3)
    x, lq = app.generate_from_nf(_StubModel(centers), 60, batchsize=20)
    e = target.potential(x.reshape(-1, 4, 3)) / 0.7
    lw = R.log_weights(lq, e)
    assert torch.equal(out["g_reweighted"], O.rdf(x.reshape(-1, 4, 3), L, nbins=12, log_weights=lw)[1])
    assert torch.equal(out["ess"], R.ess(lw))
    # the potential's own box wins over the config's
    boxed = systems.EinsteinCrystal(centers, 3, boxlength=2.5, alpha=30)
    torch.manual_seed(3)
    out = app.structure(cfg, _StubModel(centers), boxed, 60, batchsize=20, nbins=12)
    assert float(out["r"][-1] + out["r"][0]) == pytest.approx(1.25)
    cfg.dataset.boxlength = None
    with pytest.raises(ValueError, match="needs a box"):
        app.structure(cfg, _StubModel(centers), target, 60, batchsize=20)
