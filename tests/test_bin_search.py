"""CPU: the K = 8 bin search of the fused kernels' knot phase
(normalizingflow_amd/csrc/nfk_bin_search.h), compiled for the host by the
package's host build and exported as _nfk_host.bin8: the three-compare
bisection gives the bin the counting form gives -- the number of interior
knots t[1 .. 7] that are <= x -- for every non-decreasing knot vector, ties,
infinite and NaN inputs and NaN knots included."""
import numpy as np
import pytest
import torch


@pytest.fixture(scope="module")
def hs():
    from normalizingflow_amd import _hostbuild
    _hostbuild.build()
    from normalizingflow_amd import _nfk_host
    return _nfk_host


def _count(t, x):
    """The definition, in numpy: #{j in 1..7: x >= t[j]} (NaN compares false)."""
    with np.errstate(invalid="ignore"):
        return (x[:, None] >= t[:, 1:]).sum(axis=1).astype(np.int32)


def _check(hs, t, x):
    t = np.ascontiguousarray(t, dtype=np.float32)
    x = np.ascontiguousarray(x, dtype=np.float32)
    tt, xt = torch.from_numpy(t), torch.from_numpy(x)
    want = _count(t, x)
    assert np.array_equal(hs.bin8(tt, xt, 0).numpy(), want)   # the counting form is the definition
    got = hs.bin8(tt, xt, 1).numpy()
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, (t[bad[:3]], x[bad[:3]], got[bad[:3]], want[bad[:3]])
    return want


def _knots(rng, n):
    """n non-decreasing 8-knot vectors with t[0] = 0, many of them with ties:
    cumulative sums of steps of which a random third is exactly zero."""
    steps = rng.random((n, 8), dtype=np.float32) * (rng.random((n, 8)) > 1 / 3)
    steps[:, 0] = 0
    return np.cumsum(steps, axis=1, dtype=np.float32)


def test_search_equals_count_random(hs):
    rng = np.random.default_rng(0)
    t = _knots(rng, 100_000)
    assert (np.diff(t, axis=1) >= 0).all() and (np.diff(t, axis=1) == 0).any()
    x = (rng.random(len(t), dtype=np.float32) * 1.2 - 0.1) * t[:, 7]
    bins = _check(hs, t, x)
    assert set(np.unique(bins)) == set(range(8))


def test_search_equals_count_at_every_knot_and_around(hs):
    rng = np.random.default_rng(1)
    t = _knots(rng, 20_000)
    for j in range(8):
        at = t[:, j].copy()
        _check(hs, t, at)
        _check(hs, t, np.nextafter(at, np.float32(-np.inf)))
        _check(hs, t, np.nextafter(at, np.float32(np.inf)))


def test_search_equals_count_nonfinite(hs):
    rng = np.random.default_rng(2)
    t = _knots(rng, 10_000)
    n = len(t)
    assert (_check(hs, t, np.full(n, np.inf)) == 7).all()
    assert (_check(hs, t, np.full(n, -np.inf)) == 0).all()
    assert (_check(hs, t, np.full(n, np.nan)) == 0).all()
    x = rng.random(n, dtype=np.float32) * t[:, 7]
    # NaN knots (a NaN logit makes every t[j], j >= 1, NaN): bin 0
    tn = t.copy()
    tn[:, 1:] = np.nan
    assert (_check(hs, tn, x) == 0).all()
    # a NaN suffix t[j0 ..] acts as +inf in both forms
    for j0 in range(1, 8):
        tn = t.copy()
        tn[:, j0:] = np.nan
        assert (_check(hs, tn, x) < j0).all()
    # infinite knots at the end
    ti = t.copy()
    ti[:, 6:] = np.inf
    _check(hs, ti, x)
    _check(hs, ti, np.full(n, np.inf))


def test_bin8_rejects_other_shapes(hs):
    with pytest.raises(RuntimeError):
        hs.bin8(torch.zeros(4, 7), torch.zeros(4), 1)
    with pytest.raises(RuntimeError):
        hs.bin8(torch.zeros(4, 8), torch.zeros(4), 2)
