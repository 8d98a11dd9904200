"""CPU: the bench's synthetic data: the c1 two-moons rows are
seeded, shaped and placed like the make_moons formula; the other workloads
draw x ~ N(0, I)."""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench  # noqa: E402


def test_moons_shape_seed_and_arcs():
    a = bench.moons(4096, generator=torch.Generator().manual_seed(0))
    b = bench.moons(4096, generator=torch.Generator().manual_seed(0))
    assert a.shape == (4096, 2) and a.dtype == torch.float32
    assert torch.equal(a, b)
    # noise-free points lie on the two unit half circles centred (0, 0) and (1, 0.5)
    c = bench.moons(1001, noise=0.0, generator=torch.Generator().manual_seed(1)).double()
    r_out = (c - torch.tensor([0.0, 0.0], dtype=torch.float64)).norm(dim=1)
    r_in = (c - torch.tensor([1.0, 0.5], dtype=torch.float64)).norm(dim=1)
    on_out = (r_out - 1).abs() < 1e-6
    on_in = (r_in - 1).abs() < 1e-6
    assert bool((on_out | on_in).all())
    assert int(on_out.sum()) == 500 and int((on_in & ~on_out).sum()) == 501
    assert bool((c[on_out, 1] >= -1e-6).all()) and bool((c[on_in & ~on_out, 1] <= 0.5 + 1e-6).all())


def test_make_x_per_workload():
    g = torch.Generator().manual_seed(0)
    assert bench.make_x("c1", 64, g, "cpu").shape == (64, 2)
    assert bench.make_x("c3", 64, g, "cpu").shape == (64, 64)
    assert bench.make_x("c5", 8, g, "cpu").shape == (8, 256)
    assert bench.DEFAULT_BATCH.get("c1") == 4096


def test_dump_array_whole_and_sampled(tmp_path):
    """--dump-outputs files: float32 (float64 for a double tensor); an array
    within the budget is written whole, a larger one as the same seeded,
    sorted row sample in every run, with its row numbers beside it."""
    import numpy as np
    d = str(tmp_path / "out")
    lp = torch.arange(1000, dtype=torch.float32) * 0.5
    bench.dump_array(d, "log_prob", lp, 1 << 20)
    a = np.load(os.path.join(d, "log_prob.npy"))
    assert a.dtype == np.float32 and np.array_equal(a, lp.numpy())
    assert not os.path.exists(os.path.join(d, "log_prob_rows.npy"))
    bench.dump_array(d, "nll", torch.tensor(1.25, dtype=torch.float64), 4096)
    n = np.load(os.path.join(d, "nll.npy"))
    assert n.dtype == np.float64 and n.shape == (1,) and n[0] == 1.25
    for name in ("s1", "s2"):
        bench.dump_array(d, name, lp, 1200)
    s1, r1 = np.load(os.path.join(d, "s1.npy")), np.load(os.path.join(d, "s1_rows.npy"))
    s2, r2 = np.load(os.path.join(d, "s2.npy")), np.load(os.path.join(d, "s2_rows.npy"))
    assert np.array_equal(s1, s2) and np.array_equal(r1, r2)
    assert s1.nbytes + r1.nbytes <= 1200 and len(s1) == 100
    assert np.all(np.diff(r1) > 0) and np.array_equal(s1, lp.numpy()[r1.astype(np.int64)])
    assert bench.DUMP_BUDGET_BYTES <= 64 * 1000 * 1000
