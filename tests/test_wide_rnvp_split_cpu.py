"""CPU: the design of nfk_wide_rnvp.hip's arithmetic, apart from its kernels.

widernvp.rnvp_split restates on the CPU what the weight-stream RealNVP kernels
compute (fp16 hi/lo operands at power-of-two scales, three MFMA products per
32-wide k-block in fp32 accumulators, chunks added in order).  It must meet
the error rule of test_gpu_wide_rnvp_kernels.py -- max and p99 error against
the fp64 reference within 2x the fp32 reference's own -- at every master
shape but the large one, so that a kernel that misses the rule on the GPU is
a kernel bug and not the design.  Broken on purpose (an operand's lo half
dropped, one k-block skipped) it must miss the rule: the rule sees such bugs.
The plan table (widernvp.wl_plan, a restatement of wl_plan) is checked for
the tile counts, chunk lengths and edges the GPU module's shapes are there for.
"""
import pytest

import widernvp as wr

PF = 8  # k-blocks of weights in flight per wave of the default k_wl_gemm instance


def _plans(shape):
    return [wr.wl_plan(N, K) for N, K in wr.stages(*shape)]


def test_plan_table_covers_the_edges():
    print(wr.plan_table())
    l1, l2, l3 = _plans((4, 16))
    assert l1["NT"] == l2["NT"] == l3["NT"] == 1 and l1["KB"] == l2["KB"] == 1 and l1["waves"] == 1
    l1, l2, l3 = _plans((20, 300))
    assert l1["KB"] == 1 and l1["NT"] == 19 and 300 % 32 == 12
    assert (l2["KW"], l2["waves"], l2["wlast"]) == (3, 4, 1)
    l1, l2, l3 = _plans((36, 44))
    assert 36 % 32 == 4 and 36 % 16 == 4 and l1["NT"] == 3
    l1, l2, l3 = _plans((60, 52))
    assert 60 % 32 == 28 and 60 % 16 == 12 and l1["NT"] == 4 and 52 % 32 == 20
    l1, l2, l3 = _plans((132, 260))
    assert (l1["KB"], l1["KW"], l1["waves"], l1["wlast"]) == (5, 2, 3, 1)
    assert l2["KB"] == 9 and l1["NT"] == 17 and l3["NT"] == 9 and 17 % 8 == 1 and 9 % 8 == 1
    l1, l2, l3 = _plans((128, 256))
    assert 128 % 32 == 0 and 256 % 32 == 0 and l1["NT"] % 8 == 0 and l3["NT"] % 8 == 0
    # every small shape: one k-block per chunk
    for shape in wr.SMALL:
        assert all(p["KC"] == 1 for p in _plans(shape)), shape
    l1, l2, l3 = _plans(wr.MID)
    assert (l1["KS"], l1["KC"], l1["last"]) == (8, 2, 2)
    assert (l2["KS"], l2["KC"], l2["last"]) == (12, 3, 2)
    assert (l3["KS"], l3["KC"], l3["last"]) == (18, 2, 1)
    assert max(p["KC"] for p in (l1, l2, l3)) < PF
    l1, l2, l3 = _plans(wr.LARGE)
    assert (l1["KB"], l1["KC"], l1["KS"], l1["last"]) == (65, 9, 8, 2)
    assert l2["KC"] == 8
    assert (l3["NT"], l3["KC"], l3["KS"], l3["last"]) == (129, 10, 7, 4)
    assert l1["KC"] > PF and l1["KC"] % PF and l3["KC"] > PF and l3["KC"] % PF
    # KS = 1 needs nblk > 128, N >= 8208: left out (270 MB per hidden-by-hidden matrix)
    assert all(p["KS"] > 1 or p["KB"] == 1 for s in wr.SHAPES for p in _plans(s))


_CASES = {}


def _case(shape, gain):
    key = (shape, gain)
    if key not in _CASES:
        Ws, bs = wr.make_layer(*shape, gain)
        _CASES[key] = (Ws, bs, wr.make_x(shape[0]))
    return _CASES[key]


@pytest.mark.parametrize("gain", [1, 3])
@pytest.mark.parametrize("shape", wr.SMALL + [wr.MID], ids=wr.ids)
def test_restatement_meets_the_error_rule(shape, gain):
    Ws, bs, X = _case(shape, gain)
    for inverse in (False, True):
        for rows in (64, 128):
            x = X[:rows]
            z64, ld64, z32, ld32 = wr.refs(x, Ws, bs, inverse)
            z, ld = wr.rnvp_split(x, Ws, bs, inverse, fused=rows <= 64)
            label = "%s g%d %s %d" % (wr.ids(shape), gain, "inv" if inverse else "fwd", rows)
            wr.assert_rule(z, z32, z64, label + " z")
            wr.assert_rule(ld, ld32, ld64, label + " ld")


@pytest.mark.parametrize("opt", [dict(drop_w_lo=True), dict(drop_x_lo=True), dict(skip_block=1)],
                         ids=["no-w-lo", "no-x-lo", "skip-k-block"])
@pytest.mark.parametrize("shape", [(36, 44), (132, 260)], ids=wr.ids)
def test_broken_restatement_misses_the_error_rule(shape, opt):
    """Sensitivity: without the lo half of the weights or of the inputs (a
    relative error near 2^-11 per product), or with one k-block left out of
    every stage, z misses the rule in both directions."""
    Ws, bs, X = _case(shape, 1)
    for inverse in (False, True):
        x = X[:64]
        z64, ld64, z32, ld32 = wr.refs(x, Ws, bs, inverse)
        z, ld = wr.rnvp_split(x, Ws, bs, inverse, fused=True, **opt)
        ok, ratio = wr.rule(z, z32, z64, "%s broken %s" % (wr.ids(shape), sorted(opt)))
        assert not ok and ratio > 10.0, ratio


def test_pack_reference_splits_exactly():
    """hi + lo of wlin_pack_ref reproduces 2^s W to 2^-22 |2^s w| (both halfs
    normal), or 2^-25 where lo is a subnormal half."""
    import torch
    W = wr.make_layer(20, 300, 1)[0][0]
    hdr, body, tail = wr.wlin_pack_ref(W)
    N, K = W.shape
    h = body.view(torch.float16).double()
    NT, KB = body.shape[:2]
    back = (h[:, :, 0] + h[:, :, 1]).view(NT, KB, 4, 16, 8).permute(0, 3, 1, 2, 4).reshape(16 * NT, 32 * KB)
    ws = W.double() / float(hdr[0])
    err = (back[:N, :K] - ws).abs()
    assert bool((err <= torch.maximum(ws.abs() * 2.0 ** -22, torch.tensor(2.0 ** -25, dtype=torch.float64))).all())
    assert float(back[N:].abs().max()) == 0.0 and float(back[:, K:].abs().max()) == 0.0
    assert float(ws.abs().max()) < 2.0 ** 15 and float(ws.abs().max()) >= 2.0 ** 14
