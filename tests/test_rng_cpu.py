"""CPU checks of rng.py: the integer restatement of Philox4x32-10 against the
Random123 known answers, the addressing of philox_words and the normal draw."""
import math

import numpy as np
import pytest
import torch

from normalizingflow_amd import rng

PI = [0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344]
KAT = [
    ([0] * 4, [0] * 2, [0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8]),
    ([0xffffffff] * 4, [0xffffffff] * 2, [0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd]),
    (PI, [0xa4093822, 0x299f31d0], [0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1]),
]


@pytest.mark.parametrize("counter,key,want", KAT)
def test_known_answers(counter, key, want):
    got = rng.philox4x32(counter, key)
    assert got.dtype == np.uint32 and got.tolist() == want


def test_known_answers_batched():
    got = rng.philox4x32([k[0] for k in KAT], [k[1] for k in KAT])
    assert got.tolist() == [k[2] for k in KAT]


def _u32(t):
    return (t.to(torch.int64) & 0xffffffff).tolist()


def test_words_are_addressed_by_step_particle_row_seed_and_tag():
    seed, step = (1 << 62) + 12345, (1 << 32) + 5
    w = rng.philox_words(seed, rows=3, n=5, step=step, row_base=7, tag=1)
    assert w.shape == (3, 5, 4) and w.dtype == torch.int32
    for b, p in ((0, 0), (2, 4), (1, 3)):
        want = rng.philox4x32([step & 0xffffffff, step >> 32, p, 7 + b],
                              [seed & 0xffffffff, (seed >> 32) | (1 << 31)])
        assert _u32(w[b, p]) == want.tolist()
    # a row alone with its row_base, and a particle range, are sub-blocks of the batch
    assert torch.equal(rng.philox_words(seed, 1, 5, step, row_base=9, tag=1)[0], w[2])
    assert torch.equal(rng.philox_words(seed, 3, 2, step, row_base=7, tag=1), w[:, :2])
    assert not torch.equal(rng.philox_words(seed, 3, 5, step, row_base=7, tag=0), w)
    assert not torch.equal(rng.philox_words(seed, 3, 5, step + 1, row_base=7, tag=1), w)
    assert not torch.equal(rng.philox_words(seed + 1, 3, 5, step, row_base=7, tag=1), w)
    assert _u32(rng.philox_words(0, 1, 1, 0)[0, 0]) == KAT[0][2]


def test_bad_arguments():
    for kw in (dict(seed=1 << 63), dict(seed=-1), dict(step=-1), dict(tag=2), dict(row_base=1 << 32)):
        args = dict(seed=0, rows=1, n=1, step=0, row_base=0, tag=0)
        args.update(kw)
        with pytest.raises(ValueError):
            rng.philox_words(**args)
    with pytest.raises(ValueError):
        rng.philox_normal(0, 1, 1, 5, 0)


def test_normals():
    N = 1 << 18
    z = rng.philox_normal(3, 64, N // 64 // 4, 4, step=11)
    assert z.shape == (64, N // 256, 4) and z.dtype == torch.float32
    zz = z.double().flatten()
    assert abs(float(zz.mean())) < 5 / math.sqrt(N)
    assert abs(float(zz.var()) - 1) < 5 * math.sqrt(2 / N)
    assert float(zz.abs().max()) <= math.sqrt(-2 * math.log(2.0 ** -25)) + 1e-6
    # component d of a particle is normal d: fewer dimensions are a prefix
    assert torch.equal(rng.philox_normal(3, 64, N // 256, 2, step=11), z[..., :2])
    # the first pair by hand
    w = rng.philox_words(3, 1, 1, 11)[0, 0].to(torch.int64) & 0xffffffff
    u = [(float(np.float32((int(x) >> 8) + 0.5) * np.float32(2.0 ** -24))) for x in w]
    r = math.sqrt(-2 * math.log(u[0]))
    assert abs(float(z[0, 0, 0]) - r * math.cos(2 * math.pi * u[1])) < 1e-6
    assert abs(float(z[0, 0, 1]) - r * math.sin(2 * math.pi * u[1])) < 1e-6
    zm = rng.philox_normal(3, 8, 33, 3, step=2, zero_mean=True, dtype=torch.float64)
    assert float(zm.sum(1).abs().max()) < 1e-12
