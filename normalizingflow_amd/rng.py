"""Counter-based random numbers: Philox4x32-10 (Salmon et al., SC'11, the
Random123 constants) as the device generates it in nfk_rng.h, restated here in
integer arithmetic for the CPU.

A call is addressed, never drawn from a stream:

    counter = (step_lo, step_hi, particle, row)     row = (row_base + b) mod 2^32
    key     = (seed_lo, seed_hi | tag << 31)        0 <= seed < 2^63

``step`` is the absolute 64-bit step index; ``tag`` 0 is thermostat noise and 1
initial velocities.  The four words of a call give four normals by two
Box-Muller pairs, u = ((w >> 8) + 0.5) * 2^-24 rounded to fp32,
z_a = sqrt(-2 log u_a) cos(2 pi u_b), z_b = sqrt(-2 log u_a) sin(2 pi u_b) for
(a, b) = (0, 1) and (2, 3); component d of particle p is normal d, so
``dim <= 4``.

``philox_words`` and ``philox_normal`` fill [rows, n, ...] tensors.  fp32 on the
HIP device is the fill kernel (nfk_philox_fill: fp32 logf / sqrtf / sincospif,
the values the Langevin kernels use); everywhere else the words -- the
kernel's on the device, the restatement's on the CPU, bit for bit the same --
go through an fp64 Box-Muller in torch and are cast to the dtype asked for.
"""
from __future__ import annotations

import math

import numpy as np
import torch

from . import kernels as K_

__all__ = ["philox4x32", "philox_words", "philox_normal"]

_M0, _M1 = 0xD2511F53, 0xCD9E8D57
_W0, _W1 = 0x9E3779B9, 0xBB67AE85
_MASK = 0xFFFFFFFF


def philox4x32(counter, key, rounds=10):
    """Philox4x32-``rounds``: ``counter`` [..., 4] and ``key`` [..., 2] (anything
    ``np.asarray`` takes, values below 2^32, broadcast against each other) ->
    uint32 [..., 4]."""
    c = np.asarray(counter, dtype=np.uint64)
    k = np.asarray(key, dtype=np.uint64)
    if c.shape[-1] != 4 or k.shape[-1] != 2:
        raise ValueError("counter must be [..., 4] and key [..., 2]")
    shape = np.broadcast_shapes(c.shape[:-1], k.shape[:-1])
    c0, c1, c2, c3 = (np.broadcast_to(c[..., i], shape) for i in range(4))
    k0, k1 = (np.broadcast_to(k[..., i], shape) for i in range(2))
    m0, m1, mask = np.uint64(_M0), np.uint64(_M1), np.uint64(_MASK)
    s32 = np.uint64(32)
    for _ in range(rounds):
        p0, p1 = m0 * c0, m1 * c2  # 32 x 32 bits: exact in uint64
        c0, c1, c2, c3 = (p1 >> s32) ^ c1 ^ k0, p1 & mask, (p0 >> s32) ^ c3 ^ k1, p0 & mask
        k0, k1 = (k0 + np.uint64(_W0)) & mask, (k1 + np.uint64(_W1)) & mask
    return np.stack((c0, c1, c2, c3), axis=-1).astype(np.uint32)


def _check(seed, rows, n, step, row_base, tag):
    seed, rows, n, step, row_base, tag = int(seed), int(rows), int(n), int(step), int(row_base), int(tag)
    if not 0 <= seed < (1 << 63):
        raise ValueError("seed must be in [0, 2^63), got %d" % seed)
    if step < 0 or rows < 0 or n <= 0 or row_base < 0 or row_base + rows > (1 << 32):
        raise ValueError("step, rows and row_base must be >= 0, n > 0 and row_base + rows <= 2^32")
    if tag not in (0, 1):
        raise ValueError("tag must be 0 (thermostat noise) or 1 (initial velocities)")
    return seed, rows, n, step, row_base, tag


def _on_hip(device):
    return torch.device(device).type == "cuda"


def philox_words(seed, rows, n, step, row_base=0, tag=0, device="cpu"):
    """The raw words of particles 0..n-1 of rows row_base..row_base+rows-1 at
    ``step``: int32 [rows, n, 4] (the uint32 bit patterns)."""
    seed, rows, n, step, row_base, tag = _check(seed, rows, n, step, row_base, tag)
    if _on_hip(device):
        out = torch.empty(rows, n, 4, dtype=torch.int32, device=device)
        K_.philox_fill(out, n=n, dim=4, step=step, seed=seed, row_base=row_base, tag=tag, normals=False)
        return out
    counter = np.empty((rows, n, 4), dtype=np.uint64)
    counter[..., 0] = step & _MASK
    counter[..., 1] = step >> 32
    counter[..., 2] = np.arange(n, dtype=np.uint64)[None, :]
    counter[..., 3] = ((np.arange(rows, dtype=np.uint64) + np.uint64(row_base)) & np.uint64(_MASK))[:, None]
    key = np.array([seed & _MASK, (seed >> 32) | (tag << 31)], dtype=np.uint64)
    return torch.from_numpy(philox4x32(counter, key).view(np.int32)).to(device)


def normals_from_words(words, dim=4, zero_mean=False, dtype=torch.float32):
    """The fp64 Box-Muller of int32 words [rows, n, 4] -> [rows, n, dim] in
    ``dtype``; ``zero_mean`` removes each dimension's mean over the n particles
    (in fp64)."""
    if not 1 <= dim <= 4:
        raise ValueError("dim must be 1..4: a call yields four normals")
    w = words.to(torch.int64) & _MASK
    u = (((w >> 8).to(torch.float32) + 0.5) * 2.0 ** -24).double()  # the device's fp32 u
    r = torch.sqrt(-2.0 * torch.log(u[..., 0::2]))
    ang = (2.0 * math.pi) * u[..., 1::2]
    z = torch.stack((r * torch.cos(ang), r * torch.sin(ang)), dim=-1).reshape(*w.shape[:-1], 4)[..., :dim]
    if zero_mean:
        z = z - z.mean(dim=-2, keepdim=True)
    return z.to(dtype)


def philox_normal(seed, rows, n, dim, step, row_base=0, tag=0, zero_mean=False, device="cpu",
                  dtype=torch.float32):
    """Normals [rows, n, dim]: component d of particle p of row b is normal d of
    the call (step, p, row_base + b).  ``zero_mean`` subtracts each dimension's
    mean over the row's particles (the thermostat's ``zero yes``)."""
    if not 1 <= int(dim) <= 4:
        raise ValueError("dim must be 1..4: a call yields four normals")
    if _on_hip(device) and dtype == torch.float32:
        seed, rows, n, step, row_base, tag = _check(seed, rows, n, step, row_base, tag)
        out = torch.empty(rows, n, int(dim), dtype=torch.float32, device=device)
        K_.philox_fill(out, n=n, dim=int(dim), step=step, seed=seed, row_base=row_base, tag=tag,
                       zero_mean=zero_mean, normals=True)
        return out
    return normals_from_words(philox_words(seed, rows, n, step, row_base, tag, device), int(dim), zero_mean, dtype)
