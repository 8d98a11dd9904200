"""The bytes of every weight pack (csrc/nfk_pack.h) against recorded hashes.

Each case builds float32 weights on the CPU from a seeded numpy generator
(every Linear scaled by a different constant, so the three scale exponents
differ), calls the pack function of normalizingflow_amd.kernels and compares
sha256 of the pack's bytes with tests/golden/pack_sha256.json.

    python tests/test_gpu_pack_format.py --write

regenerates the JSON on a GPU.  Before it records a hash it packs a second
time into the same block after filling it with 0xFF bytes: a pack with words
no kernel writes is reported and left out.
"""
import hashlib
import json
import os
import sys

import numpy as np
import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

from normalizingflow_amd import kernels as K_  # noqa: E402

GOLDEN = os.path.join(REPO, "tests", "golden", "pack_sha256.json")
SCALES = (3.7, 0.02, 150.0)  # layer 1, 2, 3: three different scale exponents


def _fcnn(rng, n_in, H, n_out, zero=None):
    """(W0, b0, W2, b2, W4, b4) of FCNN(n_in, n_out, H); zero: index of a Linear set to 0."""
    out = []
    for l, (r, c) in enumerate(((H, n_in), (H, H), (n_out, H))):
        W = (rng.standard_normal((r, c)) * SCALES[l]).astype(np.float32)
        if zero == l:
            W[:] = 0.0
        out += [W, rng.standard_normal(r).astype(np.float32)]
    return out


def _dev(ws, dev):
    return [torch.from_numpy(w).to(dev) for w in ws]


def _nsf(fn, ok):
    def run(rng, dev, n_lo, n_up, H, K, zero=None):
        assert ok(n_lo, n_up, H, K), "shape not supported"
        ws = _dev(_fcnn(rng, n_lo, H, n_up * (3 * K - 1), zero), dev)
        return lambda: fn(*ws, n_lo, n_up, H, K)
    return run


def _rnvp(rng, dev, half, H):
    assert K_.fused_realnvp_supported(half, H), "shape not supported"
    nets = _dev([w for _ in range(4) for w in _fcnn(rng, half, H, half)], dev)
    return lambda: K_.fused_realnvp_pack(nets, half, H)


def _ar(rng, dev, dim, H, K, stream=False):
    P = 3 * K - 1
    ws = [_dev(_fcnn(rng, 2 * i, H, P), dev) for i in range(1, dim)]
    init = torch.from_numpy(rng.standard_normal(P).astype(np.float32)).to(dev)
    lib = K_._lib.load()

    def pack():
        prev = lib.nfk_debug_ar_stream(1) if stream else None
        try:
            assert K_.fused_ar_supported(dim, H, K), "shape not supported"
            assert bool(K_.fused_ar_inverse_supported(dim, H, K)) != stream, "not the layout this case names"
            return K_.fused_ar_pack(ws, init, dim, H, K)[0]
        finally:
            if stream:
                lib.nfk_debug_ar_stream(prev)
    return pack


def _lin(fn):
    def run(rng, dev, N, Kd):
        W = torch.from_numpy((rng.standard_normal((N, Kd)) * SCALES[0]).astype(np.float32)).to(dev)

        def pack():
            out = fn(W)
            assert out is not None, "shape not supported"
            return out
        return pack
    return run


_NSF = _nsf(K_.fused_nsf_pack, K_.fused_nsf_supported)
_VJP = _nsf(K_.fused_nsf_vjp_pack, K_.fused_nsf_vjp_supported)

# name -> (builder, arguments); the seed of a case is its position in this list
CASES = [
    ("nsf_2_2_32_4", _NSF, (2, 2, 32, 4)),            # T1 = 0, KBH = 1
    ("nsf_3_5_36_5", _NSF, (3, 5, 36, 5)),            # T1 = 1, ragged tiles
    ("nsf_32_32_100_8", _NSF, (32, 32, 100, 8)),      # c3
    ("nsf_8_8_128_16", _NSF, (8, 8, 128, 16)),        # the wide frame stream
    ("nsf_2_1_100_32", _NSF, (2, 1, 100, 32)),        # k_fused_cl's pack
    ("nsf_32_64_354_32", _NSF, (32, 64, 354, 32)),    # k_fused_cl's pack, the applications' width
    ("nsf_32_32_100_8_zero_w2", _NSF, (32, 32, 100, 8, 1)),  # nfk_scale_exp(0)
    ("vjp_32_32_100_8", _VJP, (32, 32, 100, 8)),
    ("vjp_1_3_33_4", _VJP, (1, 3, 33, 4)),            # the smallest other shape the VJP takes
    ("rnvp_16_64", _rnvp, (16, 64)),
    ("rnvp_16_100", _rnvp, (16, 100)),
    ("rnvp_32_100", _rnvp, (32, 100)),
    ("rnvp_64_68", _rnvp, (64, 68)),                  # (64, 100) is not supported: the widest T1 = 1 at half 64
    ("ar_4_16_4", _ar, (4, 16, 4)),
    ("ar_5_80_10", _ar, (5, 80, 10)),                 # the 16-feature tail, T1 = 2
    ("ar_5_100_8", _ar, (5, 100, 8)),
    ("ar_5_354_32", _ar, (5, 354, 32)),
    ("ar_35_100_32", _ar, (35, 100, 32)),             # two layer-1 k-blocks
    ("ars_5_100_32", _ar, (5, 100, 32, True)),        # the streamed layout (k_ars_pack)
    ("ars_35_100_32", _ar, (35, 100, 32, True)),
    ("wlin_20_40", _lin(K_.wlin_pack), (20, 40)),
    # fcnn_dh_pack has no case: words 4..63 of its header block are written by no kernel
]


def _packer(name, dev):
    i = [c[0] for c in CASES].index(name)
    _, build, args = CASES[i]
    return build(np.random.default_rng(1000 + i), dev, *args)


def _sha(pack):
    return hashlib.sha256(pack.cpu().numpy().tobytes()).hexdigest()


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


@pytest.mark.gpu
@pytest.mark.parametrize("name", [c[0] for c in CASES])
def test_pack_bytes(name, hip_device, golden):
    assert name in golden, "no recorded hash (a pack with unwritten words is left out: see the module docstring)"
    assert _sha(_packer(name, hip_device)()) == golden[name]


def _write():
    dev = torch.device("cuda:0")
    out = {}
    for name, _, _ in CASES:
        pack_fn = _packer(name, dev)
        pack = pack_fn()
        h, n, ptr = _sha(pack), pack.numel(), pack.data_ptr()
        del pack
        fill = torch.full((4 * n,), 0xFF, dtype=torch.uint8, device=dev)
        same = fill.data_ptr() == ptr
        del fill
        pack = pack_fn()
        same = same and pack.data_ptr() == ptr
        if not same:
            print("%-28s NOT RECORDED: the allocator gave another block, coverage unchecked" % name)
        elif _sha(pack) != h:
            a = np.frombuffer(pack.cpu().numpy().tobytes(), dtype=np.uint32)
            print("%-28s NOT RECORDED: %d of %d words are written by no kernel, first at %d"
                  % (name, int((a == 0xFFFFFFFF).sum()), n, int(np.argmax(a == 0xFFFFFFFF))))
        else:
            out[name] = h
            print("%-28s %9d words %s" % (name, n, h[:16]))
        del pack
    with open(GOLDEN, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    if sys.argv[1:] != ["--write"]:
        sys.exit("usage: python tests/test_gpu_pack_format.py --write")
    _write()
