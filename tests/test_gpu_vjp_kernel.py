"""GPU: nfk_fused_nsf_vjp called directly (kernels.fused_nsf_vjp), every
compiled instance, both directions, against an fp64 CPU reference of the same
operation: orc.fcnn for the logits, tanh of the two hidden pre-activations for
[h1 | 1] and [h2 | 1], autograd through orc.unconstrained_rq_spline in the
NSF_CL parametrisation (flows.py:233-236) for dL/dparams and the upper columns
of dL/dx; the lower columns of dL/dx are the identity part gz[:, lo_out] (0
for a null gz).

Every output is a view into a larger buffer pre-filled with a NaN of a payload
no arithmetic produces, and every guard word must come back unchanged: a
kernel that stores past a row or past the batch fails an assertion and never
leaves the test's own memory (the widest store of any instance is column 95 of
a row; the guards are two rows and, in the wide layout, 160 columns).

Which case reaches which (KBH, tail, K) instance of NFK_VJP_SHAPES is the
fourth column of CASES.  Hidden widths H with H % 32 > 4 run the next larger
k-block count without a tail (make_layout): their last k-block has zero-padded
features that must not be stored ("store_act overrun at padded
hidden widths").

Inputs: the layer's default initialisation, B = 3, rows randn * 1.2, about one
upper element in eight placed outside [-B, B]; every inside upper element
closer than 1e-3 to a knot (fp64, width knots forward, height knots inverse)
is moved to the midpoint of its bin, and that separation is asserted, so every
row is compared and there is no knife-edge exemption.

Tolerances are the project's: dL/dparams and dL/dx within 1e-4 of the
reference's largest element (tests/test_gpu_vjp.py), else at most 4 times the
error of the fp32 CPU autograd of the same function
(test_rqs_coupling_bwd_kernel_vs_fp64_autograd); the activations at rtol 1e-5,
atol 2e-6 (tests/test_gpu_fcnn_dh.py), else max and p99 error within 2 times
those of the fp32 CPU evaluation plus 1e-6 (close_or_on_par,
tests/test_gpu_systems.py).  Column H is exactly 1."""
import pytest
import torch
import torch.nn.functional as F

import nf.flows as nff
from normalizingflow_amd import kernels as K_
from oracle import nf_oracle as orc

pytestmark = pytest.mark.gpu

TB = 3.0            # tail bound B
SEP = 1e-3          # least distance of an inside upper element to a knot
GRAD_TOL = 1e-4     # tests/test_gpu_vjp.py
ACT_RTOL, ACT_ATOL = 1e-5, 2e-6   # tests/test_gpu_fcnn_dh.py
WIDE = 160          # row stride of the wide h1 / h2 layout
SENTINEL = 0x7FC0BEEF  # a quiet NaN whose payload no instruction generates

# (size, dim, K, hidden, mask), (KBH, tail, K) instance reached, why
CASES = [
    ((8, 2, 4, 33, [0]), (1, 1, 4), "instance no layer test ran"),
    ((6, 2, 8, 36, [1]), (1, 1, 8), "full 4-feature tail; n_up 6: a ragged 8-coordinate chunk"),
    ((16, 2, 4, 64, [1]), (2, 0, 4), ""),
    ((16, 2, 8, 64, [0]), (2, 0, 8), "instance no layer test ran"),
    ((16, 2, 4, 96, [0]), (3, 0, 4), "instance no layer test ran"),
    ((16, 2, 8, 96, [1]), (3, 0, 8), ""),
    ((16, 2, 4, 100, [0]), (3, 1, 4), "instance no layer test ran"),
    ((16, 2, 8, 97, [0]), (3, 1, 8), "tail of one feature"),
    ((16, 2, 8, 37, [0]), (2, 0, 8), "padded: 27 zero features in the last k-block"),
    ((16, 2, 8, 50, [0]), (2, 0, 8), "padded"),
    ((16, 2, 4, 63, [0]), (2, 0, 4), "padded: one zero feature"),
    ((16, 2, 8, 69, [0]), (3, 0, 8), "padded"),
    ((16, 2, 8, 80, [0]), (3, 0, 8), "padded: the RealNVP / Gaussian configurations' width"),
    ((16, 2, 4, 95, [0]), (3, 0, 4), "padded: one zero feature"),
    ((8, 3, 8, 100, [1]), (3, 1, 8), "non-adjacent maps, n_lo 8, n_up 16"),
    ((8, 3, 8, 100, [0, 2]), (3, 1, 8), "n_lo 16, n_up 8"),
    ((32, 4, 8, 100, [0]), (3, 1, 8), "n_lo 32, D 128: the largest shape vjp_ok admits"),
]
SHAPES = [c[0] for c in CASES]
PADDED = (16, 2, 8, 50, [0])
UNPADDED = (16, 2, 8, 100, [1])
EDGE_BATCHES = [1, 15, 16, 17, 63, 64, 65, 129]   # 16 rows per wave, 64 per workgroup


def _sid(s):
    return "s%d_d%d_k%d_h%d_m%s" % (s[0], s[1], s[2], s[3], "".join(map(str, s[4])))


def _instance(hidden):
    """(KBH, tail) of a hidden width, as make_layout chooses them."""
    kbf, rem = divmod(hidden, 32)
    if rem == 0:
        return kbf, 0
    if rem <= 4 and kbf >= 1:
        return kbf, 1
    return kbf + 1, 0


def test_case_table_reaches_every_instance():
    want = {(h, t, k) for h, t in ((1, 1), (2, 0), (3, 0), (3, 1)) for k in (4, 8)}
    for shape, inst, _ in CASES:
        assert _instance(shape[3]) + (shape[2],) == inst, shape
    assert {inst for _, inst, _ in CASES} == want


_LAYERS = {}


def _layer(shape, dev):
    """(CPU fp32 state dict, column maps, VJP pack) of the shape's layer, built once."""
    key = _sid(shape)
    if key not in _LAYERS:
        size, dim, K, hidden, mask = shape
        torch.manual_seed(11 + size + K + hidden + dim)
        layer = nff.NSF_CL(size=size, dim=dim, K=K, B=3, hidden_dim=hidden, mask=mask)
        sd = {k: v.detach().clone() for k, v in layer.state_dict().items()}
        layer = layer.to(dev)
        maps = layer._maps(dev)
        vpack = layer._vjp_pack(dev)
        assert vpack is not None and layer.__dict__["_vjp_cache"][2] == hidden
        _LAYERS[key] = (sd, maps, vpack)
    return _LAYERS[key]


def _logits(lo, sd):
    """(h1, h2, raw [B, n_up * P]) of the conditioner in lo's precision."""
    p = {k: v.to(lo.dtype) for k, v in sd.items()}
    h1 = torch.tanh(F.linear(lo, p["psi.network.0.weight"], p["psi.network.0.bias"]))
    h2 = torch.tanh(F.linear(h1, p["psi.network.2.weight"], p["psi.network.2.bias"]))
    raw = orc.fcnn(lo, p, "psi.")
    return h1, h2, raw


def _edges(raw, K, inverse):
    """fp64 knots [B, n_up, K + 1] of the direction's search axis."""
    u = raw[..., K:2 * K] if inverse else raw[..., :K]
    e, _ = orc._knots(2 * TB * torch.softmax(u, dim=-1), -TB, TB,
                      orc.MIN_BIN_HEIGHT if inverse else orc.MIN_BIN_WIDTH)
    return e


def _inputs(shape, maps, sd, batch, inverse, seed):
    """x, gz [batch, D], gld [batch] (CPU fp32) with the upper elements of x kept
    SEP away from every knot; also returns the boolean [batch, n_up] tail mask."""
    size, dim, K, hidden, mask = shape
    D = size * dim
    lo_in, _, up_in, _ = maps.lists
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(batch, D, generator=g) * 1.2
    gz = torch.randn(batch, D, generator=g)
    gld = torch.randn(batch, generator=g)
    up = x[:, up_in]
    far = torch.rand(up.shape, generator=g) < 0.125
    side = torch.where(torch.rand(up.shape, generator=g) < 0.5, -1.0, 1.0)
    up = torch.where(far, side * (TB + 0.05 + 1.5 * torch.rand(up.shape, generator=g)), up)
    outside = ~((up >= -TB) & (up <= TB))
    # a drawn value just past the bound: clear of it as well
    up = torch.where(outside & (up.abs() < TB + SEP), torch.sign(up) * (TB + 0.05), up)
    # the knots depend on the lower coordinates only
    _, _, raw = _logits(x[:, lo_in].double(), sd)
    edges = _edges(raw.reshape(batch, len(up_in), 3 * K - 1), K, inverse)
    u64 = up.double()
    near = ((u64[..., None] - edges).abs().amin(dim=-1) < SEP) & ~outside
    k = ((u64[..., None] >= edges).sum(dim=-1) - 1).clamp(0, K - 1)
    mid = 0.5 * (edges.gather(-1, k[..., None]) + edges.gather(-1, k[..., None] + 1))[..., 0]
    up = torch.where(near, mid.float(), up)
    x[:, up_in] = up
    outside = ~((up >= -TB) & (up <= TB))
    dist = (up.double()[..., None] - edges).abs().amin(dim=-1)
    assert float(dist.min()) >= SEP, "an upper element %.3g from a knot" % float(dist.min())
    if outside.numel() >= 256:   # both branches present (a batch of 1 may have no tail element)
        assert bool(outside.any()) and not bool(outside.all())
    return x, gz, gld, outside


def _reference(shape, maps, sd, x, gz, gld, inverse, dtype):
    """h1, h2, gparams [B, n_up, P], gx [B, D] in dtype on the CPU."""
    size, dim, K, hidden, mask = shape
    lo_in, lo_out, up_in, up_out = maps.lists
    B, P = x.shape[0], 3 * K - 1
    xx = x.to(dtype)
    h1, h2, raw = _logits(xx[:, lo_in], sd)
    u = raw.reshape(B, len(up_in), P).detach().requires_grad_(True)
    xu = xx[:, up_in].clone().requires_grad_(True)
    y, lad = orc.unconstrained_rq_spline(xu, 2 * TB * torch.softmax(u[..., :K], -1),
                                         2 * TB * torch.softmax(u[..., K:2 * K], -1), F.softplus(u[..., 2 * K:]),
                                         inverse=inverse, tail_bound=TB, strict=False)
    loss = y.sum() * 0
    if gz is not None:
        loss = loss + (y * gz.to(dtype)[:, up_out]).sum()
    if gld is not None:
        loss = loss + (lad.sum(1) * gld.to(dtype)).sum()
    loss.backward()
    gx = torch.zeros(B, x.shape[1], dtype=dtype)
    gx[:, up_in] = xu.grad
    if gz is not None:
        gx[:, lo_in] = gz.to(dtype)[:, lo_out]
    return h1.detach(), h2.detach(), u.grad, gx


def _filled(*shape, dev):
    t = torch.empty(*shape, dtype=torch.float32, device=dev)
    t.view(torch.int32).fill_(SENTINEL)
    return t


def _untouched(t):
    return bool((t.contiguous().view(torch.int32) == SENTINEL).all())


def _launch(shape, maps, vpack, xd, gzd, gldd, inverse, wide, dev):
    """One launch into guarded buffers; the guards are checked here.  Returns
    CPU copies of h1, h2 [B, H + 1], gparams [B, n_up, P] and gx [B, D]."""
    size, dim, K, hidden, mask = shape
    B, D, H = xd.shape[0], size * dim, hidden
    n_up, P = len(maps.lists[2]), 3 * K - 1
    ldh = (H + 4) // 4 * 4
    gxb = _filled(B + 2, D + 4, dev=dev)
    gpb = _filled(B + 2, n_up * P, dev=dev)
    hb = [_filled(B + 2, WIDE if wide else ldh, dev=dev) for _ in range(2)]
    h1, h2 = (t[:B, :ldh] for t in hb)
    assert h1.stride(0) == (WIDE if wide else ldh) or B == 1
    K_.fused_nsf_vjp(xd, vpack, maps.up_in, maps.up_out, maps.lo_in, maps.lo_out, H, gzd, gldd,
                     gpb[:B], gxb[:B, :D], h1, h2, K=K, tail_bound=TB, inverse=inverse)
    torch.cuda.synchronize()
    what = "%s %s batch %d %s layout" % (_sid(shape), "inverse" if inverse else "forward", B,
                                        "wide" if wide else "tight")
    assert _untouched(gxb[B:]), what + ": gx rows past the batch written"
    assert _untouched(gxb[:B, D:]), what + ": gx columns >= D written"
    assert _untouched(gpb[B:]), what + ": gparams rows past the batch written"
    for n, t in zip(("h1", "h2"), hb):
        assert _untouched(t[B:]), "%s: %s rows past the batch written" % (what, n)
        if wide:
            bad = (t[:B, ldh:].contiguous().view(torch.int32) != SENTINEL).any(dim=0).nonzero().flatten()
            assert bad.numel() == 0, "%s: %s columns >= ldh %d written: %s" % (
                what, n, ldh, (bad + ldh).tolist())
    return (h1[:, :H + 1].cpu(), h2[:, :H + 1].cpu(), gpb[:B].cpu().reshape(B, n_up, P), gxb[:B, :D].cpu())


def _check_grad(name, ours, r64, ref32):
    """Within GRAD_TOL of the fp64 reference's largest element, else within 4
    times the fp32 CPU autograd's own error."""
    assert bool(torch.isfinite(ours).all()), name
    scale = float(r64.abs().max())
    err = float((ours.double() - r64).abs().max())
    print("%s: max err %.3g, scale %.3g (ratio %.3g)" % (name, err, scale, err / max(scale, 1e-300)))
    if err <= GRAD_TOL * scale:
        return
    e32 = float((ref32().double() - r64).abs().max())
    print("%s: the fp32 autograd's error decides: ours %.3g, fp32 %.3g (ratio %.3g)" % (
        name, err, e32, err / max(e32, 1e-300)))
    assert err <= 4 * e32, "%s: err %.3g > 1e-4 x %.3g and > 4 x the fp32 autograd's %.3g" % (name, err, scale, e32)


def _check_act(name, ours, r64, ref32, H):
    """[h | 1]: columns [0, H) at the fp16-split activations' tolerance, else on
    par with the fp32 CPU evaluation; column H exactly 1."""
    assert bool(torch.isfinite(ours).all()), name
    assert bool((ours[:, H] == 1.0).all()), name + ": column H is not 1"
    eo = (ours[:, :H].double() - r64).abs()
    print("%s: max err %.3g" % (name, float(eo.max())))
    if bool((eo <= ACT_ATOL + ACT_RTOL * r64.abs()).all()):
        return
    eo, er = eo.flatten(), (ref32().double() - r64).abs().flatten()
    qo, qr = torch.quantile(eo, 0.99).item(), torch.quantile(er, 0.99).item()
    print("%s: on-par decides: max ours %.3g fp32 %.3g, p99 ours %.3g fp32 %.3g" % (
        name, eo.max().item(), er.max().item(), qo, qr))
    assert eo.max().item() <= 2 * er.max().item() + 1e-6, (name, eo.max().item(), er.max().item())
    assert qo <= 2 * qr + 1e-6, (name, qo, qr)


def _run_case(shape, inverse, batch, dev, use_gz=True, use_gld=True, strided=False):
    size, dim, K, hidden, mask = shape
    D, H = size * dim, hidden
    n_lo, n_up = len(mask) * size, (dim - len(mask)) * size
    assert K_.fused_nsf_vjp_supported(n_lo, n_up, hidden, K)
    sd, maps, vpack = _layer(shape, dev)
    lo_in, lo_out, up_in, up_out = maps.lists
    x, gz, gld, outside = _inputs(shape, maps, sd, batch, inverse, seed=1000 * batch + hidden + K + (7 if inverse else 0))
    gz_ = gz if use_gz else None
    gld_ = gld if use_gld else None
    xd = x.to(dev)
    gzd = gz.to(dev) if use_gz else None
    gldd = gld.to(dev) if use_gld else None
    tight = _launch(shape, maps, vpack, xd, gzd, gldd, inverse, False, dev)
    wide = _launch(shape, maps, vpack, xd, gzd, gldd, inverse, True, dev)
    again = _launch(shape, maps, vpack, xd, gzd, gldd, inverse, False, dev)
    names = ("h1", "h2", "gparams", "gx")
    for n, a, b, c in zip(names, tight, wide, again):
        assert torch.equal(a, b), n + ": tight and wide layouts differ"
        assert torch.equal(a, c), n + ": two launches differ"
    if strided:
        # every matrix a column slice of a wider buffer: ldx, ldgz, ldgx differ
        # from D and from each other, x starts 4 bytes off 16-byte alignment
        xw = torch.zeros(batch, D + 9, device=dev)
        xw[:, 1:1 + D] = xd
        xs = xw[:, 1:1 + D]
        assert xs.data_ptr() % 16 == 4 and xs.stride(0) == D + 9
        gzw = torch.zeros(batch, D + 6, device=dev)
        gzw[:, 2:2 + D] = gzd
        got = _launch(shape, maps, vpack, xs, gzw[:, 2:2 + D], gldd, inverse, True, dev)   # ldgx = D + 4
        for n, a, b in zip(names, tight, got):
            assert torch.equal(a, b), n + ": strided and contiguous runs differ"
    h1, h2, gp, gx = tight
    r = _reference(shape, maps, sd, x, gz_, gld_, inverse, torch.float64)
    r32 = []

    def ref32(i):
        if not r32:
            r32.extend(_reference(shape, maps, sd, x, gz_, gld_, inverse, torch.float32))
        return r32[i]

    tag = "%s %s batch %d" % (_sid(shape), "inverse" if inverse else "forward", batch)
    _check_act(tag + " h1", h1, r[0], lambda: ref32(0), H)
    _check_act(tag + " h2", h2, r[1], lambda: ref32(1), H)
    _check_grad(tag + " gparams", gp, r[2], lambda: ref32(2))
    _check_grad(tag + " gx", gx, r[3], lambda: ref32(3))
    # lower columns: the identity part, exactly
    assert torch.equal(gx[:, lo_in], gz[:, lo_out] if use_gz else torch.zeros(batch, n_lo))
    # outside the tails: gx = gz exactly and no parameter gradient
    gxu = gx[:, up_in]
    gzu = gz[:, up_out] if use_gz else torch.zeros(batch, n_up)
    assert torch.equal(gxu[outside], gzu[outside])
    assert bool((gp[outside] == 0).all())
    assert bool(torch.isfinite(gxu[~outside]).all()) and bool(torch.isfinite(gp[~outside]).all())


@pytest.mark.parametrize("inverse", [False, True], ids=["fwd", "inv"])
@pytest.mark.parametrize("shape", SHAPES, ids=_sid)
def test_vjp_kernel_every_instance(shape, inverse, hip_device):
    """The whole case table at batch 67 (one full workgroup of four 16-row waves
    and a 3-row wave of the next)."""
    _run_case(shape, inverse, 67, hip_device)


@pytest.mark.parametrize("inverse", [False, True], ids=["fwd", "inv"])
@pytest.mark.parametrize("batch", EDGE_BATCHES)
@pytest.mark.parametrize("shape", [PADDED, UNPADDED], ids=_sid)
def test_vjp_kernel_batch_edges(shape, batch, inverse, hip_device):
    """Batches around the kernel's 16-row waves and 64-row workgroups."""
    _run_case(shape, inverse, batch, hip_device)


@pytest.mark.parametrize("inverse", [False, True], ids=["fwd", "inv"])
@pytest.mark.parametrize("null", ["gz", "gld"])
@pytest.mark.parametrize("shape", [PADDED, UNPADDED], ids=_sid)
def test_vjp_kernel_null_gradients(shape, null, inverse, hip_device):
    """gz = None (zero lower dL/dx, no dL/dz term) and gld = None (no log|det|
    term): the fp64 reference with that term dropped."""
    _run_case(shape, inverse, 67, hip_device, use_gz=null != "gz", use_gld=null != "gld")


@pytest.mark.parametrize("inverse", [False, True], ids=["fwd", "inv"])
def test_vjp_kernel_strided_matrices(inverse, hip_device):
    """x, gz, gx, h1 and h2 all with row strides of their own, x misaligned:
    bitwise the contiguous run."""
    _run_case((8, 3, 8, 100, [1]), inverse, 67, hip_device, strided=True)


def test_vjp_kernel_largest_shape_supported():
    size, dim, K, hidden, mask = SHAPES[-1]
    assert size * dim == 128
    assert K_.fused_nsf_vjp_supported(len(mask) * size, (dim - len(mask)) * size, hidden, K)


def test_vjp_support_predicate():
    ok = K_.fused_nsf_vjp_supported
    assert ok(16, 16, 100, 8) and ok(16, 16, 50, 8) and ok(16, 16, 33, 4)
    for hidden in (24, 32, 66, 128):   # (1,0), (1,0), (2,1), (4,0): not instantiated
        assert not ok(16, 16, hidden, 8), hidden
        assert not ok(16, 16, hidden, 4), hidden
    assert not ok(16, 16, 100, 5)       # K: 4 and 8 only
    assert not ok(33, 31, 100, 8)       # one layer-1 k-block: n_lo <= 32
    assert ok(32, 32, 100, 8)
    for n_lo, n_up in ((16, 15), (16, 14), (15, 16), (7, 7)):   # D % 4 != 0
        assert not ok(n_lo, n_up, 100, 8), (n_lo, n_up)
    assert not ok(32, 100, 100, 8)      # D = 132 > 128
