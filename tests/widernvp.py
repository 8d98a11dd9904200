"""Shared pieces of test_gpu_wide_rnvp_kernels.py and test_wide_rnvp_split_cpu.py:
shapes, seeded weights, the fp64 / fp32 CPU reference of one RealNVP layer
(nf/flows.py:44-76 over FCNN conditioners, 20-35), a restatement of
nfk_wide_rnvp.hip's stage plan and of its arithmetic on the CPU, the reference
of nfk_wlin_pack, and the comparison rule.

Weights and biases come in the kernel's pack order ``6 c + 2 l + g``
(half-coupling c: 0 = s1/t1, 1 = s2/t2; Linear l of the FCNN; g: 0 = s, 1 = t).

The error rule (``rule``): the kernel's error against the fp64 reference, max
and 99th percentile over all elements of a run, is at most ``FACTOR`` times
the fp32 reference's own (close_or_on_par's factor in test_gpu_parity.py); no
additive floor.
"""
import math

import torch

FACTOR = 2.0
SMALL = [(4, 16), (20, 300), (36, 44), (60, 52), (132, 260), (128, 256)]
MID = (512, 1100)
LARGE = (2052, 2048)
SHAPES = SMALL + [MID, LARGE]
# MT 1 ... 8 on both sides of the fused / split-K switch at 64 / 65 rows, and
# second and third passes of MT 1, 4 and 5 (129, 192, 200, 257)
BATCHES = [1, 15, 16, 17, 33, 48, 49, 63, 65, 81, 97, 113, 127, 129, 192, 200, 257]
ROWS = 128     # rows of X of a case: the 128-row master; the 64-row master is its prefix
S_MAX = 8.0    # every case: max |s| of the fp64 reference (exp nowhere near overflow)
# every matrix is U(+-1/sqrt(K)) * gain * _FACT[i % 3], so that the packs of a
# layer carry different power-of-two scales (make_layer asserts three exponents)
_FACT = (1.0, 0.45, 0.2)
# one seed for every case.  (It was chosen while the coupling was still
# computed in fp32: seed 0 puts, at (4, 16) and gain 3, a single output alone
# in the top binade, |z| = 2.17, where that restatement was 1.3 ulp off and
# the fp32 reference 0.3 ulp, 2.7 x; seeds 1 ... 7 gave 0.4 ... 1.8.  With the
# coupling in double the restatement is within 0.95 x at seed 0 as well.)
SEED = 1


def ids(shape):
    return "h%d-H%d" % shape


# ---------------------------------------------------------------------------
# the stage plan (wl_plan, k_wl_gemm_act's KW)
def cdiv(a, b):
    return (a + b - 1) // b


def wl_plan(N, K):
    """The split-K plan of one GEMM stage [M, K] x [N, K]^T (wl_plan): a dict
    of NT, nblk, KB, KS, KC, last (k-blocks of the last chunk) and the fused
    stage's KW (k-blocks per wave) and its last live wave's share."""
    NT, KB = cdiv(N, 16), cdiv(K, 32)
    nblk = cdiv(NT, 8)
    ks = max(1, min(256 // (2 * nblk), KB))
    KC = cdiv(KB, ks)
    KS = cdiv(KB, KC)
    KW = cdiv(KB, 4)
    live = cdiv(KB, KW)
    return dict(N=N, K=K, NT=NT, nblk=nblk, KB=KB, KS=KS, KC=KC, last=KB - (KS - 1) * KC, KW=KW, waves=live,
                wlast=KB - (live - 1) * KW)


def stages(half, hidden):
    """The three stages (L1, L2, L3) of a half-coupling as (N, K)."""
    return [(hidden, half), (hidden, hidden), (half, hidden)]


def plan_table(shapes=None):
    out = ["half hidden stage    N     K  NT nblk  KB  KS  KC last | fused: KW waves last"]
    for half, hidden in shapes or SHAPES:
        for l, (N, K) in enumerate(stages(half, hidden)):
            p = wl_plan(N, K)
            fused = "%9d %5d %4d" % (p["KW"], p["waves"], p["wlast"]) if l < 2 else ""
            out.append("%4d %6d    L%d %4d %5d %3d %4d %3d %3d %3d %4d | %s"
                       % (half, hidden, l + 1, N, K, p["NT"], p["nblk"], p["KB"], p["KS"], p["KC"], p["last"], fused))
    return "\n".join(out)


def chunks(K, N, fused):
    """The k-block ranges whose sums meet in fp32, in the order they are
    added: the four waves' shares of k_wl_gemm_act, or wl_plan's splits."""
    p = wl_plan(N, K)
    step = p["KW"] if fused else p["KC"]
    return [(k0, min(k0 + step, p["KB"])) for k0 in range(0, p["KB"], step)]


# ---------------------------------------------------------------------------
# inputs
def make_layer(half, hidden, gain, seed=SEED):
    """12 weights and 12 biases (fp32, CPU) of one layer in pack order."""
    g = torch.Generator().manual_seed(100003 * half + 17 * hidden + seed)
    Ws, bs = [None] * 12, [None] * 12
    for c in range(2):
        for l, (n, k) in enumerate(stages(half, hidden)):
            for gr in range(2):
                i = 6 * c + 2 * l + gr
                bound = 1.0 / math.sqrt(k)
                Ws[i] = ((torch.rand(n, k, generator=g) * 2 - 1) * (bound * gain * _FACT[i % 3])).contiguous()
                bs[i] = ((torch.rand(n, generator=g) * 2 - 1) * bound).contiguous()
    exps = {math.frexp(float(W.abs().max()))[1] for W in Ws}
    assert len(exps) >= 3, exps
    return Ws, bs


def make_x(half, rows=ROWS, seed=SEED):
    return 0.5 * torch.randn(rows, 2 * half, generator=torch.Generator().manual_seed(half + 31 * seed + 5))


def batch_of(X, B):
    """B rows as passes of at most 128 rows, each a prefix of X."""
    parts = [X[:min(128, B - r0)] for r0 in range(0, B, 128)]
    return torch.cat(parts) if len(parts) > 1 else parts[0].clone()


def passes(B):
    return [(r0, min(128, B - r0)) for r0 in range(0, B, 128)]


# ---------------------------------------------------------------------------
# the reference: plain torch, in the dtype of the call
def _mlp(x, Ws, bs, c, g):
    h = torch.tanh(x @ Ws[6 * c + g].T + bs[6 * c + g])
    h = torch.tanh(h @ Ws[6 * c + 2 + g].T + bs[6 * c + 2 + g])
    return h @ Ws[6 * c + 4 + g].T + bs[6 * c + 4 + g]


def rnvp_ref(x, Ws, bs, inverse, dtype):
    """(z, log|det|, max|s|, per-row sum |s|) of one layer, computed in ``dtype`` on the CPU."""
    x = x.to(dtype)
    Ws, bs = [W.to(dtype) for W in Ws], [b.to(dtype) for b in bs]
    h = x.shape[1] // 2
    lower, upper = x[:, :h], x[:, h:]
    if not inverse:
        t1, s1 = _mlp(lower, Ws, bs, 0, 1), _mlp(lower, Ws, bs, 0, 0)
        upper = t1 + upper * torch.exp(s1)
        t2, s2 = _mlp(upper, Ws, bs, 1, 1), _mlp(upper, Ws, bs, 1, 0)
        lower = t2 + lower * torch.exp(s2)
        ld = torch.sum(s1, dim=1) + torch.sum(s2, dim=1)
    else:
        t2, s2 = _mlp(upper, Ws, bs, 1, 1), _mlp(upper, Ws, bs, 1, 0)
        lower = (lower - t2) * torch.exp(-s2)
        t1, s1 = _mlp(lower, Ws, bs, 0, 1), _mlp(lower, Ws, bs, 0, 0)
        upper = (upper - t1) * torch.exp(-s1)
        ld = torch.sum(-s1, dim=1) + torch.sum(-s2, dim=1)
    smax = max(float(s1.abs().max()), float(s2.abs().max()))
    return torch.cat([lower, upper], dim=1), ld, smax, s1.abs().sum(dim=1) + s2.abs().sum(dim=1)


def refs(x, Ws, bs, inverse):
    """(z64, ld64, z32, ld32): the truth and the comparator; asserts max|s| <= 8."""
    z64, ld64, smax, _ = rnvp_ref(x, Ws, bs, inverse, torch.float64)
    assert smax <= S_MAX, "max|s| = %.3g: the inputs put exp near overflow" % smax
    z32, ld32 = rnvp_ref(x, Ws, bs, inverse, torch.float32)[:2]
    return z64, ld64, z32, ld32


# ---------------------------------------------------------------------------
# the comparison rule
def errors(k, r, t):
    ek, er = (k.detach().cpu().double() - t).abs().flatten(), (r.double() - t).abs().flatten()
    return (float(ek.max()), float(er.max()), float(torch.quantile(ek, 0.99)), float(torch.quantile(er, 0.99)))


def rule(k, r, t, label):
    """Print both errors and the ratios; return (ok, largest ratio)."""
    mk, mr, qk, qr = errors(k, r, t)
    rm = mk / mr if mr > 0 else (0.0 if mk == 0 else math.inf)
    rq = qk / qr if qr > 0 else (0.0 if qk == 0 else math.inf)
    print("rule %-44s max ours %.3g ref %.3g ratio %.2f | p99 ours %.3g ref %.3g ratio %.2f"
          % (label, mk, mr, rm, qk, qr, rq))
    return (mk <= FACTOR * mr and qk <= FACTOR * qr), max(rm, rq)


def assert_rule(k, r, t, label):
    ok, ratio = rule(k, r, t, label)
    assert ok, "%s: error %.2f x the fp32 reference's (allowed %.0f x)" % (label, ratio, FACTOR)
    return ratio


# ---------------------------------------------------------------------------
# nfk_wlin_pack on the CPU
def pack_exp(W):
    mx = float(W.abs().max()) if W.numel() else 0.0
    return (math.frexp(mx)[1] if mx > 0.0 else 0), mx  # mx < 2^ex


def split16(v):
    """fp32 -> (hi, lo) halfs: hi = f16(v), lo = f16(v - hi), both round to
    nearest even; the subtraction is exact in fp32."""
    hi = v.to(torch.float16)
    return hi, (v - hi.float()).to(torch.float16)


def wlin_pack_ref(W):
    """The pack of W [N, K] as (header fp32[64], body int16[NT, KB, 2, 64, 8], tail
    int16[1024]) -- the halfs as their bits."""
    N, K = W.shape
    NT, KB = cdiv(N, 16), cdiv(K, 32)
    ex, mx = pack_exp(W)
    Wp = torch.zeros(16 * NT, 32 * KB)
    Wp[:N, :K] = W * (2.0 ** (15 - ex))
    hi, lo = split16(Wp)
    # [nt][kb][part][lane = 16 (k / 8) + n][j]: element (16 nt + n, 32 kb + 8 (lane >> 4) + j)
    body = torch.stack([hi, lo]).view(2, NT, 16, KB, 4, 8).permute(1, 3, 0, 4, 2, 5).reshape(NT, KB, 2, 64, 8)
    hdr = torch.zeros(64)
    hdr[0], hdr[1] = 2.0 ** (ex - 15), min(mx, 3.0e38)
    return hdr, body.contiguous().view(torch.int16), torch.zeros(1024, dtype=torch.int16)


def pack_decode(pack, N, K):
    """A device pack as (header, body bits, tail bits) like wlin_pack_ref."""
    NT, KB = cdiv(N, 16), cdiv(K, 32)
    p = pack.detach().cpu()
    assert p.numel() == 64 + NT * KB * 512 + 512
    body = p[64:64 + NT * KB * 512].view(torch.int16).view(NT, KB, 2, 64, 8)
    return p[:64].clone(), body, p[64 + NT * KB * 512:].view(torch.int16)


# ---------------------------------------------------------------------------
# the kernel's arithmetic on the CPU
def _row_scale(v):
    """k_wl_rows: per row 2^(14 - e) with max|row| < 2^e (e >= -64; e = 0 for a zero row)."""
    mx = v.abs().amax(dim=1)
    ex = torch.where(mx > 0, torch.frexp(mx)[1], torch.zeros_like(mx, dtype=torch.int32)).clamp(min=-64)
    return torch.ldexp(torch.ones_like(mx), 14 - ex), torch.ldexp(torch.ones_like(mx), ex - 14)


def _frag(v, K32, drop_lo):
    hi, lo = split16(v)
    M, K = v.shape
    out = torch.zeros(2, M, K32, dtype=torch.float64)
    out[0, :, :K], out[1, :, :K] = hi.double(), (lo.double() * (0.0 if drop_lo else 1.0))
    return out


def _gemm(xf, W, fused, opt):
    """fp32 sums of (x hi/lo fragments) x (W as its pack)^T: per 32-wide
    k-block lo.hi + hi.lo + hi.hi, each block's exact sum added to an fp32
    accumulator; the chunks' accumulators added in order.  Returns the sums
    and the pack's 2^-s."""
    N, K = W.shape
    KB = cdiv(K, 32)
    ex, _ = pack_exp(W)
    wf = _frag(W * (2.0 ** (15 - ex)), 32 * KB, opt.get("drop_w_lo", False))
    M = xf.shape[1]
    X, Wt = xf.view(2, M, KB, 32), wf.view(2, N, KB, 32)
    prods = [torch.einsum("mkj,nkj->kmn", X[a], Wt[b]) for a, b in ((0, 1), (1, 0), (0, 0))]
    total = None
    skip = opt.get("skip_block")
    for k0, k1 in chunks(K, N, fused):
        # k_wl_gemm: the chunk's even k-blocks in one accumulator, the odd ones
        # negated in a second, the partial sum their difference; k_wl_gemm_act: one
        acc = [torch.zeros(M, N), torch.zeros(M, N)]
        for k in range(k0, k1):
            if skip is not None and k == min(skip, KB - 1):
                continue
            odd = 0 if fused else (k - k0) & 1
            for p in prods:
                acc[odd] = (acc[odd].double() + (-p[k] if odd else p[k])).float()
        acc = acc[0] - acc[1]
        total = acc if total is None else total + acc
    return total, 2.0 ** (ex - 15)


def _act(v, un, b, KBo, drop_lo):
    h = torch.tanh(v * un + b) * 16384.0
    return _frag(h, 32 * KBo, drop_lo)


def _rowsum(s):
    """k_wl_rows' sum of s over a row: thread t its columns t, t + 1024, ...
    in order, a 64-lane xor tree, then the 16 waves in order."""
    M, h = s.shape
    J = cdiv(h, 1024)
    sp = torch.zeros(M, J * 1024)
    sp[:, :h] = s
    sp = sp.view(M, J, 1024)
    v = torch.zeros(M, 1024)
    for j in range(J):
        v = v + sp[:, j]
    v = v.view(M, 16, 64)
    lane = torch.arange(64)
    for off in (32, 16, 8, 4, 2, 1):
        v = v + v[:, :, lane ^ off]
    tot = torch.zeros(M)
    for w in range(16):
        tot = tot + v[:, w, 0]
    return tot


def rnvp_split(x, Ws, bs, inverse, fused, **opt):
    """One layer as nfk_wide_rnvp.hip computes it (finite inputs): one 2^s per
    matrix (max|W| just under 2^15), per-row 2^e for x (2^14), tanh outputs
    x 2^14, fp16 hi/lo operands, three products per k-block in fp32
    accumulators (k_wl_gemm: two per chunk, even and negated odd k-blocks,
    subtracted), chunks (``fused``: the four waves of k_wl_gemm_act for L1
    and L2; else wl_plan's splits) added in order, fp32 bias / tanh, the
    coupling and its exp in double rounded once, log|det| in k_wl_rows' order.  ``opt``: drop_w_lo, drop_x_lo
    (an operand's lo half set to zero) and skip_block (k-block index left out
    of every stage) break it on purpose for the sensitivity checks."""
    x = x.float()
    h = x.shape[1] // 2
    H = Ws[0].shape[0]
    dx = opt.get("drop_x_lo", False)
    z = x.clone()
    ld = None
    cond = x[:, h:] if inverse else x[:, :h]
    for step in range(2):
        c = 1 - step if inverse else step
        sc, un = _row_scale(cond)
        xf = _frag(cond * sc[:, None], 32 * cdiv(h, 32), dx)
        outs = []
        for g in range(2):
            W1, W2, W3 = (Ws[6 * c + 2 * l + g] for l in range(3))
            b1, b2, b3 = (bs[6 * c + 2 * l + g] for l in range(3))
            v, u = _gemm(xf, W1, fused, opt)
            f = _act(v, (u * un)[:, None], b1, cdiv(H, 32), dx)
            v, u = _gemm(f, W2, fused, opt)
            f = _act(v, torch.tensor(u / 16384.0), b2, cdiv(H, 32), dx)
            v, u = _gemm(f, W3, False, opt)
            outs.append(v * torch.tensor(u / 16384.0) + b3)
        s, t = outs
        col = slice(h, 2 * h) if c == 0 else slice(0, h)
        xin = x[:, col]
        xd, sd, td = xin.double(), s.double(), t.double()
        o = ((xd - td) * torch.exp(-sd) if inverse else td + xd * torch.exp(sd)).float()
        z[:, col] = o
        tot = _rowsum(s)
        tot = -tot if inverse else tot
        ld = tot if ld is None else ld + tot
        cond = o
    return z, ld
