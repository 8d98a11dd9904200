#!/usr/bin/env python
"""fp32 emulation of the two knot forms of the fused NSF epilogue (numpy, CPU).

Both forms share the double softmax of nfk_spline.h (max shift, exp2 with the
first 1/sum folded into the second exponent) and differ in the cumsum:

  fixed   nfk_prefix_nsf_lean: every floored fraction truncated to 2^-30 fixed
          point, exact int32 prefix sums, one convert back per knot;
  float   nfk_partials_nsf_lean + knot_phase: the sequential partial sums E_j
          of the second softmax's terms, knot j = lo + span fma(E_j, fb / s2,
          j min_bin).

Every fp32 operation is emulated as the float32 rounding of its float64
value (an fma is one rounding of the exact product-sum, exact in float64 for
these magnitudes up to double rounding); exp2 and the reciprocal are numpy's
float32 ones, so the hardware's extra ulp of v_exp_f32 / v_rcp_f32 -- the same
in both forms -- is not modelled.  The truth is the float64 evaluation of the
reference formula (nf/flows.py:233-236, nf/utils.py:73-91).

    python tools/knot_forms.py [sets]      # the table of DESIGN.md section 6
"""
import sys

import numpy as np

F = np.float32
L2E = F(1.4426950408889634)
TWO30 = F(1073741824.0)


def _fma(a, b, c):
    return (a.astype(np.float64) * np.float64(b) + np.float64(c)).astype(F)


def _seq_partials(e):
    """Sequential fp32 partial sums: P[:, j] = e_0 + ... + e_{j-1}, j = 0..K."""
    n, K = e.shape
    P = np.zeros((n, K + 1), F)
    P[:, 1] = e[:, 0]
    for i in range(1, K):
        P[:, i + 1] = P[:, i] + e[:, i]
    return P


def softmax_terms(raw, B):
    """Terms of the second softmax, as both device forms compute them."""
    m2b = F(2.0 * B) * L2E
    m = raw.max(axis=1, keepdims=True)
    mL = m * L2E
    e = np.exp2(_fma(raw, L2E, -mL))
    s1 = _seq_partials(e)[:, -1:]
    q = m2b * (F(1.0) / s1)
    return np.exp2(_fma(e, q, -m2b))


def edges_fixed(raw, B=3.0, min_bin=1e-3):
    """K + 1 edges of the fixed-point form (right end pinned)."""
    n, K = raw.shape
    lo, hi, span = F(-B), F(B), F(2.0 * B)
    fb30 = F(F(1.0) - F(min_bin) * F(K)) * TWO30
    mb30 = F(min_bin) * TWO30
    sp30 = span / TWO30
    e = softmax_terms(raw, B)
    s2 = _seq_partials(e)[:, -1:]
    f30 = fb30 * (F(1.0) / s2)
    inc = np.trunc((e.astype(np.float64) * f30 + np.float64(mb30)).astype(F)).astype(np.int64)
    pre = np.concatenate([np.zeros((n, 1), np.int64), np.cumsum(inc[:, :K - 1], axis=1)], axis=1)
    edge = _fma(pre.astype(F), sp30, lo)
    return np.concatenate([edge, np.full((n, 1), hi, F)], axis=1)


def edges_float(raw, B=3.0, min_bin=1e-3):
    """K + 1 edges of the float partial-sum form (right end pinned)."""
    n, K = raw.shape
    lo, hi, span = F(-B), F(B), F(2.0 * B)
    fb = F(F(1.0) - F(min_bin) * F(K))
    e = softmax_terms(raw, B)
    P = _seq_partials(e)
    f = fb * (F(1.0) / P[:, -1:])
    jm = (np.arange(K, dtype=F) * F(min_bin)).astype(F)
    t = (P[:, :K].astype(np.float64) * f + jm.astype(np.float64)).astype(F)
    t[:, 0] = F(0.0)
    edge = _fma(t, span, lo)
    return np.concatenate([edge, np.full((n, 1), hi, F)], axis=1)


def edges_f64(raw, B=3.0, min_bin=1e-3):
    """The reference formula in float64 on the same fp32 logits."""
    r = raw.astype(np.float64)
    K = r.shape[1]

    def sm(v):
        z = np.exp(v - v.max(axis=1, keepdims=True))
        return z / z.sum(axis=1, keepdims=True)

    w = sm(2.0 * B * sm(r))
    w = min_bin + (1.0 - min_bin * K) * w
    edge = 2.0 * B * np.concatenate([np.zeros((len(r), 1)), np.cumsum(w, axis=1)], axis=1) - B
    edge[:, 0], edge[:, -1] = -B, B
    return edge


def knot_errors(sigma, sets, seed, K=8, B=3.0):
    """{form: (max, p99, mean)} interior-knot error vs float64, and whether
    every edge sequence of each form is strictly increasing."""
    raw = (np.random.default_rng(seed).standard_normal((sets, K)) * sigma).astype(F)
    truth = edges_f64(raw, B)
    out, mono = {}, {}
    for name, fn in (("fixed", edges_fixed), ("float", edges_float)):
        ed = fn(raw, B)
        err = np.abs(ed[:, 1:K].astype(np.float64) - truth[:, 1:K])
        out[name] = (float(err.max()), float(np.quantile(err, 0.99)), float(err.mean()))
        mono[name] = bool((np.diff(ed.astype(np.float64), axis=1) > 0).all())
    return out, mono


def main():
    sets = int(sys.argv[1]) if len(sys.argv) > 1 else 400000
    for sigma in (0.3, 1.0, 3.0):
        err, mono = knot_errors(sigma, sets, seed=17)
        print("sigma %.1f: " % sigma + "; ".join(
            "%s %.3g / %.3g / %.3g%s" % ((k,) + err[k] + ("" if mono[k] else " NOT MONOTONE",)) for k in err))


if __name__ == "__main__":
    main()
