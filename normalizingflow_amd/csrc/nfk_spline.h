// nfk_spline.h -- per-element rational-quadratic spline math for gfx950.
//
// One lane evaluates one (sample, coordinate) element entirely in registers:
// no host syncs, no compaction.  The fp32 operation order follows the
// reference (nf/utils.py:58-152, nf/flows.py:233-235) so results track the
// PyTorch-CPU path to ulp level:
//   * softmax = exp(u - max) / sequential sum, applied as * (1/sum);
//   * cumsum of the floored bin fractions accumulated in double and rounded
//     per prefix (what ATen's CPU cumsum does for fp32);
//   * separate roundings everywhere (files are built with -ffp-contract=off).
// Host-side constants (NfkSplineConst) are evaluated in double exactly as the
// Python scalars of the reference are, then rounded to fp32 once.
#pragma once

#include <hip/hip_runtime.h>

#include <stdint.h>

struct NfkSplineConst {
    float scale2b;   // (float)(right-left) = (float)(2*B): NSF_CL's W,H <- 2B*softmax (flows.py:234)
    float lo, hi;    // (float)left, (float)right: knot range in x and the tails' inside test
    float span;      // (float)(right - left)
    float ylo, yhi;  // (float)bottom, (float)top
    float yspan;     // (float)(top - bottom)
    int tails;       // 1: identity outside [left, right] (unconstrained_RQS)
    float min_w, fw; // (float)min_bin_width, (float)(1 - min_bin_width*K)
    float min_h, fh; // same for heights
    float min_d;     // (float)min_derivative
    float dpad;      // (float)log(exp(1 - min_derivative) - 1) (utils.py:37)
    float knot_eps;  // 1e-6f (utils.py:20)
    float m2b;       // (float)((right-left) * log2(e)): lean knots' second-softmax multiplier
    float d_edge;    // min_d + softplus(dpad) in fp32: the boundary derivative (utils.py:36-39, 82)
};

__device__ __forceinline__ float nfk_softplus(float v) {
    // torch.nn.functional.softplus(beta=1, threshold=20)
    return v > 20.0f ? v : log1pf(expf(v));
}

// ---------------------------------------------------------------------------
// Short-sequence transcendentals for the fused kernel's epilogue, where fp32
// MFMA and VALU share one datapath and every VALU instruction costs MFMA time.
// exp: 2^(x*log2e) with the product's rounding error carried (hi/lo split of
//      log2e + exact fma residual) and folded back with one fma: ~1-2 ulp.
// rcp/div: v_rcp_f32 + one Newton step (+ residual correction for a/b):
//      correctly rounded except in rare near-tie cases.
// log: v_log_f32 (log2) times ln2 split hi/lo.
// No special-value handling: inputs are finite by construction here.
__device__ __forceinline__ float nfk_exp_fast(float x) {
    const float L2E = 1.44269502e+00f, L2E_LO = 1.92596299e-08f;  // log2(e) = L2E + L2E_LO
    const float t = x * L2E;
    const float r = __builtin_fmaf(x, L2E_LO, __builtin_fmaf(x, L2E, -t));
    const float e = __builtin_amdgcn_exp2f(t);
    return __builtin_fmaf(e, r * 0.693147182f, e);
}

__device__ __forceinline__ float nfk_rcp_fast(float b) {
    const float r = __builtin_amdgcn_rcpf(b);
    return __builtin_fmaf(r, __builtin_fmaf(-b, r, 1.0f), r);
}

__device__ __forceinline__ float nfk_div_fast(float a, float b) {
    const float r = nfk_rcp_fast(b);
    const float q = a * r;
    return __builtin_fmaf(r, __builtin_fmaf(-b, q, a), q);
}

__device__ __forceinline__ float nfk_log_fast(float x) {
    const float LN2 = 6.93147182e-01f, LN2_LO = -1.90465421e-09f;
    const float l2 = __builtin_amdgcn_logf(x);
    return __builtin_fmaf(l2, LN2_LO, l2 * LN2);
}

__device__ __forceinline__ float nfk_softplus_fast(float v) {
    return v > 20.0f ? v : nfk_log_fast(1.0f + nfk_exp_fast(v));
}

// ---------------------------------------------------------------------------
// Lean epilogue math for the fused layer kernel.  Every VALU instruction there
// costs MFMA time, so these trade the reference's exact operation order for
// short sequences whose ABSOLUTE error stays at the few-ulp level that the
// downstream consumers (linear layers, cumulative knots) are sensitive to.
constexpr float kL2E = 1.44269502e+00f;  // log2(e)
constexpr float kLN2 = 6.93147182e-01f;

// softplus (threshold 20, like torch) as log2(1 + 2^(v log2e)) ln2.
__device__ __forceinline__ float nfk_softplus_lean(float v) {
    const float s = __builtin_amdgcn_logf(1.0f + __builtin_amdgcn_exp2f(v * kL2E)) * kLN2;
    return v > 20.0f ? v : s;
}

// Knots of one element from its K raw NSF_CL conditioner logits:
//   W <- 2B softmax(raw)                 (flows.py:233-234)
//   w <- softmax(W); w <- min + (1 - min K) w; cw <- span cumsum(w) + lo
//                                        (utils.py:73-80, 84-91)
// Both softmaxes are evaluated as 2^(fma(u, log2e, -shift)): softmax is
// shift-invariant, so the rounding of the shift cancels.  The first uses the
// max logit as shift; the second the known bound 2B of its inputs (2B softmax
// lies in [0, 2B]) with the 1/sum folded into the exponent's multiplier,
// m2b = 2B log2e.  The cumsum is still accumulated in double.
// edge[0] = lo, edge[K] = hi are pinned like utils.py:78-79.
// l2e = log2(e) times any power-of-two scale the logits still carry.
template <int K>
__device__ __forceinline__ void nfk_knots_nsf_lean(const float (&raw)[K], float l2e, float lo, float hi,
                                                   float span, float min_b, float fb, float m2b,
                                                   float (&edge)[K + 1]) {
    float m = raw[0];
#pragma unroll
    for (int i = 1; i < K; ++i) m = fmaxf(m, raw[i]);
    const float mL = m * l2e;
    float e[K];
    float s = 0.0f;
#pragma unroll
    for (int i = 0; i < K; ++i) {
        e[i] = __builtin_amdgcn_exp2f(__builtin_fmaf(raw[i], l2e, -mL));
        s = i == 0 ? e[0] : s + e[i];
    }
    const float q = m2b * __builtin_amdgcn_rcpf(s);
    float s2 = 0.0f;
#pragma unroll
    for (int i = 0; i < K; ++i) {
        e[i] = __builtin_amdgcn_exp2f(__builtin_fmaf(e[i], q, -m2b));
        s2 = i == 0 ? e[0] : s2 + e[i];
    }
    // cumsum of the floored fractions in 2^-30 fixed point: every fraction is
    // >= min_b (~2^-10) so the truncation to 2^-30 loses < 2^-20 of it, the
    // int32 prefix sums are exact (total < 2^30), and each prefix is rounded
    // to fp32 once -- the double-accumulated cumsum of ATen without f64 ops.
    const float f30 = (fb * 1073741824.0f) * __builtin_amdgcn_rcpf(s2);
    const float mb30 = min_b * 1073741824.0f;
    const float sp30 = span * (1.0f / 1073741824.0f);
    int acc = 0;
    edge[0] = lo;
#pragma unroll
    for (int i = 0; i < K - 1; ++i) {
        acc += (int)__builtin_fmaf(e[i], f30, mb30);
        edge[i + 1] = __builtin_fmaf(sp30, (float)acc, lo);
    }
    edge[K] = hi;
}

// Same knots kept as 2^-30 fixed-point prefix sums: pre[j] = sum_{i<j} of
// the floored fractions (pre[0] = 0); edge j = fma(span 2^-30, (float)pre[j], lo)
// for j < K and the pinned right end for j = K.  The fused kernel searches
// the bin in this integer domain and converts only the two edges it uses.
// sum of K values, sequential (tried: a pairwise tree for shorter dependency
// chains, c3 6.28/6.30 vs 6.28/6.28 ms per chain: DESIGN.md section 6)
template <int K>
__device__ __forceinline__ float nfk_sum(const float (&v)[K]) {
    float s = v[0];
#pragma unroll
    for (int i = 1; i < K; ++i) s = s + v[i];
    return s;
}

// Returns the second softmax's sum s2 (in [1, K] for finite logits, NaN if a
// logit is NaN): the integer prefixes cannot carry a NaN, so callers place the
// knot edges at fma(s2, 0, lo) + ..., which is lo exactly unless the logits
// were NaN -- then the edges, and everything the reference computes from its
// NaN cumsum (utils.py:73-91), are NaN too.
// max of K logits as a tree of three-input v_max3_f32 (inline asm): written with
// fmaxf, hipcc first quiets every input (v_max_f32 x, x: IEEE mode's signalling
// NaNs), about one instruction more per two inputs.  The logits are MFMA results,
// never signalling NaNs, and a quiet NaN input leaves the max at the other
// values in both forms (the exps of the NaN logit make the knots NaN).
__device__ __forceinline__ float nfk_max3(float a, float b, float c) {
    float r;
    asm("v_max3_f32 %0, %1, %2, %3" : "=v"(r) : "v"(a), "v"(b), "v"(c));
    return r;
}
__device__ __forceinline__ float nfk_max2(float a, float b) {
    float r;
    asm("v_max_f32 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
    return r;
}
template <int K>
__device__ __forceinline__ float nfk_max_lean(const float (&raw)[K]) {
    float t[K];
#pragma unroll
    for (int i = 0; i < K; ++i) t[i] = raw[i];
    int n = K;
#pragma unroll
    for (int pass = 0; pass < 8 && n > 1; ++pass) {  // (constant-folded: K is a template argument)
        int w = 0;
#pragma unroll
        for (int i = 0; i < K; i += 3) {
            if (i >= n) break;
            t[w++] = (i + 2 < n) ? nfk_max3(t[i], t[i + 1], t[i + 2]) : (i + 1 < n ? nfk_max2(t[i], t[i + 1]) : t[i]);
        }
        n = w;
    }
    return t[0];
}

template <int K>
__device__ __forceinline__ float nfk_prefix_nsf_lean(const float (&raw)[K], float l2e, float m2b,
                                                     float fb30, float mb30, int (&pre)[K]) {
    const float m = nfk_max_lean<K>(raw);
    const float mL = m * l2e;
    float e[K];
#pragma unroll
    for (int i = 0; i < K; ++i) e[i] = __builtin_amdgcn_exp2f(__builtin_fmaf(raw[i], l2e, -mL));
    const float q = m2b * __builtin_amdgcn_rcpf(nfk_sum<K>(e));
#pragma unroll
    for (int i = 0; i < K; ++i) e[i] = __builtin_amdgcn_exp2f(__builtin_fmaf(e[i], q, -m2b));
    const float s2 = nfk_sum<K>(e);
    const float f30 = fb30 * __builtin_amdgcn_rcpf(s2);
    pre[0] = 0;
#pragma unroll
    for (int i = 0; i < K - 1; ++i) pre[i + 1] = pre[i] + (int)__builtin_fmaf(e[i], f30, mb30);
    return s2;
}

// The same double softmax kept in float: E[j] = sum_{i<j} of the second
// softmax's terms (E[0] = 0), the partial sums the sequential nfk_sum forms on
// its way to s2 = E[K-1] + e[K-1], which is returned -- one chain of K - 1
// adds gives the cumsum and the sum.  Knot j of the normalised range [0, 1] is
// fma(E[j], fb / s2, j min_bin); no integer conversion.  A NaN logit makes
// every E[j], j >= 1, and s2 NaN, so the knots carry it themselves.
// Knot error against fp64 (tools/knot_forms.py): no larger than the fixed-point
// form's; the exps dominate it, not the cumsum.
template <int K>
__device__ __forceinline__ float nfk_partials_nsf_lean(const float (&raw)[K], float l2e, float m2b,
                                                       float (&E)[K]) {
    const float m = nfk_max_lean<K>(raw);
    const float mL = m * l2e;
    float e[K];
#pragma unroll
    for (int i = 0; i < K; ++i) e[i] = __builtin_amdgcn_exp2f(__builtin_fmaf(raw[i], l2e, -mL));
    const float q = m2b * __builtin_amdgcn_rcpf(nfk_sum<K>(e));
#pragma unroll
    for (int i = 0; i < K; ++i) e[i] = __builtin_amdgcn_exp2f(__builtin_fmaf(e[i], q, -m2b));
    E[0] = 0.0f;
    float s = e[0];
#pragma unroll
    for (int i = 1; i < K; ++i) {
        E[i] = s;
        s = s + e[i];
    }
    return s;
}

// nfk_prefix_nsf_lean for two coordinates at once: the fp32 FMAs, multiplies
// and sums run as packed pairs (v_pk_fma_f32 / v_pk_mul_f32 / v_pk_add_f32,
// two lanes' worth of work per VALU instruction); max, exp2, rcp and the
// integer conversion stay scalar.  Every operation is the scalar one applied
// per component, in the same order, so pre0/pre1 are bitwise those of two
// nfk_prefix_nsf_lean calls.
typedef float nfk_f2 __attribute__((ext_vector_type(2)));
template <int K>
__device__ __forceinline__ nfk_f2 nfk_sum2(const nfk_f2 (&v)[K]) {
    nfk_f2 s = v[0];
#pragma unroll
    for (int i = 1; i < K; ++i) s = s + v[i];
    return s;
}

template <int K>
__device__ __forceinline__ nfk_f2 nfk_prefix_nsf_lean2(const float (&raw0)[K], const float (&raw1)[K], float l2e,
                                                       float m2b, float fb30, float mb30, int (&pre0)[K],
                                                       int (&pre1)[K]) {
    float m0 = raw0[0], m1 = raw1[0];
#pragma unroll
    for (int i = 1; i < K; ++i) {
        m0 = fmaxf(m0, raw0[i]);
        m1 = fmaxf(m1, raw1[i]);
    }
    const nfk_f2 l2 = {l2e, l2e};
    const nfk_f2 mL = nfk_f2{m0, m1} * l2;
    nfk_f2 e[K];
#pragma unroll
    for (int i = 0; i < K; ++i) {
        const nfk_f2 a = __builtin_elementwise_fma(nfk_f2{raw0[i], raw1[i]}, l2, -mL);
        e[i] = nfk_f2{__builtin_amdgcn_exp2f(a.x), __builtin_amdgcn_exp2f(a.y)};
    }
    const nfk_f2 s1 = nfk_sum2<K>(e);
    const nfk_f2 mb = {m2b, m2b};
    const nfk_f2 q = mb * nfk_f2{__builtin_amdgcn_rcpf(s1.x), __builtin_amdgcn_rcpf(s1.y)};
#pragma unroll
    for (int i = 0; i < K; ++i) {
        const nfk_f2 a = __builtin_elementwise_fma(e[i], q, -mb);
        e[i] = nfk_f2{__builtin_amdgcn_exp2f(a.x), __builtin_amdgcn_exp2f(a.y)};
    }
    const nfk_f2 s2 = nfk_sum2<K>(e);
    const nfk_f2 f30 = nfk_f2{fb30, fb30} * nfk_f2{__builtin_amdgcn_rcpf(s2.x), __builtin_amdgcn_rcpf(s2.y)};
    const nfk_f2 mb30v = {mb30, mb30};
    pre0[0] = 0;
    pre1[0] = 0;
#pragma unroll
    for (int i = 0; i < K - 1; ++i) {
        const nfk_f2 f = __builtin_elementwise_fma(e[i], f30, mb30v);
        pre0[i + 1] = pre0[i] + (int)f.x;
        pre1[i + 1] = pre1[i] + (int)f.y;
    }
    return s2;
}

// min_d + softplus(softplus(v)) of NSF_CL + RQS (flows.py:235, utils.py:82) in
// one step: e^softplus(v) = 1 + e^v, so softplus(softplus(v)) = log(2 + e^v);
// torch's threshold 20 passes v through both softplus calls unchanged.
// raw * sl2e = v log2(e) with v the derivative logit (sl2e = log2(e) times any
// power-of-two scale raw still carries): min_d + softplus(softplus(v)) as
// min_d + ln2 * (v log2e > 20 log2e ? v log2e : log2(2 + 2^(v log2e))), the
// final multiply and add one fma (7 VALU; the round-4 form took 9)
__device__ __forceinline__ float nfk_deriv_lean_s(float raw, float sl2e, float min_d) {
    const float a = raw * sl2e;
    const float t = __builtin_amdgcn_logf(2.0f + __builtin_amdgcn_exp2f(a));
    return __builtin_fmaf(a > 20.0f * kL2E ? a : t, kLN2, min_d);
}
__device__ __forceinline__ float nfk_deriv_lean(float v, float min_d) { return nfk_deriv_lean_s(v, kL2E, min_d); }

template <bool FAST>
__device__ __forceinline__ float nfk_exp(float x) { return FAST ? nfk_exp_fast(x) : expf(x); }
template <bool FAST>
__device__ __forceinline__ float nfk_log(float x) { return FAST ? nfk_log_fast(x) : logf(x); }
template <bool FAST>
__device__ __forceinline__ float nfk_div(float a, float b) { return FAST ? nfk_div_fast(a, b) : a / b; }
template <bool FAST>
__device__ __forceinline__ float nfk_splus(float v) { return FAST ? nfk_softplus_fast(v) : nfk_softplus(v); }

// softmax over K logits, in place (K compile-time so the arrays stay in VGPRs).
// Summation order of ATen's CPU kernel (vec::reduce_all, AVX-512 build the
// golden vectors come from): sequential for K < 16; for K >= 16 the K values
// are folded onto 16 lanes (lane i += x[i + 16m]) and reduced by the
// xor-8/4/2/1 butterfly.  Output = e * (1/sum).
template <int K, bool FAST = false>
__device__ __forceinline__ void nfk_softmax(float (&u)[K]) {
    float m = u[0];
#pragma unroll
    for (int i = 1; i < K; ++i) m = fmaxf(m, u[i]);
#pragma unroll
    for (int i = 0; i < K; ++i) u[i] = nfk_exp<FAST>(u[i] - m);
    float s;
    if constexpr (K < 16) {
        s = 0.0f;
#pragma unroll
        for (int i = 0; i < K; ++i) s = s + u[i];
    } else {
        float v[16];
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            v[i] = u[i];
#pragma unroll
            for (int j = i + 16; j < K; j += 16) v[i] = v[i] + u[j];
        }
#pragma unroll
        for (int i = 0; i < 8; ++i) v[i] = v[i] + v[i + 8];
#pragma unroll
        for (int i = 0; i < 4; ++i) v[i] = v[i] + v[i + 4];
#pragma unroll
        for (int i = 0; i < 2; ++i) v[i] = v[i] + v[i + 2];
        s = v[0] + v[1];
    }
    const float r = FAST ? nfk_rcp_fast(s) : 1.0f / s;
#pragma unroll
    for (int i = 0; i < K; ++i) u[i] = u[i] * r;
}

// Knot positions from unnormalised logits (utils.py:73-80 / 84-91):
// edge[0..K]; edge[0] = lo, edge[K] = hi pinned.
template <int K, bool FAST = false>
__device__ __forceinline__ void nfk_knots(float (&u)[K], float lo, float hi, float span,
                                          float min_b, float fb, float (&edge)[K + 1]) {
    nfk_softmax<K, FAST>(u);
    double acc = 0.0;
    edge[0] = lo;
#pragma unroll
    for (int i = 0; i < K; ++i) {
        const float p = min_b + fb * u[i];
        acc += (double)p;
        edge[i + 1] = span * (float)acc + lo;
    }
    edge[K] = hi;
}

// Bin index: #{j : v >= edge'[j]} - 1 with edge'[K] = edge[K] + eps (utils.py:20-25),
// clamped to [0, K-1].  Returns the selected (edge_k, size_k).
template <int K>
__device__ __forceinline__ int nfk_bin(const float (&edge)[K + 1], float v, float eps) {
    int c = 0;
#pragma unroll
    for (int j = 0; j < K; ++j) c += (v >= edge[j]) ? 1 : 0;
    c += (v >= edge[K] + eps) ? 1 : 0;
    int k = c - 1;
    k = k < 0 ? 0 : k;
    k = k > K - 1 ? K - 1 : k;
    return k;
}

template <int K>
__device__ __forceinline__ float nfk_sel(const float (&a)[K], int k) {
    // register-resident select (no dynamic indexing -> no scratch)
    float r = a[0];
#pragma unroll
    for (int j = 1; j < K; ++j) r = (k == j) ? a[j] : r;
    return r;
}

// number of derivative logits per element: K-1 interior ones (the two
// boundary ones are the constant dpad, utils.py:36-39), or all K+1 (DFULL,
// the bare RQS of utils.py:58)
template <int K, bool DFULL>
struct NfkDN {
    static constexpr int n = DFULL ? K + 1 : (K - 1 > 0 ? K - 1 : 1);
};

// Evaluate one spline element.  wr/hr: K logits each, dr: derivative logits
// (before NSF_CL pre-normalisation when PRE == true).
// out/lad: transformed value and log|det| (identity, 0 outside [-B, B]).
template <int K, bool INV, bool PRE, bool DFULL>
__device__ __forceinline__ void nfk_rqs_element(float x, float (&wr)[K], float (&hr)[K],
                                                const float (&dr)[NfkDN<K, DFULL>::n],
                                                const NfkSplineConst& c, float& out, float& lad,
                                                bool& inside, bool& neg_disc) {
    inside = !c.tails || ((x >= c.lo) && (x <= c.hi));
    neg_disc = false;
    if (!inside) {
        out = x;
        lad = 0.0f;
        return;
    }
    if (PRE) {
        nfk_softmax<K>(wr);
        nfk_softmax<K>(hr);
#pragma unroll
        for (int i = 0; i < K; ++i) {
            wr[i] = c.scale2b * wr[i];
            hr[i] = c.scale2b * hr[i];
        }
    }
    float cw[K + 1], ch[K + 1];
    nfk_knots<K>(wr, c.lo, c.hi, c.span, c.min_w, c.fw, cw);
    nfk_knots<K>(hr, c.ylo, c.yhi, c.yspan, c.min_h, c.fh, ch);

    const int k = nfk_bin<K>(INV ? ch : cw, x, c.knot_eps);
    // gather (utils.py:98-109) without dynamic register indexing
    float cw_k = cw[0], w_k = cw[1] - cw[0], ch_k = ch[0], h_k = ch[1] - ch[0];
#pragma unroll
    for (int j = 1; j < K; ++j) {
        if (k == j) {
            cw_k = cw[j];
            w_k = cw[j + 1] - cw[j];
            ch_k = ch[j];
            h_k = ch[j + 1] - ch[j];
        }
    }
    // derivatives: padded logits [dpad, d_0..d_{K-2}, dpad] -> min_d + softplus(.)
    // only the two that the bin uses are evaluated (utils.py:82, 105-107)
    float raw_k = 0.0f, raw_k1 = 0.0f;
    if (DFULL) {
        raw_k = dr[0];
        raw_k1 = dr[1];
#pragma unroll
        for (int j = 1; j < K; ++j) {
            if (k == j) {
                raw_k = dr[j];
                raw_k1 = dr[j + 1];
            }
        }
    } else {
#pragma unroll
        for (int j = 0; j < K - 1; ++j) {
            if (k == j + 1) raw_k = dr[j];  // padded index j+1 holds logit j
            if (k == j) raw_k1 = dr[j];
        }
        if (PRE) {  // NSF_CL's D <- softplus(D) (flows.py:235), only where it is used
            raw_k = nfk_softplus(raw_k);
            raw_k1 = nfk_softplus(raw_k1);
        }
        raw_k = (k == 0) ? c.dpad : raw_k;
        raw_k1 = (k == K - 1) ? c.dpad : raw_k1;
    }
    const float d_k = c.min_d + nfk_softplus(raw_k);
    const float d_k1 = c.min_d + nfk_softplus(raw_k1);
    const float delta = h_k / w_k;
    const float gap = (d_k + d_k1) - 2.0f * delta;

    float th;
    if (INV) {
        const float y = x - ch_k;
        const float qa = y * gap + h_k * (delta - d_k);
        const float qb = h_k * d_k - y * gap;
        const float qc = (-delta) * y;
        const float disc = qb * qb - (4.0f * qa) * qc;
        neg_disc = !(disc >= 0.0f);
        const float root = (2.0f * qc) / (-qb - sqrtf(disc));
        out = root * w_k + cw_k;
        th = root;
    } else {
        th = (x - cw_k) / w_k;
    }
    const float t1mt = th * (1.0f - th);
    const float den = delta + gap * t1mt;
    if (!INV) {
        const float num = h_k * (delta * (th * th) + d_k * t1mt);
        out = ch_k + num / den;
    }
    const float omt = 1.0f - th;
    const float dnum = (delta * delta) * ((d_k1 * (th * th) + (2.0f * delta) * t1mt) + d_k * (omt * omt));
    const float l = logf(dnum) - 2.0f * logf(den);
    lad = INV ? -l : l;
}

// Lean NSF_CL element (PRE: raw conditioner logits) for the streaming kernel:
// the fused kernel's epilogue math (nfk_prefix_nsf_lean knots in 2^-30 fixed
// point, integer bin search, softplus(softplus) identity, fast reciprocals;
// nfk_fused_impl.h knot_phase / epilogue C) on one element held by one lane.
// Valid for NSF_CL's constants: x and y knot ranges equal, min bin width =
// height (the host checks).  Absolute error at the few-ulp level; an element
// within an ulp of a knot may take the neighbouring bin, where the C1 spline
// agrees.
template <int K>
__device__ __forceinline__ void nfk_lean_bin_edges(const int (&pre)[K], int k, const NfkSplineConst& c,
                                                   float sp30, float s2, float& e0, float& sz) {
    const float lo = __builtin_fmaf(s2, 0.0f, c.lo);  // NaN iff the logits were (nfk_prefix_nsf_lean)
    int p0 = 0, p1 = pre[1 < K ? 1 : 0];
#pragma unroll
    for (int j = 1; j < K; ++j) {
        const bool ge = k >= j;
        p0 = ge ? pre[j] : p0;
        if (j + 1 < K) p1 = ge ? pre[j + 1] : p1;
    }
    e0 = __builtin_fmaf(sp30, (float)p0, lo);
    const float e1 = (k == K - 1) ? c.hi : __builtin_fmaf(sp30, (float)p1, lo);
    sz = e1 - e0;
}

template <int K, bool INV>
__device__ __forceinline__ void nfk_rqs_element_lean(float x, const float (&wr)[K], const float (&hr)[K],
                                                     const float (&dr)[K - 1 > 0 ? K - 1 : 1],
                                                     const NfkSplineConst& c, float& out, float& lad,
                                                     bool& inside, bool& neg_disc) {
    inside = !c.tails || ((x >= c.lo) && (x <= c.hi));
    neg_disc = false;
    const float two30 = 1073741824.0f;
    const float sp30 = c.span * (1.0f / two30), inv30 = two30 / c.span;
    const float fb30 = c.fw * two30, mb30 = c.min_w * two30;
    int pw[K], ph[K];
    const float sw = nfk_prefix_nsf_lean<K>(wr, kL2E, c.m2b, fb30, mb30, pw);
    const float sh = nfk_prefix_nsf_lean<K>(hr, kL2E, c.m2b, fb30, mb30, ph);
    const int xi = __float2int_rd(__builtin_fmaf(x, inv30, -c.lo * inv30));
    int k = 0;
#pragma unroll
    for (int j = 1; j < K; ++j) k += (xi >= (INV ? ph[j] : pw[j])) ? 1 : 0;
    float cw_k, w_k, ch_k, h_k;
    nfk_lean_bin_edges<K>(pw, k, c, sp30, sw, cw_k, w_k);
    nfk_lean_bin_edges<K>(ph, k, c, sp30, sh, ch_k, h_k);
    // padded derivative index j+1 holds logit j (utils.py:36-39)
    float raw_k = dr[0], raw_k1 = dr[0];
#pragma unroll
    for (int j = 1; j < K - 1; ++j) {
        raw_k = (k >= j + 1) ? dr[j] : raw_k;
        raw_k1 = (k >= j) ? dr[j] : raw_k1;
    }
    const float d_k = (k == 0) ? c.d_edge : nfk_deriv_lean(raw_k, c.min_d);
    const float d_k1 = (k == K - 1) ? c.d_edge : nfk_deriv_lean(raw_k1, c.min_d);
    const float rw = nfk_rcp_fast(w_k);
    const float delta = h_k * rw;
    const float gap = (d_k + d_k1) - 2.0f * delta;
    float th;
    if (INV) {
        const float y = x - ch_k;
        const float qa = y * gap + h_k * (delta - d_k);
        const float qb = h_k * d_k - y * gap;
        const float qc = (-delta) * y;
        const float disc = qb * qb - (4.0f * qa) * qc;
        neg_disc = inside && !(disc >= 0.0f);
        const float root = nfk_div_fast(2.0f * qc, -qb - sqrtf(disc));
        out = root * w_k + cw_k;
        th = root;
    } else {
        th = (x - cw_k) * rw;
    }
    const float t1mt = th * (1.0f - th);
    const float den = delta + gap * t1mt;
    if (!INV) {
        const float num = h_k * (delta * (th * th) + d_k * t1mt);
        out = ch_k + nfk_div_fast(num, den);
    }
    const float omt = 1.0f - th;
    const float dnum = (delta * delta) * ((d_k1 * (th * th) + (2.0f * delta) * t1mt) + d_k * (omt * omt));
    const float l = (__builtin_amdgcn_logf(dnum) - 2.0f * __builtin_amdgcn_logf(den)) * kLN2;
    lad = inside ? (INV ? -l : l) : 0.0f;
    out = inside ? out : x;
}
