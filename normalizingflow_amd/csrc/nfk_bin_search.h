// nfk_bin_search.h -- the bin of a value among the knots of a spline's
// normalised range: the number of interior knots t[1 .. K-1] that are <= x
// (utils.py:20-25's searchsorted over the cumulative widths or heights).
// Host and device: knot_phase (nfk_fused_impl.h) searches with it, the host
// helper exports both forms so the CPU suite can compare them.
#pragma once

#if defined(__HIPCC__)
#define NFK_HD __host__ __device__ __forceinline__
#else
#define NFK_HD inline
#endif

// The counting form: K - 1 compares, one add each.  t[0] is not read.
template <int K>
NFK_HD int nfk_bin_count(float xn, const float (&t)[K]) {
    int k = 0;
#pragma unroll
    for (int j = 1; j < K; ++j) k += (xn >= t[j]) ? 1 : 0;
    return k;
}

// K = 8 by bisection: three compares decide the bin when t[1 .. 7] is
// non-decreasing (knot_phase: t[j] = fma(E[j], f, j min_bin) with E the
// partial sums of positive terms and f >= 0, and a correctly rounded fma is
// monotone in each argument).  Equal to nfk_bin_count<8> for every such t:
// xn >= t[4] implies xn >= t[1 .. 3], xn < t[4] implies xn < t[5 .. 7], and so
// on down.  A NaN xn fails every compare in both forms (bin 0); so do NaN
// knots, and a NaN suffix t[j0 ..] acts as +inf in both.
// (The knots by value, the selects on values: a conditional between elements
// of the array is an lvalue, which the device compiler turned into an indexed
// load of a copy of the array in scratch memory.)
NFK_HD int nfk_bin_search8(float xn, float t1, float t2, float t3, float t4, float t5, float t6, float t7) {
    const bool c1 = xn >= t4;
    const float a = c1 ? t6 : t2;
    const float b1 = c1 ? t7 : t3, b0 = c1 ? t5 : t1;
    const bool c2 = xn >= a;
    const float b = c2 ? b1 : b0;
    const bool c3 = xn >= b;
    return (c1 ? 4 : 0) + (c2 ? 2 : 0) + (c3 ? 1 : 0);
}
NFK_HD int nfk_bin_search8(float xn, const float (&t)[8]) {
    return nfk_bin_search8(xn, t[1], t[2], t[3], t[4], t[5], t[6], t[7]);
}

template <int K>
NFK_HD int nfk_bin_search(float xn, const float (&t)[K]) {
    if constexpr (K == 8)
        return nfk_bin_search8(xn, t);
    else
        return nfk_bin_count<K>(xn, t);
}
