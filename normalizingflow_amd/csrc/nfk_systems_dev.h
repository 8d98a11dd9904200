// nfk_systems_dev.h -- the device arithmetic of the applications layer's
// systems (Einstein crystal, Gaussian mixture, Lennard-Jones) and the launch
// helpers around it, shared by nfk_systems.hip (log-density / energy and their
// backward passes), nfk_dynamics.hip (whole trajectories in one launch) and
// nfk_hmc_run.hip (whole HMC runs in one launch).
// One definition of every expression, so a force inside a trajectory has the
// bits of the backward kernel's.  Include after <hip/hip_runtime.h>, <cmath>,
// <cstdio> and nfk.h.
#ifndef NFK_SYSTEMS_DEV_H_
#define NFK_SYSTEMS_DEV_H_

int nfk_set_error(const char* msg);

namespace {

int launch_status(const char* what) {
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) {
        char buf[200];
        std::snprintf(buf, sizeof(buf), "%s: %s", what, hipGetErrorString(e));
        nfk_set_error(buf);
        return (int)e;
    }
    return 0;
}

template <int W>
__device__ __forceinline__ float group_sum(float v) {
    // deterministic butterfly over aligned groups of W lanes (W power of 2 <= 64)
#pragma unroll
    for (int off = W / 2; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}

inline int lanes_for(int n) {
    int w = 1;
    while (w < n && w < 64) w <<= 1;
    return w;
}

inline unsigned grid_for_rows(int64_t rows, int w) {
    const int64_t rows_per_block = (int64_t)(256 / 64) * (64 / w);
    int64_t g = (rows + rows_per_block - 1) / rows_per_block;
    if (g > 65536) g = 65536;
    if (g < 1) g = 1;
    return (unsigned)g;
}

inline unsigned grid_for(int64_t items, int per_block) {
    int64_t g = (items + per_block - 1) / per_block;
    if (g > 65536) g = 65536;
    return (unsigned)(g < 1 ? 1 : g);
}

#define NFK_ROW_PROLOGUE(W)                                                         \
    const int lane = threadIdx.x & 63;                                              \
    const int sub = lane / (W), c0 = lane % (W);                                    \
    const int64_t wave = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;      \
    const int64_t nwave = ((int64_t)gridDim.x * blockDim.x) >> 6;                   \
    constexpr int RPW = 64 / (W);

#define NFK_W_DISPATCH(w, CALL) \
    switch (w) {                \
        case 1: CALL(1); break; \
        case 2: CALL(2); break; \
        case 4: CALL(4); break; \
        case 8: CALL(8); break; \
        case 16: CALL(16); break; \
        case 32: CALL(32); break; \
        default: CALL(64); break; \
    }

// the reference's single wrap: v -= (|v| > 0.5 L) * sign(v) * L  (strict compare;
// hb = (float)(0.5 L), lf = (float)L)
__device__ __forceinline__ float wrap1(float v, float hb, float lf) {
    return fabsf(v) > hb ? v - copysignf(lf, v) : v;
}

// ---------------------------------------------------------------------------
// Einstein crystal (systems.py:366-372)
// ---------------------------------------------------------------------------
// the wrapped deviation of one coordinate
template <bool BOX>
__device__ __forceinline__ float einstein_dev(float z, float cen, float hb, float lf) {
    float dev = z - cen;
    if (BOX) dev = wrap1(dev, hb, lf);
    return dev;
}

// d log_prob / dz of one coordinate: -dev / scale^2 (neg_inv_var = (float)(-1 / scale^2))
__device__ __forceinline__ float einstein_dlp(float dev, float neg_inv_var) { return neg_inv_var * dev; }

// ---------------------------------------------------------------------------
// Gaussian mixture (systems.py:287-292)
// ---------------------------------------------------------------------------
template <int DIM>
__device__ __forceinline__ float gmix_comp(const float (&xv)[DIM], const float* __restrict__ cen,
                                           const float* __restrict__ scales,
                                           const float* __restrict__ hlds, int i, float c2pi,
                                           float (&y)[DIM]) {
    const float s = scales[i];
    float m = 0.0f;
#pragma unroll
    for (int d = 0; d < DIM; ++d) {
        y[d] = (xv[d] - cen[i * DIM + d]) / s;
        m += y[d] * y[d];
    }
    return -0.5f * (c2pi + m) - hlds[i];
}

// density of one particle, accumulated in centre order
template <int DIM>
__device__ __forceinline__ float gmix_prob(const float (&xv)[DIM], const float* __restrict__ cen,
                                           const float* __restrict__ scales,
                                           const float* __restrict__ hlds, int M, float inv_m,
                                           float c2pi) {
    float y[DIM];
    float prob = 0.0f;
    for (int i = 0; i < M; ++i) prob += inv_m * expf(gmix_comp<DIM>(xv, cen, scales, hlds, i, c2pi, y));
    return prob;
}

// d log p / dx of one particle: num[d] / prob with num = sum_i p_i (-(x - c_i) / var_i);
// returns prob and leaves the quotient in dlp (NaN where prob == 0)
template <int DIM>
__device__ __forceinline__ float gmix_dlp(const float (&xv)[DIM], const float* __restrict__ cen,
                                          const float* __restrict__ scales,
                                          const float* __restrict__ hlds, int M, float inv_m,
                                          float c2pi, float (&dlp)[DIM]) {
    float y[DIM], num[DIM];
#pragma unroll
    for (int d = 0; d < DIM; ++d) num[d] = 0.0f;
    float prob = 0.0f;
    for (int i = 0; i < M; ++i) {
        const float pi = inv_m * expf(gmix_comp<DIM>(xv, cen, scales, hlds, i, c2pi, y));
        const float s = scales[i];
        prob += pi;
#pragma unroll
        for (int d = 0; d < DIM; ++d) num[d] -= pi * (y[d] / s);
    }
#pragma unroll
    for (int d = 0; d < DIM; ++d) dlp[d] = num[d] / prob;
    return prob;
}

// ---------------------------------------------------------------------------
// Lennard-Jones (systems.py:154-189)
// ---------------------------------------------------------------------------
struct LjConst {
    float hb, lf;        // (float)(0.5 L), (float)L
    float sigma, eps4;   // (float)sigma, (float)(4 epsilon)
    float cutoff;        // (float)cutoff
    float sh2, sh1;      // (float)(s6^2), (float)s6 (0 without the shift)
    int has_cut;
};

// One (i, j) term.  FWD: returns u(i, j).  BWD: adds du/dr * d/r to f.
template <int DIM, bool BWD>
__device__ __forceinline__ float lj_pair(const float (&xi)[3], const float4 pj, const LjConst& k,
                                         float (&f)[3]) {
    float d[3];
    d[0] = wrap1(xi[0] - pj.x, k.hb, k.lf);
    d[1] = wrap1(xi[1] - pj.y, k.hb, k.lf);
    d[2] = DIM == 3 ? wrap1(xi[2] - pj.z, k.hb, k.lf) : 0.0f;
    float r2 = d[0] * d[0] + d[1] * d[1];
    if (DIM == 3) r2 += d[2] * d[2];
    const float r = sqrtf(r2);
    float inv = 1.0f / (r + (r == 0.0f ? 1.0f : 0.0f));
    if (k.has_cut && r > k.cutoff) inv = 0.0f;
    const float s = k.sigma * inv;
    const float s2 = s * s;
    const float p6 = s2 * s2 * s2;
    if (!BWD) {
        float u = p6 * p6 - p6;
        u = (u - k.sh2) + k.sh1;
        return ((k.eps4 * u) * inv) * r;
    }
    // du/dr = 4 eps (2 p6 - 1) dp6/dr, dp6/dr = -6 p6 / r; zero on the diagonal, for
    // coincident pairs (r == 0) and beyond the cutoff (inv == 0)
    const float dudr = (r == 0.0f) ? 0.0f : (k.eps4 * (2.0f * p6 - 1.0f)) * ((-6.0f * p6) * inv);
    const float w = dudr * inv;
    f[0] += w * d[0];
    f[1] += w * d[1];
    if (DIM == 3) f[2] += w * d[2];
    return 0.0f;
}

// The j loop of a row: lane c0 of a group of G lanes owns particles c0 + q G, q < PPL,
// in xi; srow holds the row's n particles as float4 (every lane of the group reads
// particle j at one address: a broadcast).  FWD: returns the lane's share of sum_ij u.
// BWD: f[q] = sum_j du/dr d/r for the lane's particles (dU/dx_i).
template <int G, int PPL, int DIM, bool BWD>
__device__ __forceinline__ float lj_row(const float (&xi)[PPL][3], const float4* srow, int n, int c0,
                                        const LjConst& k, float (&f)[PPL][3]) {
    float e = 0.0f;
#pragma unroll
    for (int q = 0; q < PPL; ++q) f[q][0] = f[q][1] = f[q][2] = 0.0f;
    for (int j = 0; j < n; ++j) {
        const float4 pj = srow[j];
#pragma unroll
        for (int q = 0; q < PPL; ++q)
            if (c0 + q * G < n) e += lj_pair<DIM, BWD>(xi[q], pj, k, f[q]);
    }
    return e;
}

inline LjConst lj_const(double L, double sigma, double epsilon, int has_cutoff, double cutoff, int shift) {
    // Python scalars of the reference, evaluated in double and rounded to fp32
    // once where the tensor op casts them
    LjConst k;
    k.hb = (float)(0.5 * L);
    k.lf = (float)L;
    k.sigma = (float)sigma;
    k.eps4 = (float)(epsilon * 4.0);
    k.has_cut = has_cutoff ? 1 : 0;
    k.cutoff = has_cutoff ? (float)cutoff : 0.0f;
    k.sh2 = k.sh1 = 0.0f;
    if (has_cutoff && shift) {
        const double s6 = std::pow(sigma / cutoff, 6);
        k.sh2 = (float)(s6 * s6);
        k.sh1 = (float)s6;
    }
    return k;
}

}  // namespace

#endif  // NFK_SYSTEMS_DEV_H_
