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

// ---------------------------------------------------------------------------
// Embedded-atom model from setfl tables (systems.py EAM)
// ---------------------------------------------------------------------------
struct EamConst {
    float lf[3], il[3];  // (float)L_a, (float)(1 / L_a)
    int ns[3];           // n_a = floor(rc / L_a + 0.5): the image shifts are -n_a..n_a
    int ks[3];           // how many consecutive shifts of one axis can be within rc of one atom
    float rc, rcp, rc2p; // the cutoff; the cutoff and its square, padded (pre-filters only)
    float inv_dr, inv_drho;
    float rho_max, f_end, fp_end;  // (Nrho - 1) drho, F and dF/drho there
    int nr2, nrho2;      // Nr - 2, Nrho - 2: the last interval of each table
};

// the cubic of one interval, q = (c3, c4, s, y): ((c3 p + c4) p + s) p + y, and its p-derivative
__device__ __forceinline__ float eam_cubic(const float4 q, float p) { return ((q.x * p + q.y) * p + q.z) * p + q.w; }
__device__ __forceinline__ float eam_dcubic(const float4 q, float p) {
    return ((3.0f * q.x) * p + 2.0f * q.y) * p + q.z;
}

// F(rho) (DERIV: dF/drho): the table's cubic, below zero that of interval 0 continued,
// from rho_max on the straight line through the last node with its slope.  A NaN takes
// the line and touches no table entry.
template <bool DERIV>
__device__ __forceinline__ float eam_embed(float rho, const float4* __restrict__ ftab, const EamConst& k) {
    if (!(rho < k.rho_max)) return DERIV ? k.fp_end : k.f_end + k.fp_end * (rho - k.rho_max);
    const float t = rho * k.inv_drho;
    const int m = max(0, min((int)t, k.nrho2));
    const float p = t - (float)m;
    const float4 q = ftab[m];
    return DERIV ? eam_dcubic(q, p) * k.inv_drho : eam_cubic(q, p);
}

// Every image (i, j, s) of one pair.  The pair vector is wrapped once into
// [-L/2, L/2] per component; the terms are visited in ascending (sx, sy, sz) and a
// term counts when 0 < r <= rc.  Per axis only the shifts that can bring this
// lane's component within the (padded) cutoff are walked, starting at the lane's
// own lowest: a superset of the counted terms in the same order, so the sums have
// the bits of the full -n_a..n_a scan.  rtab holds, per interval m, the quadruples
// of f at [2m] and of z = r phi at [2m + 1].
// MODE 0: rho += f, e += phi.  MODE 1: rho += f.  MODE 2: g += [phi' + fps f'] d / r,
// fps = F'(rho_i) + F'(rho_j).
template <int MODE>
__device__ __forceinline__ void eam_pair(const float (&xi)[3], const float4 pj, float fps, const EamConst& k,
                                         const float4* __restrict__ rtab, float& rho, float& e,
                                         float (&g)[3]) {
    const float pjv[3] = {pj.x, pj.y, pj.z};
    float d[3];
    int lo[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        float v = xi[a] - pjv[a];
        v = v - k.lf[a] * rintf(v * k.il[a]);
        d[a] = v;
        lo[a] = max((int)ceilf((-k.rcp - v) * k.il[a] - 1e-4f), -k.ns[a]);
    }
    for (int kx = 0; kx < k.ks[0]; ++kx) {
        const int sx = lo[0] + kx;
        const float dx = d[0] + (float)sx * k.lf[0];
        const float dx2 = dx * dx;
        for (int ky = 0; ky < k.ks[1]; ++ky) {
            const int sy = lo[1] + ky;
            const float dy = d[1] + (float)sy * k.lf[1];
            const float dxy2 = dx2 + dy * dy;
            const bool okxy = sx <= k.ns[0] && sy <= k.ns[1];
            for (int kz = 0; kz < k.ks[2]; ++kz) {
                const int sz = lo[2] + kz;
                const float dz = d[2] + (float)sz * k.lf[2];
                const float r2 = dxy2 + dz * dz;
                if (!(okxy && sz <= k.ns[2] && r2 <= k.rc2p)) continue;
                const float r = sqrtf(r2);
                if (!(r > 0.0f && r <= k.rc)) continue;  // r == 0: the atom itself, or a coincident one
                const float t = r * k.inv_dr;
                const int m = min((int)t, k.nr2);
                const float p = fminf(t - (float)m, 1.0f);
                const float4 qf = rtab[2 * m];
                if (MODE == 1) {
                    rho += eam_cubic(qf, p);
                    continue;
                }
                const float4 qz = rtab[2 * m + 1];
                const float inv = 1.0f / r;
                const float phi = eam_cubic(qz, p) * inv;
                if (MODE == 0) {
                    rho += eam_cubic(qf, p);
                    e += phi;
                } else {
                    const float dphi = (eam_dcubic(qz, p) * k.inv_dr - phi) * inv;
                    const float w = (dphi + fps * (eam_dcubic(qf, p) * k.inv_dr)) * inv;
                    g[0] += w * dx;
                    g[1] += w * dy;
                    g[2] += w * dz;
                }
            }
        }
    }
}

// The (j, s) loops of a row in k_eam's mapping (nfk_eam.hip): lane c0 of a group of
// G lanes owns atoms c0 + q G, q < PPL, in xi; srow holds the row's n atoms as
// float4, read by broadcast, j outermost.  The expressions and the summation order
// are k_eam's, so a force inside a trajectory has the bits of the backward kernel's.
// rho_i of the lane's atoms.
template <int G, int PPL>
__device__ __forceinline__ void eam_row_density(const float (&xi)[PPL][3], const float4* srow, int n, int c0,
                                                const EamConst& k, const float4* __restrict__ rtab,
                                                float (&rho)[PPL]) {
    float e[PPL], f[PPL][3];
#pragma unroll
    for (int q = 0; q < PPL; ++q) rho[q] = e[q] = f[q][0] = f[q][1] = f[q][2] = 0.0f;
    for (int j = 0; j < n; ++j) {
        const float4 pj = srow[j];
#pragma unroll
        for (int q = 0; q < PPL; ++q)
            if (c0 + q * G < n) eam_pair<1>(xi[q], pj, 0.0f, k, rtab, rho[q], e[q], f[q]);
    }
}

// dU/dx_i of the lane's atoms in f, given F'(rho_i) in fpi and F'(rho_j) in the .w
// of the staged slots.  j == i is skipped: the self images' r does not depend on x_i.
template <int G, int PPL>
__device__ __forceinline__ void eam_row_force(const float (&xi)[PPL][3], const float (&fpi)[PPL],
                                              const float4* srow, int n, int c0, const EamConst& k,
                                              const float4* __restrict__ rtab, float (&f)[PPL][3]) {
    float rho[PPL], e[PPL];
#pragma unroll
    for (int q = 0; q < PPL; ++q) rho[q] = e[q] = f[q][0] = f[q][1] = f[q][2] = 0.0f;
    for (int j = 0; j < n; ++j) {
        const float4 pj = srow[j];
#pragma unroll
        for (int q = 0; q < PPL; ++q) {
            const int i = c0 + q * G;
            if (i < n && i != j) eam_pair<2>(xi[q], pj, fpi[q] + pj.w, k, rtab, rho[q], e[q], f[q]);
        }
    }
}

// The lane's share of the row's energy, sum_q F(rho_q) + 0.5 e_q; the row's is its
// group_sum<G>.
template <int G, int PPL>
__device__ __forceinline__ float eam_row_energy(const float (&xi)[PPL][3], const float4* srow, int n, int c0,
                                                const EamConst& k, const float4* __restrict__ rtab,
                                                const float4* __restrict__ ftab) {
    float rho[PPL], e[PPL], f[PPL][3];
#pragma unroll
    for (int q = 0; q < PPL; ++q) rho[q] = e[q] = f[q][0] = f[q][1] = f[q][2] = 0.0f;
    for (int j = 0; j < n; ++j) {
        const float4 pj = srow[j];
#pragma unroll
        for (int q = 0; q < PPL; ++q)
            if (c0 + q * G < n) eam_pair<0>(xi[q], pj, 0.0f, k, rtab, rho[q], e[q], f[q]);
    }
    float u = 0.0f;
#pragma unroll
    for (int q = 0; q < PPL; ++q)
        if (c0 + q * G < n) u += eam_embed<false>(rho[q], ftab, k) + 0.5f * e[q];
    return u;
}

// The integrator's force on the lane's atoms, F = -(1.0f * dU/dx) (what EAM.force makes
// of the backward kernel at g = 1), from the row staged in srow: the density loop,
// F'(rho_i) left in the .w of the lane's own slots, a barrier, the force loop.  The
// __syncthreads is unconditional, so every call sits in block-uniform control flow;
// a row with ok == false walks the barrier without touching memory and gets zeros.
template <int G, int PPL>
__device__ __forceinline__ void eam_row_step_force(bool ok, const float (&xi)[PPL][3], float4* srow, int n,
                                                   int c0, const EamConst& k,
                                                   const float4* __restrict__ rtab,
                                                   const float4* __restrict__ ftab, float (&F)[PPL][3]) {
    float rho[PPL], fpi[PPL], f[PPL][3];
#pragma unroll
    for (int q = 0; q < PPL; ++q) rho[q] = 0.0f;
    if (ok) eam_row_density<G, PPL>(xi, srow, n, c0, k, rtab, rho);
#pragma unroll
    for (int q = 0; q < PPL; ++q) {
        const int i = c0 + q * G;
        fpi[q] = 0.0f;
        if (ok && i < n) {
            fpi[q] = eam_embed<true>(rho[q], ftab, k);
            reinterpret_cast<float*>(srow + i)[3] = fpi[q];
        }
    }
    __syncthreads();
#pragma unroll
    for (int q = 0; q < PPL; ++q) f[q][0] = f[q][1] = f[q][2] = 0.0f;
    if (ok) eam_row_force<G, PPL>(xi, fpi, srow, n, c0, k, rtab, f);
#pragma unroll
    for (int q = 0; q < PPL; ++q)
#pragma unroll
        for (int d = 0; d < 3; ++d) F[q][d] = ok ? -(1.0f * f[q][d]) : 0.0f;
}

inline int eam_const(EamConst& k, int nr, double dr, int nrho, double drho, double f_end, double fp_end,
                     double lx, double ly, double lz, double rc) {
    const double L[3] = {lx, ly, lz};
    if (nr < 2 || nrho < 2 || !(dr > 0.0) || !(drho > 0.0) || !(rc > 0.0)) return 1;
    const double rcp = rc * (1.0 + 1e-5);
    for (int a = 0; a < 3; ++a) {
        if (!(L[a] > 0.0) || rc / L[a] > 8.0) return 1;
        k.lf[a] = (float)L[a];
        k.il[a] = (float)(1.0 / L[a]);
        k.ns[a] = (int)std::floor(rc / L[a] + 0.5);
        const int span = (int)std::floor(2.0 * rcp / L[a] + 2e-4) + 1;
        k.ks[a] = span < 2 * k.ns[a] + 1 ? span : 2 * k.ns[a] + 1;
    }
    k.rc = (float)rc;
    k.rcp = (float)rcp;
    k.rc2p = (float)(rcp * rcp);
    k.inv_dr = (float)(1.0 / dr);
    k.inv_drho = (float)(1.0 / drho);
    k.rho_max = (float)((nrho - 1) * drho);
    k.f_end = (float)f_end;
    k.fp_end = (float)fp_end;
    k.nr2 = nr - 2;
    k.nrho2 = nrho - 2;
    return 0;
}

// The table and box checks of nfk_eam_potential for the dynamics entry points: 0 with k
// filled, or NFK_EINVAL after nfk_set_error.
inline int eam_setup(const char* who, EamConst& k, const void* rtab, int nr, double dr, const void* ftab,
                     int nrho, double drho, double f_end, double fp_end, double lx, double ly, double lz,
                     double rc) {
    char buf[120];
    const char* why = nullptr;
    if ((((uintptr_t)rtab) | ((uintptr_t)ftab)) & 15) why = "tables need 16-byte alignment";
    else if (eam_const(k, nr, dr, nrho, drho, f_end, fp_end, lx, ly, lz, rc)) why = "bad tables, box or cutoff";
    if (!why) return 0;
    std::snprintf(buf, sizeof(buf), "%s: %s", who, why);
    return nfk_set_error(buf);
}

}  // namespace

#endif  // NFK_SYSTEMS_DEV_H_
