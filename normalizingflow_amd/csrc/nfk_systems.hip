// nfk_systems.hip -- priors and targets of the applications layer
// (applications/src/systems.py): the Einstein crystal's and the Gaussian
// mixture's log-densities with the fused "+ sign * log|det|" epilogue of
// nfk_normal_logprob, the Lennard-Jones energy of a periodic box, and their
// backward passes.  Streaming / pairwise VALU kernels: no MFMA, no float
// atomics, every sum in a fixed order.  Built with -ffp-contract=off like the
// other streaming kernels, so each fp32 op rounds as the reference's ATen op.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdio>

#include "../../include/nfk.h"
#include "nfk_systems_dev.h"

namespace {

// ---------------------------------------------------------------------------
// Einstein crystal (systems.py:366-372)
// ---------------------------------------------------------------------------
template <int W, bool BOX>
__global__ __launch_bounds__(256) void k_einstein_lp(const float* __restrict__ z, int64_t ldz,
                                                     const float* __restrict__ cen,
                                                     const float* __restrict__ logdet, float* out,
                                                     int64_t batch, int D, float lii, float c2pi,
                                                     float hld, float hb, float lf, int sign,
                                                     int32_t* status) {
    NFK_ROW_PROLOGUE(W)
    for (int64_t r0 = wave * RPW; r0 < batch; r0 += nwave * RPW) {
        const int64_t b = r0 + sub;
        const bool ok = b < batch;
        float m = 0.0f;
        if (ok)
            for (int c = c0; c < D; c += W) {
                const float dev = einstein_dev<BOX>(z[b * ldz + c], cen[c], hb, lf);
                const float y = dev / lii;  // triangular solve with L = sqrt(1/alpha) I
                m += y * y;
            }
        m = group_sum<W>(m);
        if (ok && c0 == 0) {
            float lp = -0.5f * (c2pi + m) - hld;
            if (logdet) lp = (sign >= 0) ? (lp + logdet[b]) : (lp - logdet[b]);
            out[b] = lp;
        }
        // a NaN in the row makes m NaN (squares of infinities stay infinite)
        if (__any(ok && c0 == 0 && m != m) && status != nullptr && (threadIdx.x & 63) == 0)
            atomicOr(status, NFK_ST_NAN_Z);
    }
}

// float4 form for D % 4 == 0 and 16-B aligned rows (centers come from a
// hipMalloc'ed tensor and are checked for alignment too)
template <int W, bool BOX>
__global__ __launch_bounds__(256) void k_einstein_lp4(const float4* __restrict__ z4, int64_t ldz4,
                                                      const float4* __restrict__ cen4,
                                                      const float* __restrict__ logdet, float* out,
                                                      int64_t batch, int D4, float inv_l, float c2pi,
                                                      float hld, float hb, float lf, int sign,
                                                      int32_t* status) {
    NFK_ROW_PROLOGUE(W)
    for (int64_t r0 = wave * RPW; r0 < batch; r0 += nwave * RPW) {
        const int64_t b = r0 + sub;
        const bool ok = b < batch;
        float m = 0.0f;
        if (ok)
            for (int c = c0; c < D4; c += W) {
                const float4 v = z4[b * ldz4 + c];
                const float4 q = cen4[c];
                float d0 = v.x - q.x, d1 = v.y - q.y, d2 = v.z - q.z, d3 = v.w - q.w;
                if (BOX) {
                    d0 = wrap1(d0, hb, lf);
                    d1 = wrap1(d1, hb, lf);
                    d2 = wrap1(d2, hb, lf);
                    d3 = wrap1(d3, hb, lf);
                }
                const float y0 = d0 * inv_l, y1 = d1 * inv_l, y2 = d2 * inv_l, y3 = d3 * inv_l;
                m += (y0 * y0 + y1 * y1) + (y2 * y2 + y3 * y3);
            }
        m = group_sum<W>(m);
        if (ok && c0 == 0) {
            float lp = -0.5f * (c2pi + m) - hld;
            if (logdet) lp = (sign >= 0) ? (lp + logdet[b]) : (lp - logdet[b]);
            out[b] = lp;
        }
        if (__any(ok && c0 == 0 && m != m) && status != nullptr && (threadIdx.x & 63) == 0)
            atomicOr(status, NFK_ST_NAN_Z);
    }
}

__global__ __launch_bounds__(256) void k_einstein_bwd(const float* __restrict__ z, int64_t ldz,
                                                      const float* __restrict__ cen,
                                                      const float* __restrict__ g, float* gz,
                                                      int64_t ldgz, int64_t batch, int D,
                                                      float neg_inv_var, int box, float hb, float lf) {
    const int64_t tot = batch * D;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < tot;
         i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t b = i / D;
        const int c = (int)(i - b * D);
        const float dev = box ? einstein_dev<true>(z[b * ldz + c], cen[c], hb, lf)
                              : einstein_dev<false>(z[b * ldz + c], cen[c], hb, lf);
        gz[b * ldgz + c] = einstein_dlp(dev, neg_inv_var) * g[b];
    }
}

// ---------------------------------------------------------------------------
// Gaussian mixture (systems.py:287-292).  The centre loop's index is wave
// uniform, so centres, scales and hlds come through scalar loads.
// ---------------------------------------------------------------------------
template <int W, int DIM>
__global__ __launch_bounds__(256) void k_gmix_lp(const float* __restrict__ x, int64_t ldx,
                                                 const float* __restrict__ cen,
                                                 const float* __restrict__ scales,
                                                 const float* __restrict__ hlds,
                                                 const float* __restrict__ logdet, float* out,
                                                 int64_t batch, int npart, int M, float inv_m,
                                                 float c2pi, int sign, int32_t* status) {
    NFK_ROW_PROLOGUE(W)
    for (int64_t r0 = wave * RPW; r0 < batch; r0 += nwave * RPW) {
        const int64_t b = r0 + sub;
        const bool ok = b < batch;
        float acc = 0.0f;
        if (ok)
            for (int p = c0; p < npart; p += W) {
                float xv[DIM];
#pragma unroll
                for (int d = 0; d < DIM; ++d) xv[d] = x[b * ldx + p * DIM + d];
                acc += logf(gmix_prob<DIM>(xv, cen, scales, hlds, M, inv_m, c2pi));
            }
        acc = group_sum<W>(acc);
        if (ok && c0 == 0) {
            float lp = acc;
            if (logdet) lp = (sign >= 0) ? (lp + logdet[b]) : (lp - logdet[b]);
            out[b] = lp;
        }
        // a NaN coordinate makes its particle's log p NaN; -inf (a far particle) is not one
        if (__any(ok && c0 == 0 && acc != acc) && status != nullptr && (threadIdx.x & 63) == 0)
            atomicOr(status, NFK_ST_NAN_Z);
    }
}

// one lane per particle
template <int DIM>
__global__ __launch_bounds__(256) void k_gmix_bwd(const float* __restrict__ x, int64_t ldx,
                                                  const float* __restrict__ cen,
                                                  const float* __restrict__ scales,
                                                  const float* __restrict__ hlds,
                                                  const float* __restrict__ g, float* gx, int64_t ldgx,
                                                  int64_t batch, int npart, int M, float inv_m,
                                                  float c2pi) {
    const int64_t tot = batch * npart;
    for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < tot;
         t += (int64_t)gridDim.x * blockDim.x) {
        const int64_t b = t / npart;
        const int p = (int)(t - b * npart);
        float xv[DIM], dlp[DIM];
#pragma unroll
        for (int d = 0; d < DIM; ++d) xv[d] = x[b * ldx + p * DIM + d];
        gmix_dlp<DIM>(xv, cen, scales, hlds, M, inv_m, c2pi, dlp);
        const float gb = g[b];
#pragma unroll
        for (int d = 0; d < DIM; ++d) gx[b * ldgx + p * DIM + d] = gb * dlp[d];
    }
}

// ---------------------------------------------------------------------------
// Lennard-Jones (systems.py:154-189)
// ---------------------------------------------------------------------------
// A row occupies G lanes (64 / G rows per wave, 4 waves per block); lane c0 owns
// particles c0 + k G, k < PPL (PPL > 1 only with G == 64).  The block's rows
// are staged in LDS as float4 per particle; every lane of a group reads
// particle j at one address (a broadcast), so the j loop costs one LDS read.
template <int G, int PPL, int DIM, bool BWD>
__global__ __launch_bounds__(256) void k_lj(const float* __restrict__ x, int64_t ldx,
                                            const float* __restrict__ g, float* out, int64_t ldo,
                                            int64_t batch, int n, LjConst k) {
    extern __shared__ __attribute__((aligned(16))) float4 s_pos[];
    constexpr int RPW = 64 / G, RPB = 4 * RPW;
    const int lane = threadIdx.x & 63;
    const int rb = (threadIdx.x >> 6) * RPW + lane / G;  // row within the block
    const int c0 = lane % G;
    float4* srow = s_pos + (size_t)rb * n;
    for (int64_t r0 = (int64_t)blockIdx.x * RPB; r0 < batch; r0 += (int64_t)gridDim.x * RPB) {
        const int64_t b = r0 + rb;
        const bool ok = b < batch;
        float xi[PPL][3];
#pragma unroll
        for (int q = 0; q < PPL; ++q) {
            const int i = c0 + q * G;
            xi[q][0] = xi[q][1] = xi[q][2] = 0.0f;
            if (ok && i < n) {
                const float* p = x + b * ldx + (int64_t)i * DIM;
                xi[q][0] = p[0];
                xi[q][1] = p[1];
                if (DIM == 3) xi[q][2] = p[2];
                srow[i] = make_float4(xi[q][0], xi[q][1], xi[q][2], 0.0f);
            }
        }
        __syncthreads();
        float e = 0.0f;
        float f[PPL][3];
        if (ok) e = lj_row<G, PPL, DIM, BWD>(xi, srow, n, c0, k, f);
        if (BWD) {
            if (ok) {
                const float gb = g[b];
#pragma unroll
                for (int q = 0; q < PPL; ++q) {
                    const int i = c0 + q * G;
                    if (i < n) {
                        float* p = out + b * ldo + (int64_t)i * DIM;
                        p[0] = gb * f[q][0];
                        p[1] = gb * f[q][1];
                        if (DIM == 3) p[2] = gb * f[q][2];
                    }
                }
            }
        } else {
            e = group_sum<G>(e);
            if (ok && c0 == 0) out[b] = e / 2.0f;
        }
        __syncthreads();  // the next round overwrites the staged rows
    }
}

template <bool BWD>
int lj_launch(const float* x, int64_t ldx, const float* g, float* out, int64_t ldo, int64_t batch,
              int n, int dim, const LjConst& k, hipStream_t st) {
    const int G = lanes_for(n);
    const int ppl = (n + 63) / 64;
    const int rpb = 4 * (64 / G);
    int64_t grid = (batch + rpb - 1) / rpb;
    if (grid > 16384) grid = 16384;
    if (grid < 1) grid = 1;
    const size_t lds = (size_t)rpb * n * sizeof(float4);  // <= 16 KiB (n <= 256)
#define LJ_CALL2(GG, PP)                                                                              \
    do {                                                                                              \
        if (dim == 3)                                                                                 \
            hipLaunchKernelGGL((k_lj<GG, PP, 3, BWD>), dim3((unsigned)grid), dim3(256), lds, st, x, ldx, \
                               g, out, ldo, batch, n, k);                                             \
        else                                                                                          \
            hipLaunchKernelGGL((k_lj<GG, PP, 2, BWD>), dim3((unsigned)grid), dim3(256), lds, st, x, ldx, \
                               g, out, ldo, batch, n, k);                                             \
    } while (0)
#define LJ_CALL(W) LJ_CALL2(W, 1)
    if (ppl <= 1) {
        NFK_W_DISPATCH(G, LJ_CALL)
    } else if (ppl == 2) {
        LJ_CALL2(64, 2);
    } else if (ppl == 3) {
        LJ_CALL2(64, 3);
    } else {
        LJ_CALL2(64, 4);
    }
#undef LJ_CALL
#undef LJ_CALL2
    return 0;
}

}  // namespace

// ---------------------------------------------------------------------------
// C ABI
// ---------------------------------------------------------------------------
extern "C" int nfk_einstein_logprob(const float* z, int64_t ldz, const float* centers,
                                    const float* logdet, float* out, int64_t batch, int32_t natoms,
                                    int32_t dim, float scale, float half_log_det, int32_t has_box,
                                    double boxlength, int32_t sign, int32_t* status,
                                    nfk_stream_t stream) {
    if (batch < 0 || natoms <= 0 || dim <= 0 || (int64_t)natoms * dim > (1 << 24) || !(scale > 0.0f))
        return nfk_set_error("nfk_einstein_logprob: bad args");
    if (batch == 0) return 0;
    if (!z || !centers || !out) return nfk_set_error("nfk_einstein_logprob: null pointer");
    const int D = natoms * dim;
    if (ldz < D && batch > 1) return nfk_set_error("nfk_einstein_logprob: ldz below the row width");
    hipStream_t st = (hipStream_t)stream;
    const float c2pi = (float)(D * std::log(2.0 * M_PI));
    const float hld = (float)((double)natoms * (double)half_log_det);
    const float hb = (float)(0.5 * boxlength), lf = (float)boxlength;
    if (D % 4 == 0 && ldz % 4 == 0 && ((uintptr_t)z & 15) == 0 && ((uintptr_t)centers & 15) == 0) {
        const int D4 = D / 4, w4 = lanes_for(D4);
        const unsigned g4 = grid_for_rows(batch, w4);
        const float inv_l = 1.0f / scale;
#define CALL4(W)                                                                                        \
    if (has_box)                                                                                        \
        hipLaunchKernelGGL((k_einstein_lp4<W, true>), dim3(g4), dim3(256), 0, st, (const float4*)z,     \
                           ldz / 4, (const float4*)centers, logdet, out, batch, D4, inv_l, c2pi, hld, hb, \
                           lf, sign, status);                                                           \
    else                                                                                                \
        hipLaunchKernelGGL((k_einstein_lp4<W, false>), dim3(g4), dim3(256), 0, st, (const float4*)z,    \
                           ldz / 4, (const float4*)centers, logdet, out, batch, D4, inv_l, c2pi, hld, hb, \
                           lf, sign, status);
        NFK_W_DISPATCH(w4, CALL4)
#undef CALL4
        return launch_status("nfk_einstein_logprob");
    }
    const int w = lanes_for(D);
    const unsigned g = grid_for_rows(batch, w);
#define CALL(W)                                                                                       \
    if (has_box)                                                                                      \
        hipLaunchKernelGGL((k_einstein_lp<W, true>), dim3(g), dim3(256), 0, st, z, ldz, centers, logdet, \
                           out, batch, D, scale, c2pi, hld, hb, lf, sign, status);                    \
    else                                                                                              \
        hipLaunchKernelGGL((k_einstein_lp<W, false>), dim3(g), dim3(256), 0, st, z, ldz, centers, logdet, \
                           out, batch, D, scale, c2pi, hld, hb, lf, sign, status);
    NFK_W_DISPATCH(w, CALL)
#undef CALL
    return launch_status("nfk_einstein_logprob");
}

extern "C" int nfk_einstein_logprob_bwd(const float* z, int64_t ldz, const float* centers,
                                        const float* g, float* gz, int64_t ldgz, int64_t batch,
                                        int32_t natoms, int32_t dim, float scale, int32_t has_box,
                                        double boxlength, nfk_stream_t stream) {
    if (batch < 0 || natoms <= 0 || dim <= 0 || (int64_t)natoms * dim > (1 << 24) || !(scale > 0.0f))
        return nfk_set_error("nfk_einstein_logprob_bwd: bad args");
    if (batch == 0) return 0;
    if (!z || !centers || !g || !gz) return nfk_set_error("nfk_einstein_logprob_bwd: null pointer");
    const int D = natoms * dim;
    if ((ldz < D || ldgz < D) && batch > 1)
        return nfk_set_error("nfk_einstein_logprob_bwd: leading dimension below the row width");
    const float niv = (float)(-1.0 / ((double)scale * (double)scale));
    hipLaunchKernelGGL(k_einstein_bwd, dim3(grid_for(batch * D, 256)), dim3(256), 0, (hipStream_t)stream,
                       z, ldz, centers, g, gz, ldgz, batch, D, niv, has_box ? 1 : 0,
                       (float)(0.5 * boxlength), (float)boxlength);
    return launch_status("nfk_einstein_logprob_bwd");
}

extern "C" int nfk_gmix_supported(int32_t ncenters, int32_t dim) {
    return (ncenters >= 1 && ncenters <= 64 && dim >= 1 && dim <= 4) ? 1 : 0;
}

extern "C" int nfk_gmix_logprob(const float* x, int64_t ldx, const float* centers,
                                const float* scales, const float* hlds, const float* logdet,
                                float* out, int64_t batch, int32_t npart, int32_t dim,
                                int32_t ncenters, int32_t sign, int32_t* status,
                                nfk_stream_t stream) {
    if (batch < 0 || npart <= 0 || npart > (1 << 22)) return nfk_set_error("nfk_gmix_logprob: bad sizes");
    if (!nfk_gmix_supported(ncenters, dim)) return nfk_set_error("nfk_gmix_logprob: shape not supported");
    if (batch == 0) return 0;
    if (!x || !centers || !scales || !hlds || !out) return nfk_set_error("nfk_gmix_logprob: null pointer");
    if (ldx < (int64_t)npart * dim && batch > 1)
        return nfk_set_error("nfk_gmix_logprob: ldx below the row width");
    hipStream_t st = (hipStream_t)stream;
    const float inv_m = (float)(1.0 / ncenters);
    const float c2pi = (float)(dim * std::log(2.0 * M_PI));
    const int w = lanes_for(npart);
    const unsigned g = grid_for_rows(batch, w);
#define CALLD(W, DD)                                                                              \
    hipLaunchKernelGGL((k_gmix_lp<W, DD>), dim3(g), dim3(256), 0, st, x, ldx, centers, scales, hlds, \
                       logdet, out, batch, npart, ncenters, inv_m, c2pi, sign, status)
#define CALL(W)                         \
    switch (dim) {                      \
        case 1: CALLD(W, 1); break;     \
        case 2: CALLD(W, 2); break;     \
        case 3: CALLD(W, 3); break;     \
        default: CALLD(W, 4); break;    \
    }
    NFK_W_DISPATCH(w, CALL)
#undef CALL
#undef CALLD
    return launch_status("nfk_gmix_logprob");
}

extern "C" int nfk_gmix_logprob_bwd(const float* x, int64_t ldx, const float* centers,
                                    const float* scales, const float* hlds, const float* g, float* gx,
                                    int64_t ldgx, int64_t batch, int32_t npart, int32_t dim,
                                    int32_t ncenters, nfk_stream_t stream) {
    if (batch < 0 || npart <= 0 || npart > (1 << 22)) return nfk_set_error("nfk_gmix_logprob_bwd: bad sizes");
    if (!nfk_gmix_supported(ncenters, dim))
        return nfk_set_error("nfk_gmix_logprob_bwd: shape not supported");
    if (batch == 0) return 0;
    if (!x || !centers || !scales || !hlds || !g || !gx)
        return nfk_set_error("nfk_gmix_logprob_bwd: null pointer");
    const int64_t wd = (int64_t)npart * dim;
    if ((ldx < wd || ldgx < wd) && batch > 1)
        return nfk_set_error("nfk_gmix_logprob_bwd: leading dimension below the row width");
    hipStream_t st = (hipStream_t)stream;
    const float inv_m = (float)(1.0 / ncenters);
    const float c2pi = (float)(dim * std::log(2.0 * M_PI));
    const unsigned grid = grid_for(batch * npart, 256);
#define CALLD(DD)                                                                                  \
    hipLaunchKernelGGL((k_gmix_bwd<DD>), dim3(grid), dim3(256), 0, st, x, ldx, centers, scales, hlds, g, \
                       gx, ldgx, batch, npart, ncenters, inv_m, c2pi)
    switch (dim) {
        case 1: CALLD(1); break;
        case 2: CALLD(2); break;
        case 3: CALLD(3); break;
        default: CALLD(4); break;
    }
#undef CALLD
    return launch_status("nfk_gmix_logprob_bwd");
}

extern "C" int nfk_lj_supported(int32_t n, int32_t dim) {
    return (n >= 1 && n <= 256 && (dim == 2 || dim == 3)) ? 1 : 0;
}

extern "C" int nfk_lj_potential(const float* x, int64_t ldx, float* out, int64_t batch, int32_t n,
                                int32_t dim, double boxlength, double sigma, double epsilon,
                                int32_t has_cutoff, double cutoff, int32_t shift, nfk_stream_t stream) {
    if (batch < 0) return nfk_set_error("nfk_lj_potential: bad batch");
    if (!nfk_lj_supported(n, dim)) return nfk_set_error("nfk_lj_potential: shape not supported");
    if (has_cutoff && !(cutoff > 0.0)) return nfk_set_error("nfk_lj_potential: bad cutoff");
    if (batch == 0) return 0;
    if (!x || !out) return nfk_set_error("nfk_lj_potential: null pointer");
    if (ldx < (int64_t)n * dim && batch > 1) return nfk_set_error("nfk_lj_potential: ldx below the row width");
    const LjConst k = lj_const(boxlength, sigma, epsilon, has_cutoff, cutoff, shift);
    lj_launch<false>(x, ldx, nullptr, out, 0, batch, n, dim, k, (hipStream_t)stream);
    return launch_status("nfk_lj_potential");
}

extern "C" int nfk_lj_potential_bwd(const float* x, int64_t ldx, const float* g, float* gx,
                                    int64_t ldgx, int64_t batch, int32_t n, int32_t dim,
                                    double boxlength, double sigma, double epsilon, int32_t has_cutoff,
                                    double cutoff, int32_t shift, nfk_stream_t stream) {
    if (batch < 0) return nfk_set_error("nfk_lj_potential_bwd: bad batch");
    if (!nfk_lj_supported(n, dim)) return nfk_set_error("nfk_lj_potential_bwd: shape not supported");
    if (has_cutoff && !(cutoff > 0.0)) return nfk_set_error("nfk_lj_potential_bwd: bad cutoff");
    if (batch == 0) return 0;
    if (!x || !g || !gx) return nfk_set_error("nfk_lj_potential_bwd: null pointer");
    const int64_t wd = (int64_t)n * dim;
    if ((ldx < wd || ldgx < wd) && batch > 1)
        return nfk_set_error("nfk_lj_potential_bwd: leading dimension below the row width");
    const LjConst k = lj_const(boxlength, sigma, epsilon, has_cutoff, cutoff, shift);
    lj_launch<true>(x, ldx, g, gx, ldgx, batch, n, dim, k, (hipStream_t)stream);
    return launch_status("nfk_lj_potential_bwd");
}
