// nfk_dynamics.hip -- whole molecular-dynamics trajectories of the applications
// layer's systems in ONE launch (integration_step, systems.py:297-338 and
// 382-401) and the Metropolis step of HMC (nf/hmc.py:56-63).  A trajectory's
// position, velocity and current force stay in registers across the path_len
// loop; the forces are the expressions of nfk_systems.hip's backward kernels
// (nfk_systems_dev.h), so a fused trajectory has the bits of the per-step chain
// of force kernels and elementwise ops.  VALU kernels: no MFMA, no atomics,
// every sum in a fixed order, -ffp-contract=off.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdio>

#include "../../include/nfk.h"
#include "nfk_step.h"  // Step, step_x, step_v, make_step: shared with nfk_hmc_run.hip
#include "nfk_systems_dev.h"

namespace {

// ---------------------------------------------------------------------------
// Einstein crystal: a coordinate's force depends on that coordinate alone, so a
// lane carries one coordinate through the whole path (and then the next one,
// W lanes further on); only the potential at the end is a row sum.
// ---------------------------------------------------------------------------
template <int W, bool BOX>
__global__ __launch_bounds__(256) void k_einstein_traj(const float* x_in, int64_t ldxi, const float* v_in,
                                                       int64_t ldvi, const float* __restrict__ cen,
                                                       float* x_out, int64_t ldxo, float* v_out,
                                                       int64_t ldvo, float* __restrict__ pot,
                                                       int64_t batch, int D, Step s, float neg_inv_var,
                                                       float lii, float c2pi, float hld, float hb,
                                                       float lf) {
    NFK_ROW_PROLOGUE(W)
    for (int64_t r0 = wave * RPW; r0 < batch; r0 += nwave * RPW) {
        const int64_t b = r0 + sub;
        const bool ok = b < batch;
        float m = 0.0f;
        if (ok)
            for (int c = c0; c < D; c += W) {
                const float cc = cen[c];
                float x = x_in[b * ldxi + c], v = v_in[b * ldvi + c];
                float G = einstein_dlp(einstein_dev<BOX>(x, cc, hb, lf), neg_inv_var);
                for (int k = 0; k < s.path_len; ++k) {
                    const float xn = step_x(x, v, G, s);
                    const float Gn = einstein_dlp(einstein_dev<BOX>(s.verlet ? xn : x, cc, hb, lf), neg_inv_var);
                    v = step_v(v, G, Gn, s);
                    x = xn;
                    G = Gn;
                }
                x_out[b * ldxo + c] = x;
                v_out[b * ldvo + c] = v;
                const float y = einstein_dev<BOX>(x, cc, hb, lf) / lii;
                m += y * y;
            }
        m = group_sum<W>(m);
        if (ok && c0 == 0) pot[b] = -(-0.5f * (c2pi + m) - hld);
    }
}

// ---------------------------------------------------------------------------
// Gaussian mixture: particles are independent, a lane carries one particle.
// ---------------------------------------------------------------------------
template <int W, int DIM>
__global__ __launch_bounds__(256) void k_gmix_traj(const float* x_in, int64_t ldxi, const float* v_in,
                                                   int64_t ldvi, const float* __restrict__ cen,
                                                   const float* __restrict__ scales,
                                                   const float* __restrict__ hlds, float* x_out,
                                                   int64_t ldxo, float* v_out, int64_t ldvo,
                                                   float* __restrict__ pot, int64_t batch, int npart,
                                                   int M, Step s, float inv_m, float c2pi) {
    NFK_ROW_PROLOGUE(W)
    for (int64_t r0 = wave * RPW; r0 < batch; r0 += nwave * RPW) {
        const int64_t b = r0 + sub;
        const bool ok = b < batch;
        float acc = 0.0f;
        if (ok)
            for (int p = c0; p < npart; p += W) {
                float x[DIM], v[DIM], G[DIM], xn[DIM], Gn[DIM];
#pragma unroll
                for (int d = 0; d < DIM; ++d) {
                    x[d] = x_in[b * ldxi + p * DIM + d];
                    v[d] = v_in[b * ldvi + p * DIM + d];
                }
                gmix_dlp<DIM>(x, cen, scales, hlds, M, inv_m, c2pi, G);
                for (int k = 0; k < s.path_len; ++k) {
#pragma unroll
                    for (int d = 0; d < DIM; ++d) xn[d] = step_x(x[d], v[d], G[d], s);
                    if (s.verlet)
                        gmix_dlp<DIM>(xn, cen, scales, hlds, M, inv_m, c2pi, Gn);
                    else
                        gmix_dlp<DIM>(x, cen, scales, hlds, M, inv_m, c2pi, Gn);
#pragma unroll
                    for (int d = 0; d < DIM; ++d) {
                        v[d] = step_v(v[d], G[d], Gn[d], s);
                        x[d] = xn[d];
                        G[d] = Gn[d];
                    }
                }
#pragma unroll
                for (int d = 0; d < DIM; ++d) {
                    x_out[b * ldxo + p * DIM + d] = x[d];
                    v_out[b * ldvo + p * DIM + d] = v[d];
                }
                acc += logf(gmix_prob<DIM>(x, cen, scales, hlds, M, inv_m, c2pi));
            }
        acc = group_sum<W>(acc);
        if (ok && c0 == 0) pot[b] = -acc;
    }
}

// ---------------------------------------------------------------------------
// Lennard-Jones: k_lj's mapping (a row on G lanes, PPL particles per lane, the
// row staged in LDS as float4 and read by broadcast).  A row never leaves its
// wave.  Every step stages the new positions in the row's other LDS buffer, so
// a step needs one barrier: the buffer being written was last read before the
// previous step's barrier.
// ---------------------------------------------------------------------------
template <int G, int PPL, int DIM>
__global__ __launch_bounds__(256) void k_lj_traj(const float* x_in, int64_t ldxi, const float* v_in,
                                                 int64_t ldvi, float* x_out, int64_t ldxo, float* v_out,
                                                 int64_t ldvo, float* __restrict__ pot, int64_t batch,
                                                 int n, Step s, LjConst k) {
    extern __shared__ __attribute__((aligned(16))) float4 s_pos[];
    constexpr int RPW = 64 / G, RPB = 4 * RPW;
    const int lane = threadIdx.x & 63;
    const int rb = (threadIdx.x >> 6) * RPW + lane / G;  // row within the block
    const int c0 = lane % G;
    float4* srow = s_pos + (size_t)rb * n;  // buffer 0; buffer 1 lies RPB rows further on
    const int other = RPB * n;
    for (int64_t r0 = (int64_t)blockIdx.x * RPB; r0 < batch; r0 += (int64_t)gridDim.x * RPB) {
        const int64_t b = r0 + rb;
        const bool ok = b < batch;
        float x[PPL][3], v[PPL][3], F[PPL][3], xn[PPL][3], f[PPL][3];
#pragma unroll
        for (int q = 0; q < PPL; ++q) {
            const int i = c0 + q * G;
            x[q][0] = x[q][1] = x[q][2] = 0.0f;
            v[q][0] = v[q][1] = v[q][2] = 0.0f;
            if (ok && i < n) {
                const float* px = x_in + b * ldxi + (int64_t)i * DIM;
                const float* pv = v_in + b * ldvi + (int64_t)i * DIM;
#pragma unroll
                for (int d = 0; d < DIM; ++d) {
                    x[q][d] = px[d];
                    v[q][d] = pv[d];
                }
                srow[i] = make_float4(x[q][0], x[q][1], x[q][2], 0.0f);
            }
        }
        __syncthreads();
        int cur = 0;
        if (ok) lj_row<G, PPL, DIM, true>(x, srow, n, c0, k, f);
#pragma unroll
        for (int q = 0; q < PPL; ++q)
#pragma unroll
            for (int d = 0; d < 3; ++d) F[q][d] = ok ? -f[q][d] : 0.0f;
        for (int st = 0; st < s.path_len; ++st) {
#pragma unroll
            for (int q = 0; q < PPL; ++q)
#pragma unroll
                for (int d = 0; d < 3; ++d) xn[q][d] = d < DIM ? step_x(x[q][d], v[q][d], F[q][d], s) : 0.0f;
            if (!s.verlet && ok) lj_row<G, PPL, DIM, true>(x, srow + cur * other, n, c0, k, f);
#pragma unroll
            for (int q = 0; q < PPL; ++q) {
                const int i = c0 + q * G;
                if (ok && i < n) srow[(cur ^ 1) * other + i] = make_float4(xn[q][0], xn[q][1], xn[q][2], 0.0f);
            }
            __syncthreads();
            cur ^= 1;
            if (s.verlet && ok) lj_row<G, PPL, DIM, true>(xn, srow + cur * other, n, c0, k, f);
#pragma unroll
            for (int q = 0; q < PPL; ++q)
#pragma unroll
                for (int d = 0; d < 3; ++d) {
                    const float Fn = ok ? -f[q][d] : 0.0f;
                    v[q][d] = step_v(v[q][d], F[q][d], Fn, s);
                    x[q][d] = xn[q][d];
                    F[q][d] = Fn;
                }
        }
        float e = 0.0f;
        if (ok) {
            e = lj_row<G, PPL, DIM, false>(x, srow + cur * other, n, c0, k, f);
#pragma unroll
            for (int q = 0; q < PPL; ++q) {
                const int i = c0 + q * G;
                if (i < n) {
                    float* px = x_out + b * ldxo + (int64_t)i * DIM;
                    float* pv = v_out + b * ldvo + (int64_t)i * DIM;
#pragma unroll
                    for (int d = 0; d < DIM; ++d) {
                        px[d] = x[q][d];
                        pv[d] = v[q][d];
                    }
                }
            }
        }
        e = group_sum<G>(e);
        if (ok && c0 == 0) pot[b] = e / 2.0f;
        __syncthreads();  // the next round overwrites the staged rows
    }
}

// ---------------------------------------------------------------------------
// Embedded-atom model: k_eam's mapping and k_lj_traj's two LDS buffers per row.
// A force evaluation on a staged buffer is two (j, s) loops with a barrier between
// them (eam_row_step_force: the densities, F'(rho_i) into the .w of the lane's own
// slots, the barrier, the forces), so a step has two barriers: that one and the
// one after the new positions are staged in the other buffer, which was last read
// before the previous step's staging barrier.  path_len and the scheme are
// kernel-uniform and rows past `batch` walk the barriers without touching
// memory: every __syncthreads sits in block-uniform control flow.
// ---------------------------------------------------------------------------
template <int G, int PPL>
__global__ __launch_bounds__(256) void k_eam_traj(const float* x_in, int64_t ldxi, const float* v_in,
                                                  int64_t ldvi, float* x_out, int64_t ldxo, float* v_out,
                                                  int64_t ldvo, float* __restrict__ pot, int64_t batch,
                                                  int n, Step s, const float4* __restrict__ rtab,
                                                  const float4* __restrict__ ftab, EamConst k) {
    extern __shared__ __attribute__((aligned(16))) float4 s_pos[];
    constexpr int RPW = 64 / G, RPB = 4 * RPW;
    const int lane = threadIdx.x & 63;
    const int rb = (threadIdx.x >> 6) * RPW + lane / G;  // row within the block
    const int c0 = lane % G;
    float4* srow = s_pos + (size_t)rb * n;  // buffer 0; buffer 1 lies RPB rows further on
    const int other = RPB * n;
    for (int64_t r0 = (int64_t)blockIdx.x * RPB; r0 < batch; r0 += (int64_t)gridDim.x * RPB) {
        const int64_t b = r0 + rb;
        const bool ok = b < batch;
        float x[PPL][3], v[PPL][3], F[PPL][3], xn[PPL][3], Fn[PPL][3];
#pragma unroll
        for (int q = 0; q < PPL; ++q) {
            const int i = c0 + q * G;
            x[q][0] = x[q][1] = x[q][2] = 0.0f;
            v[q][0] = v[q][1] = v[q][2] = 0.0f;
            if (ok && i < n) {
                const float* px = x_in + b * ldxi + (int64_t)i * 3;
                const float* pv = v_in + b * ldvi + (int64_t)i * 3;
#pragma unroll
                for (int d = 0; d < 3; ++d) {
                    x[q][d] = px[d];
                    v[q][d] = pv[d];
                }
                srow[i] = make_float4(x[q][0], x[q][1], x[q][2], 0.0f);
            }
        }
        __syncthreads();
        int cur = 0;
        eam_row_step_force<G, PPL>(ok, x, srow, n, c0, k, rtab, ftab, F);
        for (int st = 0; st < s.path_len; ++st) {
#pragma unroll
            for (int q = 0; q < PPL; ++q)
#pragma unroll
                for (int d = 0; d < 3; ++d) xn[q][d] = step_x(x[q][d], v[q][d], F[q][d], s);
            if (!s.verlet) eam_row_step_force<G, PPL>(ok, x, srow + cur * other, n, c0, k, rtab, ftab, Fn);
#pragma unroll
            for (int q = 0; q < PPL; ++q) {
                const int i = c0 + q * G;
                if (ok && i < n) srow[(cur ^ 1) * other + i] = make_float4(xn[q][0], xn[q][1], xn[q][2], 0.0f);
            }
            __syncthreads();
            cur ^= 1;
            if (s.verlet) eam_row_step_force<G, PPL>(ok, xn, srow + cur * other, n, c0, k, rtab, ftab, Fn);
#pragma unroll
            for (int q = 0; q < PPL; ++q)
#pragma unroll
                for (int d = 0; d < 3; ++d) {
                    v[q][d] = step_v(v[q][d], F[q][d], Fn[q][d], s);
                    x[q][d] = xn[q][d];
                    F[q][d] = Fn[q][d];
                }
        }
        float e = 0.0f;
        if (ok) {
            e = eam_row_energy<G, PPL>(x, srow + cur * other, n, c0, k, rtab, ftab);
#pragma unroll
            for (int q = 0; q < PPL; ++q) {
                const int i = c0 + q * G;
                if (i < n) {
                    float* px = x_out + b * ldxo + (int64_t)i * 3;
                    float* pv = v_out + b * ldvo + (int64_t)i * 3;
#pragma unroll
                    for (int d = 0; d < 3; ++d) {
                        px[d] = x[q][d];
                        pv[d] = v[q][d];
                    }
                }
            }
        }
        e = group_sum<G>(e);
        if (ok && c0 == 0) pot[b] = e;
        __syncthreads();  // the next round overwrites the staged rows
    }
}

// ---------------------------------------------------------------------------
// Metropolis step: a chain on W lanes; the group's first lane decides and
// updates the chain's scalars, the group copies the row.
// ---------------------------------------------------------------------------
template <int W>
__global__ __launch_bounds__(256) void k_hmc_accept(float* __restrict__ x_cur, int64_t ldc,
                                                    const float* __restrict__ x_new, int64_t ldn,
                                                    float* u_cur, const float* __restrict__ u_new,
                                                    const float* __restrict__ k_cur,
                                                    const float* __restrict__ k_new,
                                                    const float* __restrict__ r, int32_t* naccept,
                                                    int64_t chains, int width, float beta) {
    NFK_ROW_PROLOGUE(W)
    for (int64_t r0 = wave * RPW; r0 < chains; r0 += nwave * RPW) {
        const int64_t c = r0 + sub;
        const bool ok = c < chains;
        int acc = 0;
        if (ok && c0 == 0) {
            const float un = u_new[c];
            float d = u_cur[c] - un;
            if (k_cur != nullptr) d = (d + k_cur[c]) - k_new[c];
            acc = r[c] < expf(d * beta) ? 1 : 0;  // a NaN exponent compares false: rejected
            if (acc) {
                u_cur[c] = un;
                if (naccept != nullptr) naccept[c] += 1;
            }
        }
        acc = __shfl(acc, sub * W, 64);
        if (ok && acc)
            for (int j = c0; j < width; j += W) x_cur[c * ldc + j] = x_new[c * ldn + j];
    }
}

int check_traj(const char* who, const void* x_in, int64_t ldxi, const void* v_in, int64_t ldvi,
               const void* x_out, int64_t ldxo, const void* v_out, int64_t ldvo, const void* pot,
               int64_t batch, int64_t width, int32_t path_len, int32_t scheme) {
    char buf[160];
    const char* why = nullptr;
    if (batch < 0) why = "bad batch";
    else if (path_len < 0) why = "path_len below zero";
    else if (scheme != 0 && scheme != 1) why = "scheme must be 0 (lagged force) or 1 (velocity Verlet)";
    else if (batch > 0 && (!x_in || !v_in || !x_out || !v_out || !pot)) why = "null pointer";
    else if (batch > 1 && (ldxi < width || ldvi < width || ldxo < width || ldvo < width))
        why = "leading dimension below the row width";
    if (why == nullptr) return 0;
    std::snprintf(buf, sizeof(buf), "%s: %s", who, why);
    return nfk_set_error(buf);
}

}  // namespace

// ---------------------------------------------------------------------------
// C ABI
// ---------------------------------------------------------------------------
extern "C" int nfk_einstein_trajectory(const float* x_in, int64_t ldxi, const float* v_in, int64_t ldvi,
                                       float* x_out, int64_t ldxo, float* v_out, int64_t ldvo,
                                       float* pot_out, int64_t batch, int32_t path_len, double dt,
                                       double dt_sq, int32_t scheme, const float* centers,
                                       int32_t natoms, int32_t dim, float scale, float half_log_det,
                                       int32_t has_box, double boxlength, nfk_stream_t stream) {
    if (natoms <= 0 || dim <= 0 || (int64_t)natoms * dim > (1 << 24) || !(scale > 0.0f))
        return nfk_set_error("nfk_einstein_trajectory: bad args");
    const int D = natoms * dim;
    if (check_traj("nfk_einstein_trajectory", x_in, ldxi, v_in, ldvi, x_out, ldxo, v_out, ldvo, pot_out,
                   batch, D, path_len, scheme))
        return NFK_EINVAL;
    if (batch == 0) return 0;
    if (!centers) return nfk_set_error("nfk_einstein_trajectory: null pointer");
    hipStream_t st = (hipStream_t)stream;
    const Step s = make_step(path_len, dt, dt_sq, scheme);
    const float c2pi = (float)(D * std::log(2.0 * M_PI));
    const float hld = (float)((double)natoms * (double)half_log_det);
    const float niv = (float)(-1.0 / ((double)scale * (double)scale));
    const float hb = (float)(0.5 * boxlength), lf = (float)boxlength;
    const int w = lanes_for(D);
    const unsigned g = grid_for_rows(batch, w);
#define CALL(W)                                                                                          \
    if (has_box)                                                                                         \
        hipLaunchKernelGGL((k_einstein_traj<W, true>), dim3(g), dim3(256), 0, st, x_in, ldxi, v_in, ldvi, \
                           centers, x_out, ldxo, v_out, ldvo, pot_out, batch, D, s, niv, scale, c2pi, hld, \
                           hb, lf);                                                                      \
    else                                                                                                 \
        hipLaunchKernelGGL((k_einstein_traj<W, false>), dim3(g), dim3(256), 0, st, x_in, ldxi, v_in, ldvi, \
                           centers, x_out, ldxo, v_out, ldvo, pot_out, batch, D, s, niv, scale, c2pi, hld, \
                           hb, lf);
    NFK_W_DISPATCH(w, CALL)
#undef CALL
    return launch_status("nfk_einstein_trajectory");
}

extern "C" int nfk_gmix_trajectory(const float* x_in, int64_t ldxi, const float* v_in, int64_t ldvi,
                                   float* x_out, int64_t ldxo, float* v_out, int64_t ldvo, float* pot_out,
                                   int64_t batch, int32_t path_len, double dt, double dt_sq,
                                   int32_t scheme, const float* centers, const float* scales,
                                   const float* hlds, int32_t npart, int32_t dim, int32_t ncenters,
                                   nfk_stream_t stream) {
    if (npart <= 0 || npart > (1 << 22)) return nfk_set_error("nfk_gmix_trajectory: bad sizes");
    if (!nfk_gmix_supported(ncenters, dim)) return nfk_set_error("nfk_gmix_trajectory: shape not supported");
    if (check_traj("nfk_gmix_trajectory", x_in, ldxi, v_in, ldvi, x_out, ldxo, v_out, ldvo, pot_out, batch,
                   (int64_t)npart * dim, path_len, scheme))
        return NFK_EINVAL;
    if (batch == 0) return 0;
    if (!centers || !scales || !hlds) return nfk_set_error("nfk_gmix_trajectory: null pointer");
    hipStream_t st = (hipStream_t)stream;
    const Step s = make_step(path_len, dt, dt_sq, scheme);
    const float inv_m = (float)(1.0 / ncenters);
    const float c2pi = (float)(dim * std::log(2.0 * M_PI));
    const int w = lanes_for(npart);
    const unsigned g = grid_for_rows(batch, w);
#define CALLD(W, DD)                                                                                  \
    hipLaunchKernelGGL((k_gmix_traj<W, DD>), dim3(g), dim3(256), 0, st, x_in, ldxi, v_in, ldvi, centers, \
                       scales, hlds, x_out, ldxo, v_out, ldvo, pot_out, batch, npart, ncenters, s, inv_m, \
                       c2pi)
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
    return launch_status("nfk_gmix_trajectory");
}

extern "C" int nfk_lj_trajectory(const float* x_in, int64_t ldxi, const float* v_in, int64_t ldvi,
                                 float* x_out, int64_t ldxo, float* v_out, int64_t ldvo, float* pot_out,
                                 int64_t batch, int32_t path_len, double dt, double dt_sq, int32_t scheme,
                                 int32_t n, int32_t dim, double boxlength, double sigma, double epsilon,
                                 int32_t has_cutoff, double cutoff, int32_t shift, nfk_stream_t stream) {
    if (!nfk_lj_supported(n, dim)) return nfk_set_error("nfk_lj_trajectory: shape not supported");
    if (has_cutoff && !(cutoff > 0.0)) return nfk_set_error("nfk_lj_trajectory: bad cutoff");
    if (check_traj("nfk_lj_trajectory", x_in, ldxi, v_in, ldvi, x_out, ldxo, v_out, ldvo, pot_out, batch,
                   (int64_t)n * dim, path_len, scheme))
        return NFK_EINVAL;
    if (batch == 0) return 0;
    hipStream_t st = (hipStream_t)stream;
    const Step s = make_step(path_len, dt, dt_sq, scheme);
    const LjConst k = lj_const(boxlength, sigma, epsilon, has_cutoff, cutoff, shift);
    const int G = lanes_for(n);
    const int ppl = (n + 63) / 64;
    const int rpb = 4 * (64 / G);
    int64_t grid = (batch + rpb - 1) / rpb;
    if (grid > 16384) grid = 16384;
    const size_t lds = (size_t)2 * rpb * n * sizeof(float4);  // two buffers per row, <= 32 KiB (n <= 256)
#define LJ_CALL2(GG, PP)                                                                                 \
    do {                                                                                                 \
        if (dim == 3)                                                                                    \
            hipLaunchKernelGGL((k_lj_traj<GG, PP, 3>), dim3((unsigned)grid), dim3(256), lds, st, x_in, ldxi, \
                               v_in, ldvi, x_out, ldxo, v_out, ldvo, pot_out, batch, n, s, k);           \
        else                                                                                             \
            hipLaunchKernelGGL((k_lj_traj<GG, PP, 2>), dim3((unsigned)grid), dim3(256), lds, st, x_in, ldxi, \
                               v_in, ldvi, x_out, ldxo, v_out, ldvo, pot_out, batch, n, s, k);           \
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
    return launch_status("nfk_lj_trajectory");
}

extern "C" int nfk_eam_trajectory(const float* x_in, int64_t ldxi, const float* v_in, int64_t ldvi,
                                  float* x_out, int64_t ldxo, float* v_out, int64_t ldvo, float* pot_out,
                                  int64_t batch, int32_t path_len, double dt, double dt_sq, int32_t scheme,
                                  int32_t n, const float* rtab, int32_t nr, double dr, const float* ftab,
                                  int32_t nrho, double drho, double f_end, double fp_end, double lx,
                                  double ly, double lz, double rc, nfk_stream_t stream) {
    if (!nfk_eam_supported(n)) return nfk_set_error("nfk_eam_trajectory: shape not supported");
    if (check_traj("nfk_eam_trajectory", x_in, ldxi, v_in, ldvi, x_out, ldxo, v_out, ldvo, pot_out, batch,
                   (int64_t)n * 3, path_len, scheme))
        return NFK_EINVAL;
    EamConst k;
    if (eam_setup("nfk_eam_trajectory", k, rtab, nr, dr, ftab, nrho, drho, f_end, fp_end, lx, ly, lz, rc))
        return NFK_EINVAL;
    if (batch == 0) return 0;
    if (!rtab || !ftab) return nfk_set_error("nfk_eam_trajectory: null pointer");
    hipStream_t st = (hipStream_t)stream;
    const Step s = make_step(path_len, dt, dt_sq, scheme);
    const int G = lanes_for(n);
    const int ppl = (n + 63) / 64;
    const int rpb = 4 * (64 / G);
    int64_t grid = (batch + rpb - 1) / rpb;
    if (grid > 16384) grid = 16384;
    const size_t lds = (size_t)2 * rpb * n * sizeof(float4);  // two buffers per row, <= 32 KiB (n <= 256)
#define EAM_CALL2(GG, PP)                                                                                   \
    hipLaunchKernelGGL((k_eam_traj<GG, PP>), dim3((unsigned)grid), dim3(256), lds, st, x_in, ldxi, v_in, ldvi, \
                       x_out, ldxo, v_out, ldvo, pot_out, batch, n, s, (const float4*)rtab,                 \
                       (const float4*)ftab, k)
#define EAM_CALL(W) EAM_CALL2(W, 1)
    if (ppl <= 1) {
        NFK_W_DISPATCH(G, EAM_CALL)
    } else if (ppl == 2) {
        EAM_CALL2(64, 2);
    } else if (ppl == 3) {
        EAM_CALL2(64, 3);
    } else {
        EAM_CALL2(64, 4);
    }
#undef EAM_CALL
#undef EAM_CALL2
    return launch_status("nfk_eam_trajectory");
}

extern "C" int nfk_hmc_accept(float* x_cur, int64_t ldc, const float* x_new, int64_t ldn, float* u_cur,
                              const float* u_new, const float* k_cur, const float* k_new, const float* r,
                              int32_t* naccept, int64_t chains, int32_t width, double beta,
                              nfk_stream_t stream) {
    if (chains < 0 || width <= 0 || width > (1 << 24)) return nfk_set_error("nfk_hmc_accept: bad sizes");
    if (chains == 0) return 0;
    if (!x_cur || !x_new || !u_cur || !u_new || !r) return nfk_set_error("nfk_hmc_accept: null pointer");
    if ((k_cur == nullptr) != (k_new == nullptr))
        return nfk_set_error("nfk_hmc_accept: k_cur and k_new come together");
    if (chains > 1 && (ldc < width || ldn < width))
        return nfk_set_error("nfk_hmc_accept: leading dimension below the row width");
    const int w = lanes_for(width);
    const unsigned g = grid_for_rows(chains, w);
#define CALL(W)                                                                                        \
    hipLaunchKernelGGL((k_hmc_accept<W>), dim3(g), dim3(256), 0, (hipStream_t)stream, x_cur, ldc, x_new, \
                       ldn, u_cur, u_new, k_cur, k_new, r, naccept, chains, width, (float)beta);
    NFK_W_DISPATCH(w, CALL)
#undef CALL
    return launch_status("nfk_hmc_accept");
}
