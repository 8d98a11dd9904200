// nfk_langevin.hip -- thermostatted (NVT) trajectories of the applications layer's
// systems in ONE launch per chunk of steps, and the fill kernel of the device
// random numbers.  The integrator is BAOAB (Leimkuhler & Matthews, 2013) with the
// noise generated where it is used (nfk_rng.h: Philox4x32-10 keyed by the
// absolute step, the particle and the row, so a result never depends on the
// launch geometry or on how a run is cut into launches).  The kernels follow
// nfk_dynamics.hip: the same mappings, x, v and F in registers, two LDS row
// buffers, every __syncthreads in block-uniform control flow; the forces and
// the potentials are the device functions of nfk_systems_dev.h.  VALU kernels:
// no MFMA, no atomics, plain vector stores, every sum in a fixed order,
// -ffp-contract=off.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdio>

#include "../../include/nfk.h"
#include "nfk_systems_dev.h"
#include "nfk_rng.h"

namespace {

// The constants of a call.  Per step k < nsteps, in fp32 and in this order:
//   v = v + hb*F;  x = x + hd*v;  v = c1*v + c2*xi(step0 + k);  x = x + hd*v;
//   F = force(x);  v = v + hb*F
// A frame is written after every step with (step0 + k + 1) % record_every == 0,
// frame (step0 + k + 1) / record_every - 1 - frame0 of this call's records.
struct Lv {
    float hb, hd, c1, c2;
    int nsteps, record_every;
    uint64_t step0;
    int64_t frame0;  // step0 / record_every
};

__device__ __forceinline__ void lv_first_half(float& x, float& v, float F, float xi, const Lv& s) {
    v = v + s.hb * F;
    x = x + s.hd * v;
    v = s.c1 * v + s.c2 * xi;
    x = x + s.hd * v;
}

__device__ __forceinline__ float lv_last_kick(float v, float F, const Lv& s) { return v + s.hb * F; }

// -1, or the frame of this call's records that step k closes
__device__ __forceinline__ int64_t lv_frame(const Lv& s, int k) {
    if (s.record_every <= 0) return -1;
    const uint64_t done = s.step0 + (uint64_t)k + 1;
    if (done % (uint64_t)s.record_every != 0) return -1;
    return (int64_t)(done / (uint64_t)s.record_every) - 1 - s.frame0;
}

__device__ __forceinline__ float pick4(const float (&z)[4], int d) {
    return d == 0 ? z[0] : d == 1 ? z[1] : d == 2 ? z[2] : z[3];
}

// ---------------------------------------------------------------------------
// nfk_philox_fill
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_fill_words(int32_t* out, int64_t rows, int n, uint64_t step, RngKey key) {
    const int64_t tot = rows * n;
    for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < tot;
         t += (int64_t)gridDim.x * blockDim.x) {
        const int64_t b = t / n;
        const int p = (int)(t - b * n);
        const Words4 o = rng_words(key, step, (uint32_t)p, key.row_base + (uint32_t)b);
#pragma unroll
        for (int d = 0; d < 4; ++d) out[t * 4 + d] = (int32_t)o.w[d];
    }
}

__global__ __launch_bounds__(256) void k_fill_normal(float* out, int64_t rows, int n, int dim, uint64_t step,
                                                     RngKey key) {
    const int64_t tot = rows * n;
    for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < tot;
         t += (int64_t)gridDim.x * blockDim.x) {
        const int64_t b = t / n;
        const int p = (int)(t - b * n);
        float z[4];
        rng_normal4(key, step, (uint32_t)p, key.row_base + (uint32_t)b, z);
        for (int d = 0; d < dim; ++d) out[t * dim + d] = pick4(z, d);
    }
}

// zero_mean: the rows on G = lanes_for(n) lanes, as the kernels that consume the values
template <int G>
__global__ __launch_bounds__(256) void k_fill_normal_zm(float* out, int64_t rows, int n, int dim, uint64_t step,
                                                        RngKey key) {
    NFK_ROW_PROLOGUE(G)
    for (int64_t r0 = wave * RPW; r0 < rows; r0 += nwave * RPW) {
        const int64_t b = r0 + sub;
        const bool ok = b < rows;
        const uint32_t row = key.row_base + (uint32_t)b;
        float mean[4], z[4];
        rng_row_mean<G>(key, step, row, n, c0, mean);
        if (ok)
            for (int p = c0; p < n; p += G) {
                rng_normal4(key, step, (uint32_t)p, row, z);
                for (int d = 0; d < dim; ++d) out[(b * n + p) * dim + d] = pick4(z, d) - pick4(mean, d);
            }
    }
}

// ---------------------------------------------------------------------------
// Einstein crystal: k_einstein_traj's mapping, a coordinate per lane (component
// c % dim of atom c / dim), W coordinates of a row per pass.  The passes are
// walked by every lane of the group, so the shuffles of the noise mean and of
// the closing sums see the whole wave.  The recorded potentials are row sums
// over all passes: they are summed afterwards from the frames, each lane reading
// back the coordinates it wrote itself.
// ---------------------------------------------------------------------------
template <int W, bool BOX>
__global__ __launch_bounds__(256) void k_einstein_lv(const float* x_in, int64_t ldxi, const float* v_in,
                                                     int64_t ldvi, const float* __restrict__ cen, float* x_out,
                                                     int64_t ldxo, float* v_out, int64_t ldvo,
                                                     float* __restrict__ pot, int64_t batch, int D, int dim,
                                                     int natoms, int glanes, Lv s, RngKey key, float* pos_rec,
                                                     float* pot_rec, int64_t nframes, float neg_inv_var,
                                                     float lii, float c2pi, float hld, float hb, float lf) {
    NFK_ROW_PROLOGUE(W)
    for (int64_t r0 = wave * RPW; r0 < batch; r0 += nwave * RPW) {
        const int64_t b = r0 + sub;
        const bool ok = b < batch;
        const uint32_t row = key.row_base + (uint32_t)b;
        float m = 0.0f;
        for (int cb = 0; cb < D; cb += W) {
            const int c = cb + c0;
            const bool live = ok && c < D;
            const int atom = c / dim, comp = c - atom * dim;
            const float cc = live ? cen[c] : 0.0f;
            float x = live ? x_in[b * ldxi + c] : 0.0f, v = live ? v_in[b * ldvi + c] : 0.0f;
            float F = einstein_dlp(einstein_dev<BOX>(x, cc, hb, lf), neg_inv_var);
            for (int k = 0; k < s.nsteps; ++k) {
                const uint64_t step = s.step0 + (uint64_t)k;
                float mean[4] = {0.0f, 0.0f, 0.0f, 0.0f}, z[4];
                if (key.zero_mean) rng_row_mean_in<W>(key, step, row, natoms, glanes, c0, mean);
                rng_normal4(key, step, (uint32_t)atom, row, z);
                float xi = pick4(z, comp);
                if (key.zero_mean) xi = xi - pick4(mean, comp);
                lv_first_half(x, v, F, xi, s);
                F = einstein_dlp(einstein_dev<BOX>(x, cc, hb, lf), neg_inv_var);
                v = lv_last_kick(v, F, s);
                const int64_t fr = lv_frame(s, k);
                if (fr >= 0 && live && pos_rec != nullptr) pos_rec[(fr * batch + b) * D + c] = x;
            }
            if (live) {
                x_out[b * ldxo + c] = x;
                v_out[b * ldvo + c] = v;
                const float y = einstein_dev<BOX>(x, cc, hb, lf) / lii;
                m += y * y;
            }
        }
        m = group_sum<W>(m);
        if (ok && c0 == 0) pot[b] = -(-0.5f * (c2pi + m) - hld);
        if (pos_rec != nullptr)
            for (int64_t fr = 0; fr < nframes; ++fr) {
                float mf = 0.0f;
                if (ok)
                    for (int c = c0; c < D; c += W) {
                        const float y = einstein_dev<BOX>(pos_rec[(fr * batch + b) * D + c], cen[c], hb, lf) / lii;
                        mf += y * y;
                    }
                mf = group_sum<W>(mf);
                if (ok && c0 == 0) pot_rec[fr * batch + b] = -(-0.5f * (c2pi + mf) - hld);
            }
    }
}

// ---------------------------------------------------------------------------
// Gaussian mixture: k_gmix_traj's mapping, a particle per lane, W particles of a
// row per pass; passes and recorded potentials as in k_einstein_lv.
// ---------------------------------------------------------------------------
template <int W, int DIM>
__global__ __launch_bounds__(256) void k_gmix_lv(const float* x_in, int64_t ldxi, const float* v_in, int64_t ldvi,
                                                 const float* __restrict__ cen, const float* __restrict__ scales,
                                                 const float* __restrict__ hlds, float* x_out, int64_t ldxo,
                                                 float* v_out, int64_t ldvo, float* __restrict__ pot,
                                                 int64_t batch, int npart, int M, Lv s, RngKey key,
                                                 float* pos_rec, float* pot_rec, int64_t nframes, float inv_m,
                                                 float c2pi) {
    NFK_ROW_PROLOGUE(W)
    const int64_t width = (int64_t)npart * DIM;
    for (int64_t r0 = wave * RPW; r0 < batch; r0 += nwave * RPW) {
        const int64_t b = r0 + sub;
        const bool ok = b < batch;
        const uint32_t row = key.row_base + (uint32_t)b;
        float acc = 0.0f;
        for (int pb = 0; pb < npart; pb += W) {
            const int p = pb + c0;
            const bool live = ok && p < npart;
            float x[DIM], v[DIM], F[DIM];
#pragma unroll
            for (int d = 0; d < DIM; ++d) {
                x[d] = live ? x_in[b * ldxi + p * DIM + d] : 0.0f;
                v[d] = live ? v_in[b * ldvi + p * DIM + d] : 0.0f;
            }
            gmix_dlp<DIM>(x, cen, scales, hlds, M, inv_m, c2pi, F);
            for (int k = 0; k < s.nsteps; ++k) {
                const uint64_t step = s.step0 + (uint64_t)k;
                float mean[4] = {0.0f, 0.0f, 0.0f, 0.0f}, z[4];
                if (key.zero_mean) rng_row_mean<W>(key, step, row, npart, c0, mean);
                rng_normal4(key, step, (uint32_t)p, row, z);
#pragma unroll
                for (int d = 0; d < DIM; ++d) {
                    const float xi = key.zero_mean ? z[d] - mean[d] : z[d];
                    lv_first_half(x[d], v[d], F[d], xi, s);
                }
                gmix_dlp<DIM>(x, cen, scales, hlds, M, inv_m, c2pi, F);
#pragma unroll
                for (int d = 0; d < DIM; ++d) v[d] = lv_last_kick(v[d], F[d], s);
                const int64_t fr = lv_frame(s, k);
                if (fr >= 0 && live && pos_rec != nullptr) {
#pragma unroll
                    for (int d = 0; d < DIM; ++d) pos_rec[(fr * batch + b) * width + p * DIM + d] = x[d];
                }
            }
            if (live) {
#pragma unroll
                for (int d = 0; d < DIM; ++d) {
                    x_out[b * ldxo + p * DIM + d] = x[d];
                    v_out[b * ldvo + p * DIM + d] = v[d];
                }
                acc += logf(gmix_prob<DIM>(x, cen, scales, hlds, M, inv_m, c2pi));
            }
        }
        acc = group_sum<W>(acc);
        if (ok && c0 == 0) pot[b] = -acc;
        if (pos_rec != nullptr)
            for (int64_t fr = 0; fr < nframes; ++fr) {
                float af = 0.0f;
                if (ok)
                    for (int p = c0; p < npart; p += W) {
                        float xv[DIM];
#pragma unroll
                        for (int d = 0; d < DIM; ++d) xv[d] = pos_rec[(fr * batch + b) * width + p * DIM + d];
                        af += logf(gmix_prob<DIM>(xv, cen, scales, hlds, M, inv_m, c2pi));
                    }
                af = group_sum<W>(af);
                if (ok && c0 == 0) pot_rec[fr * batch + b] = -af;
            }
    }
}

// The noise of the lane's particles c0 + q G, q < PPL, for one step: normal d of
// each particle, less the row's mean under zero_mean (rng_row_mean's sums: the
// lane's own particles in ascending order, the butterfly, the division by n).
// Every lane of the wave calls it.
template <int G, int PPL>
__device__ __forceinline__ void lv_noise(const RngKey& key, uint64_t step, uint32_t row, int n, int c0,
                                         float (&z)[PPL][4]) {
    float sum[4] = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
    for (int q = 0; q < PPL; ++q) {
        const int i = c0 + q * G;
        z[q][0] = z[q][1] = z[q][2] = z[q][3] = 0.0f;
        if (i < n) {
            rng_normal4(key, step, (uint32_t)i, row, z[q]);
#pragma unroll
            for (int d = 0; d < 4; ++d) sum[d] += z[q][d];
        }
    }
    if (key.zero_mean) {
        const float fn = (float)n;
#pragma unroll
        for (int d = 0; d < 4; ++d) {
            const float mean = group_sum<G>(sum[d]) / fn;
#pragma unroll
            for (int q = 0; q < PPL; ++q) z[q][d] = z[q][d] - mean;
        }
    }
}

// ---------------------------------------------------------------------------
// Lennard-Jones: k_lj_traj's mapping and its two LDS buffers per row.  A step
// stages the new positions in the row's other buffer, so it needs one barrier.
// nsteps and the record schedule are kernel-uniform and rows past `batch` walk
// the barriers without touching memory.
// ---------------------------------------------------------------------------
template <int G, int PPL, int DIM>
__global__ __launch_bounds__(256) void k_lj_lv(const float* x_in, int64_t ldxi, const float* v_in, int64_t ldvi,
                                               float* x_out, int64_t ldxo, float* v_out, int64_t ldvo,
                                               float* __restrict__ pot, int64_t batch, int n, Lv s, RngKey key,
                                               float* pos_rec, float* pot_rec, LjConst k) {
    extern __shared__ __attribute__((aligned(16))) float4 s_pos[];
    constexpr int RPW = 64 / G, RPB = 4 * RPW;
    const int lane = threadIdx.x & 63;
    const int rb = (threadIdx.x >> 6) * RPW + lane / G;  // row within the block
    const int c0 = lane % G;
    float4* srow = s_pos + (size_t)rb * n;  // buffer 0; buffer 1 lies RPB rows further on
    const int other = RPB * n;
    const int64_t width = (int64_t)n * DIM;
    for (int64_t r0 = (int64_t)blockIdx.x * RPB; r0 < batch; r0 += (int64_t)gridDim.x * RPB) {
        const int64_t b = r0 + rb;
        const bool ok = b < batch;
        const uint32_t row = key.row_base + (uint32_t)b;
        float x[PPL][3], v[PPL][3], F[PPL][3], f[PPL][3], z[PPL][4];
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
        for (int st = 0; st < s.nsteps; ++st) {
            lv_noise<G, PPL>(key, s.step0 + (uint64_t)st, row, n, c0, z);
#pragma unroll
            for (int q = 0; q < PPL; ++q)
#pragma unroll
                for (int d = 0; d < DIM; ++d) lv_first_half(x[q][d], v[q][d], F[q][d], z[q][d], s);
#pragma unroll
            for (int q = 0; q < PPL; ++q) {
                const int i = c0 + q * G;
                if (ok && i < n) srow[(cur ^ 1) * other + i] = make_float4(x[q][0], x[q][1], x[q][2], 0.0f);
            }
            __syncthreads();
            cur ^= 1;
            if (ok) lj_row<G, PPL, DIM, true>(x, srow + cur * other, n, c0, k, f);
#pragma unroll
            for (int q = 0; q < PPL; ++q)
#pragma unroll
                for (int d = 0; d < DIM; ++d) {
                    F[q][d] = ok ? -f[q][d] : 0.0f;
                    v[q][d] = lv_last_kick(v[q][d], F[q][d], s);
                }
            const int64_t fr = lv_frame(s, st);
            if (fr >= 0 && pos_rec != nullptr) {  // kernel-uniform
                float e = 0.0f;
                if (ok) {
                    e = lj_row<G, PPL, DIM, false>(x, srow + cur * other, n, c0, k, f);
#pragma unroll
                    for (int q = 0; q < PPL; ++q) {
                        const int i = c0 + q * G;
                        if (i < n) {
                            float* px = pos_rec + (fr * batch + b) * width + (int64_t)i * DIM;
#pragma unroll
                            for (int d = 0; d < DIM; ++d) px[d] = x[q][d];
                        }
                    }
                }
                e = group_sum<G>(e);
                if (ok && c0 == 0) pot_rec[fr * batch + b] = e / 2.0f;
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
// Embedded-atom model: k_eam_traj's mapping; a step has two barriers, the one
// after the new positions are staged and the one inside eam_row_step_force.
// ---------------------------------------------------------------------------
template <int G, int PPL>
__global__ __launch_bounds__(256) void k_eam_lv(const float* x_in, int64_t ldxi, const float* v_in, int64_t ldvi,
                                                float* x_out, int64_t ldxo, float* v_out, int64_t ldvo,
                                                float* __restrict__ pot, int64_t batch, int n, Lv s, RngKey key,
                                                float* pos_rec, float* pot_rec,
                                                const float4* __restrict__ rtab,
                                                const float4* __restrict__ ftab, EamConst k) {
    extern __shared__ __attribute__((aligned(16))) float4 s_pos[];
    constexpr int RPW = 64 / G, RPB = 4 * RPW;
    const int lane = threadIdx.x & 63;
    const int rb = (threadIdx.x >> 6) * RPW + lane / G;  // row within the block
    const int c0 = lane % G;
    float4* srow = s_pos + (size_t)rb * n;  // buffer 0; buffer 1 lies RPB rows further on
    const int other = RPB * n;
    const int64_t width = (int64_t)n * 3;
    for (int64_t r0 = (int64_t)blockIdx.x * RPB; r0 < batch; r0 += (int64_t)gridDim.x * RPB) {
        const int64_t b = r0 + rb;
        const bool ok = b < batch;
        const uint32_t row = key.row_base + (uint32_t)b;
        float x[PPL][3], v[PPL][3], F[PPL][3], z[PPL][4];
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
        for (int st = 0; st < s.nsteps; ++st) {
            lv_noise<G, PPL>(key, s.step0 + (uint64_t)st, row, n, c0, z);
#pragma unroll
            for (int q = 0; q < PPL; ++q)
#pragma unroll
                for (int d = 0; d < 3; ++d) lv_first_half(x[q][d], v[q][d], F[q][d], z[q][d], s);
#pragma unroll
            for (int q = 0; q < PPL; ++q) {
                const int i = c0 + q * G;
                if (ok && i < n) srow[(cur ^ 1) * other + i] = make_float4(x[q][0], x[q][1], x[q][2], 0.0f);
            }
            __syncthreads();
            cur ^= 1;
            eam_row_step_force<G, PPL>(ok, x, srow + cur * other, n, c0, k, rtab, ftab, F);
#pragma unroll
            for (int q = 0; q < PPL; ++q)
#pragma unroll
                for (int d = 0; d < 3; ++d) v[q][d] = lv_last_kick(v[q][d], F[q][d], s);
            const int64_t fr = lv_frame(s, st);
            if (fr >= 0 && pos_rec != nullptr) {  // kernel-uniform
                float e = 0.0f;
                if (ok) {
                    e = eam_row_energy<G, PPL>(x, srow + cur * other, n, c0, k, rtab, ftab);
#pragma unroll
                    for (int q = 0; q < PPL; ++q) {
                        const int i = c0 + q * G;
                        if (i < n) {
                            float* px = pos_rec + (fr * batch + b) * width + (int64_t)i * 3;
#pragma unroll
                            for (int d = 0; d < 3; ++d) px[d] = x[q][d];
                        }
                    }
                }
                e = group_sum<G>(e);
                if (ok && c0 == 0) pot_rec[fr * batch + b] = e;
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

const int64_t ROWS_MAX = (int64_t)1 << 32;

int check_seed(const char* who, int64_t seed, int64_t row_base, int64_t rows, int64_t step) {
    char buf[160];
    const char* why = nullptr;
    if (seed < 0) why = "seed must be in [0, 2^63)";
    else if (step < 0) why = "step below zero";
    else if (rows < 0) why = "bad batch";
    else if (row_base < 0 || row_base > ROWS_MAX || rows > ROWS_MAX - row_base)
        why = "row_base + rows must stay below 2^32";
    if (why == nullptr) return 0;
    std::snprintf(buf, sizeof(buf), "%s: %s", who, why);
    return nfk_set_error(buf);
}

// check_traj's checks for a Langevin call; fills s and key
int check_lv(const char* who, const void* x_in, int64_t ldxi, const void* v_in, int64_t ldvi, const void* x_out,
             int64_t ldxo, const void* v_out, int64_t ldvo, const void* pot, int64_t batch, int64_t width,
             int32_t nsteps, int64_t step0, int64_t row_base, int64_t seed, int32_t zero_mean, float hb, float hd,
             float c1, float c2, int32_t record_every, const void* pos_rec, const void* pot_rec, Lv& s,
             RngKey& key, int64_t& nframes) {
    char buf[160];
    const char* why = nullptr;
    if (nsteps < 0) why = "nsteps below zero";
    else if (record_every < 0) why = "record_every below zero";
    else if ((pos_rec == nullptr) != (pot_rec == nullptr)) why = "pos_rec and pot_rec come together";
    else if (batch > 0 && (!x_in || !v_in || !x_out || !v_out || !pot)) why = "null pointer";
    else if (batch > 1 && (ldxi < width || ldvi < width || ldxo < width || ldvo < width))
        why = "leading dimension below the row width";
    if (why != nullptr) {
        std::snprintf(buf, sizeof(buf), "%s: %s", who, why);
        return nfk_set_error(buf);
    }
    if (check_seed(who, seed, row_base, batch, step0)) return NFK_EINVAL;
    s.hb = hb;
    s.hd = hd;
    s.c1 = c1;
    s.c2 = c2;
    s.nsteps = nsteps;
    s.record_every = record_every;
    s.step0 = (uint64_t)step0;
    s.frame0 = record_every > 0 ? step0 / record_every : 0;
    nframes = record_every > 0 && pos_rec != nullptr ? (step0 + nsteps) / record_every - s.frame0 : 0;
    key = rng_key(seed, 0, row_base, zero_mean);
    return 0;
}

}  // namespace

// ---------------------------------------------------------------------------
// C ABI
// ---------------------------------------------------------------------------
extern "C" int nfk_philox_fill(void* out, int32_t normals, int64_t rows, int32_t n, int32_t dim, int64_t step,
                               int64_t row_base, int64_t seed, int32_t tag, int32_t zero_mean,
                               nfk_stream_t stream) {
    if (n <= 0 || n > (1 << 24)) return nfk_set_error("nfk_philox_fill: bad sizes");
    if (normals && (dim < 1 || dim > 4)) return nfk_set_error("nfk_philox_fill: dim must be 1..4");
    if (tag != 0 && tag != 1) return nfk_set_error("nfk_philox_fill: tag must be 0 or 1");
    if (!normals && zero_mean) return nfk_set_error("nfk_philox_fill: zero_mean needs normals");
    if (check_seed("nfk_philox_fill", seed, row_base, rows, step)) return NFK_EINVAL;
    if (rows == 0) return 0;
    if (!out) return nfk_set_error("nfk_philox_fill: null pointer");
    hipStream_t st = (hipStream_t)stream;
    const RngKey key = rng_key(seed, tag, row_base, zero_mean);
    if (!normals) {
        hipLaunchKernelGGL(k_fill_words, dim3(grid_for(rows * n, 256)), dim3(256), 0, st, (int32_t*)out, rows, n,
                           (uint64_t)step, key);
    } else if (!zero_mean) {
        hipLaunchKernelGGL(k_fill_normal, dim3(grid_for(rows * n, 256)), dim3(256), 0, st, (float*)out, rows, n,
                           dim, (uint64_t)step, key);
    } else {
        const int w = lanes_for(n);
        const unsigned g = grid_for_rows(rows, w);
#define CALL(W)                                                                                              \
    hipLaunchKernelGGL((k_fill_normal_zm<W>), dim3(g), dim3(256), 0, st, (float*)out, rows, n, dim, (uint64_t)step, \
                       key);
        NFK_W_DISPATCH(w, CALL)
#undef CALL
    }
    return launch_status("nfk_philox_fill");
}

#define LV_ARGS_CHECK(who, width)                                                                               \
    Lv s;                                                                                                       \
    RngKey key;                                                                                                 \
    int64_t nframes = 0;                                                                                        \
    if (check_lv(who, x_in, ldxi, v_in, ldvi, x_out, ldxo, v_out, ldvo, pot_out, batch, width, nsteps, step0,   \
                 row_base, seed, zero_mean, hb, hd, c1, c2, record_every, pos_rec, pot_rec, s, key, nframes))   \
        return NFK_EINVAL;

extern "C" int nfk_einstein_langevin(const float* x_in, int64_t ldxi, const float* v_in, int64_t ldvi,
                                     float* x_out, int64_t ldxo, float* v_out, int64_t ldvo, float* pot_out,
                                     int64_t batch, int32_t nsteps, int64_t step0, int64_t row_base, int64_t seed,
                                     int32_t zero_mean, float hb, float hd, float c1, float c2,
                                     int32_t record_every, float* pos_rec, float* pot_rec, const float* centers,
                                     int32_t natoms, int32_t dim, float scale, float half_log_det,
                                     int32_t has_box, double boxlength, nfk_stream_t stream) {
    if (natoms <= 0 || dim <= 0 || (int64_t)natoms * dim > (1 << 24) || !(scale > 0.0f))
        return nfk_set_error("nfk_einstein_langevin: bad args");
    if (dim > 4) return nfk_set_error("nfk_einstein_langevin: shape not supported (dim > 4)");
    const int D = natoms * dim;
    LV_ARGS_CHECK("nfk_einstein_langevin", D)
    if (batch == 0) return 0;
    if (!centers) return nfk_set_error("nfk_einstein_langevin: null pointer");
    hipStream_t st = (hipStream_t)stream;
    const float c2pi = (float)(D * std::log(2.0 * M_PI));
    const float hld = (float)((double)natoms * (double)half_log_det);
    const float niv = (float)(-1.0 / ((double)scale * (double)scale));
    const float hbox = (float)(0.5 * boxlength), lf = (float)boxlength;
    const int w = lanes_for(D), gl = lanes_for(natoms);
    const unsigned g = grid_for_rows(batch, w);
#define CALLB(W, BOX)                                                                                          \
    hipLaunchKernelGGL((k_einstein_lv<W, BOX>), dim3(g), dim3(256), 0, st, x_in, ldxi, v_in, ldvi, centers, x_out, \
                       ldxo, v_out, ldvo, pot_out, batch, D, dim, natoms, gl, s, key, pos_rec, pot_rec, nframes, \
                       niv, scale, c2pi, hld, hbox, lf)
#define CALL(W)            \
    if (has_box)           \
        CALLB(W, true);    \
    else                   \
        CALLB(W, false);
    NFK_W_DISPATCH(w, CALL)
#undef CALL
#undef CALLB
    return launch_status("nfk_einstein_langevin");
}

extern "C" int nfk_gmix_langevin(const float* x_in, int64_t ldxi, const float* v_in, int64_t ldvi, float* x_out,
                                 int64_t ldxo, float* v_out, int64_t ldvo, float* pot_out, int64_t batch,
                                 int32_t nsteps, int64_t step0, int64_t row_base, int64_t seed, int32_t zero_mean,
                                 float hb, float hd, float c1, float c2, int32_t record_every, float* pos_rec,
                                 float* pot_rec, const float* centers, const float* scales, const float* hlds,
                                 int32_t npart, int32_t dim, int32_t ncenters, nfk_stream_t stream) {
    if (npart <= 0 || npart > (1 << 22)) return nfk_set_error("nfk_gmix_langevin: bad sizes");
    if (!nfk_gmix_supported(ncenters, dim)) return nfk_set_error("nfk_gmix_langevin: shape not supported");
    LV_ARGS_CHECK("nfk_gmix_langevin", (int64_t)npart * dim)
    if (batch == 0) return 0;
    if (!centers || !scales || !hlds) return nfk_set_error("nfk_gmix_langevin: null pointer");
    hipStream_t st = (hipStream_t)stream;
    const float inv_m = (float)(1.0 / ncenters);
    const float c2pi = (float)(dim * std::log(2.0 * M_PI));
    const int w = lanes_for(npart);
    const unsigned g = grid_for_rows(batch, w);
#define CALLD(W, DD)                                                                                           \
    hipLaunchKernelGGL((k_gmix_lv<W, DD>), dim3(g), dim3(256), 0, st, x_in, ldxi, v_in, ldvi, centers, scales,  \
                       hlds, x_out, ldxo, v_out, ldvo, pot_out, batch, npart, ncenters, s, key, pos_rec, pot_rec, \
                       nframes, inv_m, c2pi)
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
    return launch_status("nfk_gmix_langevin");
}

extern "C" int nfk_lj_langevin(const float* x_in, int64_t ldxi, const float* v_in, int64_t ldvi, float* x_out,
                               int64_t ldxo, float* v_out, int64_t ldvo, float* pot_out, int64_t batch,
                               int32_t nsteps, int64_t step0, int64_t row_base, int64_t seed, int32_t zero_mean,
                               float hb, float hd, float c1, float c2, int32_t record_every, float* pos_rec,
                               float* pot_rec, int32_t n, int32_t dim, double boxlength, double sigma,
                               double epsilon, int32_t has_cutoff, double cutoff, int32_t shift,
                               nfk_stream_t stream) {
    if (!nfk_lj_supported(n, dim)) return nfk_set_error("nfk_lj_langevin: shape not supported");
    if (has_cutoff && !(cutoff > 0.0)) return nfk_set_error("nfk_lj_langevin: bad cutoff");
    LV_ARGS_CHECK("nfk_lj_langevin", (int64_t)n * dim)
    if (batch == 0) return 0;
    hipStream_t st = (hipStream_t)stream;
    const LjConst k = lj_const(boxlength, sigma, epsilon, has_cutoff, cutoff, shift);
    const int G = lanes_for(n);
    const int ppl = (n + 63) / 64;
    const int rpb = 4 * (64 / G);
    int64_t grid = (batch + rpb - 1) / rpb;
    if (grid > 16384) grid = 16384;
    const size_t lds = (size_t)2 * rpb * n * sizeof(float4);  // two buffers per row, <= 32 KiB (n <= 256)
#define LJ_CALL2(GG, PP)                                                                                       \
    do {                                                                                                       \
        if (dim == 3)                                                                                          \
            hipLaunchKernelGGL((k_lj_lv<GG, PP, 3>), dim3((unsigned)grid), dim3(256), lds, st, x_in, ldxi, v_in, \
                               ldvi, x_out, ldxo, v_out, ldvo, pot_out, batch, n, s, key, pos_rec, pot_rec, k); \
        else                                                                                                   \
            hipLaunchKernelGGL((k_lj_lv<GG, PP, 2>), dim3((unsigned)grid), dim3(256), lds, st, x_in, ldxi, v_in, \
                               ldvi, x_out, ldxo, v_out, ldvo, pot_out, batch, n, s, key, pos_rec, pot_rec, k); \
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
    return launch_status("nfk_lj_langevin");
}

extern "C" int nfk_eam_langevin(const float* x_in, int64_t ldxi, const float* v_in, int64_t ldvi, float* x_out,
                                int64_t ldxo, float* v_out, int64_t ldvo, float* pot_out, int64_t batch,
                                int32_t nsteps, int64_t step0, int64_t row_base, int64_t seed, int32_t zero_mean,
                                float hb, float hd, float c1, float c2, int32_t record_every, float* pos_rec,
                                float* pot_rec, int32_t n, const float* rtab, int32_t nr, double dr,
                                const float* ftab, int32_t nrho, double drho, double f_end, double fp_end,
                                double lx, double ly, double lz, double rc, nfk_stream_t stream) {
    if (!nfk_eam_supported(n)) return nfk_set_error("nfk_eam_langevin: shape not supported");
    LV_ARGS_CHECK("nfk_eam_langevin", (int64_t)n * 3)
    EamConst k;
    if (eam_setup("nfk_eam_langevin", k, rtab, nr, dr, ftab, nrho, drho, f_end, fp_end, lx, ly, lz, rc))
        return NFK_EINVAL;
    if (batch == 0) return 0;
    if (!rtab || !ftab) return nfk_set_error("nfk_eam_langevin: null pointer");
    hipStream_t st = (hipStream_t)stream;
    const int G = lanes_for(n);
    const int ppl = (n + 63) / 64;
    const int rpb = 4 * (64 / G);
    int64_t grid = (batch + rpb - 1) / rpb;
    if (grid > 16384) grid = 16384;
    const size_t lds = (size_t)2 * rpb * n * sizeof(float4);  // two buffers per row, <= 32 KiB (n <= 256)
#define EAM_CALL2(GG, PP)                                                                                       \
    hipLaunchKernelGGL((k_eam_lv<GG, PP>), dim3((unsigned)grid), dim3(256), lds, st, x_in, ldxi, v_in, ldvi, x_out, \
                       ldxo, v_out, ldvo, pot_out, batch, n, s, key, pos_rec, pot_rec, (const float4*)rtab,     \
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
    return launch_status("nfk_eam_langevin");
}
