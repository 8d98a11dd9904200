// nfk_hmc_run.hip -- a whole HMC run of the applications layer's systems in ONE
// launch: all `epochs` moves of every chain (nf/hmc.py:50-63), the velocity and
// uniform draws read from tensors that torch filled beforehand.  A chain's
// position, potential and acceptance count stay on chip across the epoch loop.
// An epoch is nfk_*_trajectory's arithmetic (step_x / step_v of nfk_step.h, the
// forces and closing potentials of nfk_systems_dev.h, the same group_sum tree)
// followed by k_hmc_accept's decision, so a run has the bits of the chain of
// per-epoch launches it replaces; the one exception is the kinetic energy of
// hamiltonian runs, summed here in the kernel (nfk.h).  VALU kernels: no MFMA,
// no atomics, nothing between workgroups, -ffp-contract=off.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdio>

#include "../../include/nfk.h"
#include "nfk_step.h"
#include "nfk_systems_dev.h"

namespace {

// What every system's run shares.  W is the row width in floats.
struct HmcRun {
    float* x_cur;            // [chains, W], row stride ldx: start state in, final state out
    int64_t ldx;
    float* u_cur;            // [chains]
    int32_t* naccept;        // [chains] or null
    const float* v_draws;    // [epochs, chains, W] dense
    const float* r;          // [epochs, chains]
    float* v_last;           // [chains, W], row stride ldv, or null
    int64_t ldv;
    float* pos_rec;          // [epochs, chains, W] dense or null
    float* pot_rec;          // [epochs, chains] or null (with pos_rec)
    int64_t chains;
    int epochs;
    int hamiltonian;
    float beta;
};

// k_hmc_accept's test: r < expf(((u_cur - u_new) [+ k_cur) - k_new] * beta); a NaN rejects
__device__ __forceinline__ int hmc_decide(float u_cur, float u_new, float k_cur, float k_new, float r,
                                          float beta, int hamiltonian) {
    float d = u_cur - u_new;
    if (hamiltonian) d = (d + k_cur) - k_new;
    return r < expf(d * beta) ? 1 : 0;
}

// ---------------------------------------------------------------------------
// Einstein crystal: a chain on W lanes, lane c0 keeps coordinates c0 + q W,
// q < NPL, in registers for the whole run.
// ---------------------------------------------------------------------------
template <int W, int NPL, bool BOX>
__global__ __launch_bounds__(256) void k_einstein_hmc(HmcRun a, const float* __restrict__ cen, int D, Step s,
                                                      float neg_inv_var, float lii, float c2pi, float hld,
                                                      float hb, float lf) {
    NFK_ROW_PROLOGUE(W)
    for (int64_t r0 = wave * RPW; r0 < a.chains; r0 += nwave * RPW) {
        const int64_t b = r0 + sub;
        const bool ok = b < a.chains;
        float xc[NPL], cc[NPL], vl[NPL], xn[NPL];
        float u = 0.0f;
        int nacc = 0;
#pragma unroll
        for (int q = 0; q < NPL; ++q) {
            const int c = c0 + q * W;
            const bool live = ok && c < D;
            xc[q] = live ? a.x_cur[b * a.ldx + c] : 0.0f;
            cc[q] = live ? cen[c] : 0.0f;
            vl[q] = 0.0f;
        }
        if (ok) u = a.u_cur[b];
        for (int e = 0; e < a.epochs; ++e) {
            const int64_t ec = (int64_t)e * a.chains + b;  // this chain's row of the epoch's draws
            float m = 0.0f, kc = 0.0f, kn = 0.0f;
#pragma unroll
            for (int q = 0; q < NPL; ++q) {
                const int c = c0 + q * W;
                xn[q] = xc[q];
                if (ok && c < D) {
                    if (a.pos_rec != nullptr) a.pos_rec[ec * D + c] = xc[q];
                    float x = xc[q], v = a.v_draws[ec * D + c];
                    kc += v * v;
                    float G = einstein_dlp(einstein_dev<BOX>(x, cc[q], hb, lf), neg_inv_var);
                    for (int k = 0; k < s.path_len; ++k) {
                        const float xs = step_x(x, v, G, s);
                        const float Gn =
                            einstein_dlp(einstein_dev<BOX>(s.verlet ? xs : x, cc[q], hb, lf), neg_inv_var);
                        v = step_v(v, G, Gn, s);
                        x = xs;
                        G = Gn;
                    }
                    xn[q] = x;
                    vl[q] = v;
                    kn += v * v;
                    const float y = einstein_dev<BOX>(x, cc[q], hb, lf) / lii;
                    m += y * y;
                }
            }
            m = group_sum<W>(m);
            const float un = -(-0.5f * (c2pi + m) - hld);
            if (a.hamiltonian) {
                kc = group_sum<W>(kc) * 0.5f;
                kn = group_sum<W>(kn) * 0.5f;
            }
            int acc = 0;
            if (ok && c0 == 0) {
                if (a.pot_rec != nullptr) a.pot_rec[ec] = u;
                acc = hmc_decide(u, un, kc, kn, a.r[ec], a.beta, a.hamiltonian);
            }
            acc = __shfl(acc, sub * W, 64);
            if (acc) {
                u = un;
                nacc += 1;
#pragma unroll
                for (int q = 0; q < NPL; ++q) xc[q] = xn[q];
            }
        }
#pragma unroll
        for (int q = 0; q < NPL; ++q) {
            const int c = c0 + q * W;
            if (ok && c < D) {
                a.x_cur[b * a.ldx + c] = xc[q];
                if (a.v_last != nullptr) a.v_last[b * a.ldv + c] = vl[q];
            }
        }
        if (ok && c0 == 0) {
            a.u_cur[b] = u;
            if (a.naccept != nullptr) a.naccept[b] += nacc;
        }
    }
}

// ---------------------------------------------------------------------------
// Gaussian mixture: a chain on W lanes, lane c0 keeps particles c0 + q W,
// q < PPL, in registers.
// ---------------------------------------------------------------------------
template <int W, int PPL, int DIM>
__global__ __launch_bounds__(256) void k_gmix_hmc(HmcRun a, const float* __restrict__ cen,
                                                  const float* __restrict__ scales,
                                                  const float* __restrict__ hlds, int npart, int M, Step s,
                                                  float inv_m, float c2pi) {
    NFK_ROW_PROLOGUE(W)
    const int64_t width = (int64_t)npart * DIM;
    for (int64_t r0 = wave * RPW; r0 < a.chains; r0 += nwave * RPW) {
        const int64_t b = r0 + sub;
        const bool ok = b < a.chains;
        float xc[PPL][DIM], vl[PPL][DIM], xp[PPL][DIM];
        float u = 0.0f;
        int nacc = 0;
#pragma unroll
        for (int q = 0; q < PPL; ++q) {
            const int p = c0 + q * W;
#pragma unroll
            for (int d = 0; d < DIM; ++d) {
                xc[q][d] = (ok && p < npart) ? a.x_cur[b * a.ldx + p * DIM + d] : 0.0f;
                vl[q][d] = 0.0f;
            }
        }
        if (ok) u = a.u_cur[b];
        for (int e = 0; e < a.epochs; ++e) {
            const int64_t ec = (int64_t)e * a.chains + b;
            float lp = 0.0f, kc = 0.0f, kn = 0.0f;
#pragma unroll
            for (int q = 0; q < PPL; ++q) {
                const int p = c0 + q * W;
#pragma unroll
                for (int d = 0; d < DIM; ++d) xp[q][d] = xc[q][d];
                if (ok && p < npart) {
                    float x[DIM], v[DIM], G[DIM], xs[DIM], Gn[DIM];
#pragma unroll
                    for (int d = 0; d < DIM; ++d) {
                        if (a.pos_rec != nullptr) a.pos_rec[ec * width + p * DIM + d] = xc[q][d];
                        x[d] = xc[q][d];
                        v[d] = a.v_draws[ec * width + p * DIM + d];
                        kc += v[d] * v[d];
                    }
                    gmix_dlp<DIM>(x, cen, scales, hlds, M, inv_m, c2pi, G);
                    for (int k = 0; k < s.path_len; ++k) {
#pragma unroll
                        for (int d = 0; d < DIM; ++d) xs[d] = step_x(x[d], v[d], G[d], s);
                        if (s.verlet)
                            gmix_dlp<DIM>(xs, cen, scales, hlds, M, inv_m, c2pi, Gn);
                        else
                            gmix_dlp<DIM>(x, cen, scales, hlds, M, inv_m, c2pi, Gn);
#pragma unroll
                        for (int d = 0; d < DIM; ++d) {
                            v[d] = step_v(v[d], G[d], Gn[d], s);
                            x[d] = xs[d];
                            G[d] = Gn[d];
                        }
                    }
#pragma unroll
                    for (int d = 0; d < DIM; ++d) {
                        xp[q][d] = x[d];
                        vl[q][d] = v[d];
                        kn += v[d] * v[d];
                    }
                    lp += logf(gmix_prob<DIM>(x, cen, scales, hlds, M, inv_m, c2pi));
                }
            }
            lp = group_sum<W>(lp);
            const float un = -lp;
            if (a.hamiltonian) {
                kc = group_sum<W>(kc) * 0.5f;
                kn = group_sum<W>(kn) * 0.5f;
            }
            int acc = 0;
            if (ok && c0 == 0) {
                if (a.pot_rec != nullptr) a.pot_rec[ec] = u;
                acc = hmc_decide(u, un, kc, kn, a.r[ec], a.beta, a.hamiltonian);
            }
            acc = __shfl(acc, sub * W, 64);
            if (acc) {
                u = un;
                nacc += 1;
#pragma unroll
                for (int q = 0; q < PPL; ++q)
#pragma unroll
                    for (int d = 0; d < DIM; ++d) xc[q][d] = xp[q][d];
            }
        }
#pragma unroll
        for (int q = 0; q < PPL; ++q) {
            const int p = c0 + q * W;
            if (ok && p < npart) {
#pragma unroll
                for (int d = 0; d < DIM; ++d) {
                    a.x_cur[b * a.ldx + p * DIM + d] = xc[q][d];
                    if (a.v_last != nullptr) a.v_last[b * a.ldv + p * DIM + d] = vl[q][d];
                }
            }
        }
        if (ok && c0 == 0) {
            a.u_cur[b] = u;
            if (a.naccept != nullptr) a.naccept[b] += nacc;
        }
    }
}

// ---------------------------------------------------------------------------
// Lennard-Jones: k_lj_traj's mapping (a row on G lanes, PPL particles per lane,
// the row staged in LDS as float4 and read by broadcast; a row never leaves its
// wave).  x_cur stays in registers; every integrator step and, after the
// decision, every epoch stages positions in the row's other LDS buffer, which
// was last read before the previous barrier, so each costs one barrier.  The
// restage after the decision is unconditional and epochs and path_len are
// kernel-uniform: every __syncthreads sits in block-uniform control flow, and
// rows past `chains` walk the barriers without touching memory.
// ---------------------------------------------------------------------------
template <int G, int PPL, int DIM>
__global__ __launch_bounds__(256) void k_lj_hmc(HmcRun a, int n, Step s, LjConst k) {
    extern __shared__ __attribute__((aligned(16))) float4 s_pos[];
    constexpr int RPW = 64 / G, RPB = 4 * RPW;
    const int lane = threadIdx.x & 63;
    const int rb = (threadIdx.x >> 6) * RPW + lane / G;  // row within the block
    const int c0 = lane % G;
    const int64_t width = (int64_t)n * DIM;
    float4* srow = s_pos + (size_t)rb * n;  // buffer 0; buffer 1 lies RPB rows further on
    const int other = RPB * n;
    for (int64_t r0 = (int64_t)blockIdx.x * RPB; r0 < a.chains; r0 += (int64_t)gridDim.x * RPB) {
        const int64_t b = r0 + rb;
        const bool ok = b < a.chains;
        float xc[PPL][3], x[PPL][3], v[PPL][3], F[PPL][3], xn[PPL][3], f[PPL][3];
        float u = 0.0f;
        int nacc = 0;
#pragma unroll
        for (int q = 0; q < PPL; ++q) {
            const int i = c0 + q * G;
            xc[q][0] = xc[q][1] = xc[q][2] = 0.0f;
            v[q][0] = v[q][1] = v[q][2] = 0.0f;
            if (ok && i < n) {
                const float* px = a.x_cur + b * a.ldx + (int64_t)i * DIM;
#pragma unroll
                for (int d = 0; d < DIM; ++d) xc[q][d] = px[d];
                srow[i] = make_float4(xc[q][0], xc[q][1], xc[q][2], 0.0f);
            }
        }
        if (ok) u = a.u_cur[b];
        __syncthreads();
        int cur = 0;
        for (int e = 0; e < a.epochs; ++e) {
            const int64_t ec = (int64_t)e * a.chains + b;
            float kc = 0.0f, kn = 0.0f;
#pragma unroll
            for (int q = 0; q < PPL; ++q) {
                const int i = c0 + q * G;
#pragma unroll
                for (int d = 0; d < 3; ++d) {
                    x[q][d] = xc[q][d];
                    v[q][d] = 0.0f;
                }
                if (ok && i < n) {
#pragma unroll
                    for (int d = 0; d < DIM; ++d) {
                        if (a.pos_rec != nullptr) a.pos_rec[ec * width + (int64_t)i * DIM + d] = xc[q][d];
                        v[q][d] = a.v_draws[ec * width + (int64_t)i * DIM + d];
                        kc += v[q][d] * v[q][d];
                    }
                }
            }
            if (ok) lj_row<G, PPL, DIM, true>(x, srow + cur * other, n, c0, k, f);
#pragma unroll
            for (int q = 0; q < PPL; ++q)
#pragma unroll
                for (int d = 0; d < 3; ++d) F[q][d] = ok ? -f[q][d] : 0.0f;
            for (int st = 0; st < s.path_len; ++st) {
#pragma unroll
                for (int q = 0; q < PPL; ++q)
#pragma unroll
                    for (int d = 0; d < 3; ++d)
                        xn[q][d] = d < DIM ? step_x(x[q][d], v[q][d], F[q][d], s) : 0.0f;
                if (!s.verlet && ok) lj_row<G, PPL, DIM, true>(x, srow + cur * other, n, c0, k, f);
#pragma unroll
                for (int q = 0; q < PPL; ++q) {
                    const int i = c0 + q * G;
                    if (ok && i < n)
                        srow[(cur ^ 1) * other + i] = make_float4(xn[q][0], xn[q][1], xn[q][2], 0.0f);
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
            float en = 0.0f;
            if (ok) en = lj_row<G, PPL, DIM, false>(x, srow + cur * other, n, c0, k, f);
            en = group_sum<G>(en);
            const float un = en / 2.0f;
            if (a.hamiltonian) {
#pragma unroll
                for (int q = 0; q < PPL; ++q) {
                    if (ok && c0 + q * G < n) {
#pragma unroll
                        for (int d = 0; d < DIM; ++d) kn += v[q][d] * v[q][d];
                    }
                }
                kc = group_sum<G>(kc) * 0.5f;
                kn = group_sum<G>(kn) * 0.5f;
            }
            int acc = 0;
            if (ok && c0 == 0) {
                if (a.pot_rec != nullptr) a.pot_rec[ec] = u;
                acc = hmc_decide(u, un, kc, kn, a.r[ec], a.beta, a.hamiltonian);
            }
            acc = __shfl(acc, lane - c0, 64);
            if (acc) {
                u = un;
                nacc += 1;
#pragma unroll
                for (int q = 0; q < PPL; ++q)
#pragma unroll
                    for (int d = 0; d < 3; ++d) xc[q][d] = x[q][d];
            }
            // the next epoch starts from x_cur, accepted or not
#pragma unroll
            for (int q = 0; q < PPL; ++q) {
                const int i = c0 + q * G;
                if (ok && i < n) srow[(cur ^ 1) * other + i] = make_float4(xc[q][0], xc[q][1], xc[q][2], 0.0f);
            }
            __syncthreads();
            cur ^= 1;
        }
        if (ok) {
#pragma unroll
            for (int q = 0; q < PPL; ++q) {
                const int i = c0 + q * G;
                if (i < n) {
                    float* px = a.x_cur + b * a.ldx + (int64_t)i * DIM;
#pragma unroll
                    for (int d = 0; d < DIM; ++d) {
                        px[d] = xc[q][d];
                        if (a.v_last != nullptr) a.v_last[b * a.ldv + (int64_t)i * DIM + d] = v[q][d];
                    }
                }
            }
            if (c0 == 0) {
                a.u_cur[b] = u;
                if (a.naccept != nullptr) a.naccept[b] += nacc;
            }
        }
        // the next round's first stage writes buffer 0; every read of this round
        // came before the last epoch's barrier
    }
}

// ---------------------------------------------------------------------------
// Embedded-atom model: k_eam_traj's mapping and arithmetic (two LDS buffers per
// row, eam_row_step_force with its barrier between the density and the force
// loop) inside k_lj_hmc's epoch loop: x_cur, u and the count on chip, the
// unconditional restage of x_cur after the decision.  epochs, path_len and the
// scheme are kernel-uniform, so every __syncthreads sits in block-uniform
// control flow; rows past `chains` walk the barriers without touching memory.
// ---------------------------------------------------------------------------
template <int G, int PPL>
__global__ __launch_bounds__(256) void k_eam_hmc(HmcRun a, int n, Step s, const float4* __restrict__ rtab,
                                                 const float4* __restrict__ ftab, EamConst k) {
    extern __shared__ __attribute__((aligned(16))) float4 s_pos[];
    constexpr int RPW = 64 / G, RPB = 4 * RPW;
    const int lane = threadIdx.x & 63;
    const int rb = (threadIdx.x >> 6) * RPW + lane / G;  // row within the block
    const int c0 = lane % G;
    const int64_t width = (int64_t)n * 3;
    float4* srow = s_pos + (size_t)rb * n;  // buffer 0; buffer 1 lies RPB rows further on
    const int other = RPB * n;
    for (int64_t r0 = (int64_t)blockIdx.x * RPB; r0 < a.chains; r0 += (int64_t)gridDim.x * RPB) {
        const int64_t b = r0 + rb;
        const bool ok = b < a.chains;
        float xc[PPL][3], x[PPL][3], v[PPL][3], F[PPL][3], xn[PPL][3], Fn[PPL][3];
        float u = 0.0f;
        int nacc = 0;
#pragma unroll
        for (int q = 0; q < PPL; ++q) {
            const int i = c0 + q * G;
            xc[q][0] = xc[q][1] = xc[q][2] = 0.0f;
            v[q][0] = v[q][1] = v[q][2] = 0.0f;
            if (ok && i < n) {
                const float* px = a.x_cur + b * a.ldx + (int64_t)i * 3;
#pragma unroll
                for (int d = 0; d < 3; ++d) xc[q][d] = px[d];
                srow[i] = make_float4(xc[q][0], xc[q][1], xc[q][2], 0.0f);
            }
        }
        if (ok) u = a.u_cur[b];
        __syncthreads();
        int cur = 0;
        for (int e = 0; e < a.epochs; ++e) {
            const int64_t ec = (int64_t)e * a.chains + b;
            float kc = 0.0f, kn = 0.0f;
#pragma unroll
            for (int q = 0; q < PPL; ++q) {
                const int i = c0 + q * G;
#pragma unroll
                for (int d = 0; d < 3; ++d) {
                    x[q][d] = xc[q][d];
                    v[q][d] = 0.0f;
                }
                if (ok && i < n) {
#pragma unroll
                    for (int d = 0; d < 3; ++d) {
                        if (a.pos_rec != nullptr) a.pos_rec[ec * width + (int64_t)i * 3 + d] = xc[q][d];
                        v[q][d] = a.v_draws[ec * width + (int64_t)i * 3 + d];
                        kc += v[q][d] * v[q][d];
                    }
                }
            }
            eam_row_step_force<G, PPL>(ok, x, srow + cur * other, n, c0, k, rtab, ftab, F);
            for (int st = 0; st < s.path_len; ++st) {
#pragma unroll
                for (int q = 0; q < PPL; ++q)
#pragma unroll
                    for (int d = 0; d < 3; ++d) xn[q][d] = step_x(x[q][d], v[q][d], F[q][d], s);
                if (!s.verlet) eam_row_step_force<G, PPL>(ok, x, srow + cur * other, n, c0, k, rtab, ftab, Fn);
#pragma unroll
                for (int q = 0; q < PPL; ++q) {
                    const int i = c0 + q * G;
                    if (ok && i < n)
                        srow[(cur ^ 1) * other + i] = make_float4(xn[q][0], xn[q][1], xn[q][2], 0.0f);
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
            float en = 0.0f;
            if (ok) en = eam_row_energy<G, PPL>(x, srow + cur * other, n, c0, k, rtab, ftab);
            const float un = group_sum<G>(en);
            if (a.hamiltonian) {
#pragma unroll
                for (int q = 0; q < PPL; ++q) {
                    if (ok && c0 + q * G < n) {
#pragma unroll
                        for (int d = 0; d < 3; ++d) kn += v[q][d] * v[q][d];
                    }
                }
                kc = group_sum<G>(kc) * 0.5f;
                kn = group_sum<G>(kn) * 0.5f;
            }
            int acc = 0;
            if (ok && c0 == 0) {
                if (a.pot_rec != nullptr) a.pot_rec[ec] = u;
                acc = hmc_decide(u, un, kc, kn, a.r[ec], a.beta, a.hamiltonian);
            }
            acc = __shfl(acc, lane - c0, 64);
            if (acc) {
                u = un;
                nacc += 1;
#pragma unroll
                for (int q = 0; q < PPL; ++q)
#pragma unroll
                    for (int d = 0; d < 3; ++d) xc[q][d] = x[q][d];
            }
            // the next epoch starts from x_cur, accepted or not
#pragma unroll
            for (int q = 0; q < PPL; ++q) {
                const int i = c0 + q * G;
                if (ok && i < n) srow[(cur ^ 1) * other + i] = make_float4(xc[q][0], xc[q][1], xc[q][2], 0.0f);
            }
            __syncthreads();
            cur ^= 1;
        }
        if (ok) {
#pragma unroll
            for (int q = 0; q < PPL; ++q) {
                const int i = c0 + q * G;
                if (i < n) {
                    float* px = a.x_cur + b * a.ldx + (int64_t)i * 3;
#pragma unroll
                    for (int d = 0; d < 3; ++d) {
                        px[d] = xc[q][d];
                        if (a.v_last != nullptr) a.v_last[b * a.ldv + (int64_t)i * 3 + d] = v[q][d];
                    }
                }
            }
            if (c0 == 0) {
                a.u_cur[b] = u;
                if (a.naccept != nullptr) a.naccept[b] += nacc;
            }
        }
        // the next round's first stage writes buffer 0; every read of this round
        // came before the last epoch's barrier
    }
}

// Host checks shared by the entry points; `shape_ok` is the system's
// *_hmc_supported answer.  Returns 0 to go on, 1 to return 0 without a launch,
// NFK_EINVAL after nfk_set_error.
int check_run(const char* who, const void* x_cur, int64_t ldx, const void* u_cur, const void* v_draws,
              const void* r, const void* v_last, int64_t ldv, const void* pos_rec, const void* pot_rec,
              int64_t chains, int32_t epochs, int32_t path_len, int32_t scheme, int64_t width,
              int shape_ok) {
    char buf[160];
    const char* why = nullptr;
    if (chains < 0) why = "bad chains";
    else if (epochs < 0) why = "epochs below zero";
    else if (path_len < 0) why = "path_len below zero";
    else if (scheme != 0 && scheme != 1) why = "scheme must be 0 (lagged force) or 1 (velocity Verlet)";
    else if (!shape_ok) why = "shape not supported";
    else if ((pos_rec == nullptr) != (pot_rec == nullptr)) why = "pos_rec and pot_rec come together";
    else if (chains == 0 || epochs == 0) return 1;
    else if (!x_cur || !u_cur || !v_draws || !r) why = "null pointer";
    else if (ldx < width || (v_last != nullptr && ldv < width)) why = "leading dimension below the row width";
    if (why == nullptr) return 0;
    std::snprintf(buf, sizeof(buf), "%s: %s", who, why);
    return nfk_set_error(buf);
}

HmcRun make_run(float* x_cur, int64_t ldx, float* u_cur, int32_t* naccept, const float* v_draws,
                const float* r, float* v_last, int64_t ldv, float* pos_rec, float* pot_rec, int64_t chains,
                int32_t epochs, double beta, int32_t hamiltonian) {
    HmcRun a;
    a.x_cur = x_cur;
    a.ldx = ldx;
    a.u_cur = u_cur;
    a.naccept = naccept;
    a.v_draws = v_draws;
    a.r = r;
    a.v_last = v_last;
    a.ldv = ldv;
    a.pos_rec = pos_rec;
    a.pot_rec = pot_rec;
    a.chains = chains;
    a.epochs = epochs;
    a.hamiltonian = hamiltonian ? 1 : 0;
    a.beta = (float)beta;
    return a;
}

}  // namespace

// ---------------------------------------------------------------------------
// C ABI
// ---------------------------------------------------------------------------
extern "C" int nfk_einstein_hmc_supported(int32_t natoms, int32_t dim) {
    return natoms > 0 && dim > 0 && (int64_t)natoms * dim <= 512;
}

extern "C" int nfk_gmix_hmc_supported(int32_t npart, int32_t dim, int32_t ncenters) {
    return npart > 0 && npart <= 256 && nfk_gmix_supported(ncenters, dim) != 0;
}

extern "C" int nfk_lj_hmc_supported(int32_t n, int32_t dim) { return nfk_lj_supported(n, dim); }

extern "C" int nfk_eam_hmc_supported(int32_t n) { return nfk_eam_supported(n); }

extern "C" int nfk_einstein_hmc_run(float* x_cur, int64_t ldx, float* u_cur, int32_t* naccept,
                                    const float* v_draws, const float* r, float* v_last, int64_t ldv,
                                    float* pos_rec, float* pot_rec, int64_t chains, int32_t epochs,
                                    int32_t path_len, double dt, double dt_sq, int32_t scheme, double beta,
                                    int32_t hamiltonian, const float* centers, int32_t natoms, int32_t dim,
                                    float scale, float half_log_det, int32_t has_box, double boxlength,
                                    nfk_stream_t stream) {
    const int shape_ok = nfk_einstein_hmc_supported(natoms, dim) && scale > 0.0f;
    const int D = shape_ok ? natoms * dim : 0;
    const int rc = check_run("nfk_einstein_hmc_run", x_cur, ldx, u_cur, v_draws, r, v_last, ldv, pos_rec,
                             pot_rec, chains, epochs, path_len, scheme, D, shape_ok);
    if (rc != 0) return rc == 1 ? 0 : rc;
    if (!centers) return nfk_set_error("nfk_einstein_hmc_run: null pointer");
    hipStream_t st = (hipStream_t)stream;
    const HmcRun a = make_run(x_cur, ldx, u_cur, naccept, v_draws, r, v_last, ldv, pos_rec, pot_rec, chains,
                              epochs, beta, hamiltonian);
    const Step s = make_step(path_len, dt, dt_sq, scheme);
    const float c2pi = (float)(D * std::log(2.0 * M_PI));
    const float hld = (float)((double)natoms * (double)half_log_det);
    const float niv = (float)(-1.0 / ((double)scale * (double)scale));
    const float hb = (float)(0.5 * boxlength), lf = (float)boxlength;
    const int w = lanes_for(D);
    const int npl = (D + w - 1) / w;
    const unsigned g = grid_for_rows(chains, w);
#define CALLN(W, N)                                                                                        \
    do {                                                                                                   \
        if (has_box)                                                                                       \
            hipLaunchKernelGGL((k_einstein_hmc<W, N, true>), dim3(g), dim3(256), 0, st, a, centers, D, s, niv, \
                               scale, c2pi, hld, hb, lf);                                                  \
        else                                                                                               \
            hipLaunchKernelGGL((k_einstein_hmc<W, N, false>), dim3(g), dim3(256), 0, st, a, centers, D, s,  \
                               niv, scale, c2pi, hld, hb, lf);                                             \
    } while (0)
#define CALL(W) CALLN(W, 1)
    if (npl <= 1) {
        NFK_W_DISPATCH(w, CALL)
    } else if (npl == 2) {
        CALLN(64, 2);
    } else if (npl <= 4) {
        CALLN(64, 4);
    } else {
        CALLN(64, 8);
    }
#undef CALL
#undef CALLN
    return launch_status("nfk_einstein_hmc_run");
}

extern "C" int nfk_gmix_hmc_run(float* x_cur, int64_t ldx, float* u_cur, int32_t* naccept,
                                const float* v_draws, const float* r, float* v_last, int64_t ldv,
                                float* pos_rec, float* pot_rec, int64_t chains, int32_t epochs,
                                int32_t path_len, double dt, double dt_sq, int32_t scheme, double beta,
                                int32_t hamiltonian, const float* centers, const float* scales,
                                const float* hlds, int32_t npart, int32_t dim, int32_t ncenters,
                                nfk_stream_t stream) {
    const int shape_ok = nfk_gmix_hmc_supported(npart, dim, ncenters);
    const int rc = check_run("nfk_gmix_hmc_run", x_cur, ldx, u_cur, v_draws, r, v_last, ldv, pos_rec, pot_rec,
                             chains, epochs, path_len, scheme, shape_ok ? (int64_t)npart * dim : 0, shape_ok);
    if (rc != 0) return rc == 1 ? 0 : rc;
    if (!centers || !scales || !hlds) return nfk_set_error("nfk_gmix_hmc_run: null pointer");
    hipStream_t st = (hipStream_t)stream;
    const HmcRun a = make_run(x_cur, ldx, u_cur, naccept, v_draws, r, v_last, ldv, pos_rec, pot_rec, chains,
                              epochs, beta, hamiltonian);
    const Step s = make_step(path_len, dt, dt_sq, scheme);
    const float inv_m = (float)(1.0 / ncenters);
    const float c2pi = (float)(dim * std::log(2.0 * M_PI));
    const int w = lanes_for(npart);
    const int ppl = (npart + w - 1) / w;
    const unsigned g = grid_for_rows(chains, w);
#define CALLD(W, PP, DD)                                                                                \
    hipLaunchKernelGGL((k_gmix_hmc<W, PP, DD>), dim3(g), dim3(256), 0, st, a, centers, scales, hlds, npart, \
                       ncenters, s, inv_m, c2pi)
#define CALLP(W, PP)                     \
    switch (dim) {                       \
        case 1: CALLD(W, PP, 1); break;  \
        case 2: CALLD(W, PP, 2); break;  \
        case 3: CALLD(W, PP, 3); break;  \
        default: CALLD(W, PP, 4); break; \
    }
#define CALL(W) CALLP(W, 1)
    if (ppl <= 1) {
        NFK_W_DISPATCH(w, CALL)
    } else if (ppl == 2) {
        CALLP(64, 2)
    } else {
        CALLP(64, 4)
    }
#undef CALL
#undef CALLP
#undef CALLD
    return launch_status("nfk_gmix_hmc_run");
}

extern "C" int nfk_lj_hmc_run(float* x_cur, int64_t ldx, float* u_cur, int32_t* naccept, const float* v_draws,
                              const float* r, float* v_last, int64_t ldv, float* pos_rec, float* pot_rec,
                              int64_t chains, int32_t epochs, int32_t path_len, double dt, double dt_sq,
                              int32_t scheme, double beta, int32_t hamiltonian, int32_t n, int32_t dim,
                              double boxlength, double sigma, double epsilon, int32_t has_cutoff,
                              double cutoff, int32_t shift, nfk_stream_t stream) {
    const int shape_ok = nfk_lj_hmc_supported(n, dim);
    if (shape_ok && has_cutoff && !(cutoff > 0.0)) return nfk_set_error("nfk_lj_hmc_run: bad cutoff");
    const int rc = check_run("nfk_lj_hmc_run", x_cur, ldx, u_cur, v_draws, r, v_last, ldv, pos_rec, pot_rec,
                             chains, epochs, path_len, scheme, shape_ok ? (int64_t)n * dim : 0, shape_ok);
    if (rc != 0) return rc == 1 ? 0 : rc;
    hipStream_t st = (hipStream_t)stream;
    const HmcRun a = make_run(x_cur, ldx, u_cur, naccept, v_draws, r, v_last, ldv, pos_rec, pot_rec, chains,
                              epochs, beta, hamiltonian);
    const Step s = make_step(path_len, dt, dt_sq, scheme);
    const LjConst k = lj_const(boxlength, sigma, epsilon, has_cutoff, cutoff, shift);
    const int G = lanes_for(n);
    const int ppl = (n + 63) / 64;
    const int rpb = 4 * (64 / G);
    int64_t grid = (chains + rpb - 1) / rpb;
    if (grid > 16384) grid = 16384;
    const size_t lds = (size_t)2 * rpb * n * sizeof(float4);  // two buffers per row, <= 32 KiB (n <= 256)
#define LJ_CALL2(GG, PP)                                                                                  \
    do {                                                                                                  \
        if (dim == 3)                                                                                     \
            hipLaunchKernelGGL((k_lj_hmc<GG, PP, 3>), dim3((unsigned)grid), dim3(256), lds, st, a, n, s, k); \
        else                                                                                              \
            hipLaunchKernelGGL((k_lj_hmc<GG, PP, 2>), dim3((unsigned)grid), dim3(256), lds, st, a, n, s, k); \
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
    return launch_status("nfk_lj_hmc_run");
}

extern "C" int nfk_eam_hmc_run(float* x_cur, int64_t ldx, float* u_cur, int32_t* naccept, const float* v_draws,
                               const float* r, float* v_last, int64_t ldv, float* pos_rec, float* pot_rec,
                               int64_t chains, int32_t epochs, int32_t path_len, double dt, double dt_sq,
                               int32_t scheme, double beta, int32_t hamiltonian, int32_t n, const float* rtab,
                               int32_t nr, double dr, const float* ftab, int32_t nrho, double drho,
                               double f_end, double fp_end, double lx, double ly, double lz, double rc,
                               nfk_stream_t stream) {
    const int shape_ok = nfk_eam_hmc_supported(n);
    EamConst k;
    if (shape_ok &&
        eam_setup("nfk_eam_hmc_run", k, rtab, nr, dr, ftab, nrho, drho, f_end, fp_end, lx, ly, lz, rc))
        return NFK_EINVAL;
    const int rcode = check_run("nfk_eam_hmc_run", x_cur, ldx, u_cur, v_draws, r, v_last, ldv, pos_rec, pot_rec,
                                chains, epochs, path_len, scheme, shape_ok ? (int64_t)n * 3 : 0, shape_ok);
    if (rcode != 0) return rcode == 1 ? 0 : rcode;
    if (!rtab || !ftab) return nfk_set_error("nfk_eam_hmc_run: null pointer");
    hipStream_t st = (hipStream_t)stream;
    const HmcRun a = make_run(x_cur, ldx, u_cur, naccept, v_draws, r, v_last, ldv, pos_rec, pot_rec, chains,
                              epochs, beta, hamiltonian);
    const Step s = make_step(path_len, dt, dt_sq, scheme);
    const int G = lanes_for(n);
    const int ppl = (n + 63) / 64;
    const int rpb = 4 * (64 / G);
    int64_t grid = (chains + rpb - 1) / rpb;
    if (grid > 16384) grid = 16384;
    const size_t lds = (size_t)2 * rpb * n * sizeof(float4);  // two buffers per row, <= 32 KiB (n <= 256)
#define EAM_CALL2(GG, PP)                                                                              \
    hipLaunchKernelGGL((k_eam_hmc<GG, PP>), dim3((unsigned)grid), dim3(256), lds, st, a, n, s,         \
                       (const float4*)rtab, (const float4*)ftab, k)
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
    return launch_status("nfk_eam_hmc_run");
}
