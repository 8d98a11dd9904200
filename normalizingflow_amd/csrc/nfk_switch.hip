// nfk_switch.hip -- Hamiltonian switching between an Einstein crystal A and a
// target B (Lennard-Jones or the embedded-atom model) in ONE launch per chunk of
// steps: Langevin dynamics (BAOAB, the noise of nfk_rng.h) on the mixed reduced
// potential u_lam = (1 - lam) u_A + lam U_B / kT at temperature kT, with the
// switching work accumulated in fp64 on the way (Frenkel-Ladd / Jarzynski-Crooks).
// The kernel follows k_lj_lv / k_eam_lv of nfk_langevin.hip: a group of G lanes per
// row, the lane's PPL particles with x, v, the two forces and the Einstein centres
// in registers, two LDS row buffers, every __syncthreads in block-uniform control
// flow, rows past `batch` walking the barriers without touching memory.  The forces
// and energies are the device functions of nfk_systems_dev.h.  VALU kernels: no
// MFMA, no atomics, plain vector stores, every sum in a fixed order,
// -ffp-contract=off.
//
// Per step k < nsteps, with l0 = lam[step0 + k], l1 = lam[step0 + k + 1]:
//   if (l1 != l0)   w = w + ((double)l1 - (double)l0) * ((double)U_B(x) * inv_kT - (double)u_A(x))
//   a = (1.0f - l1) * kT;  b = l1;  F = a * g_A + b * g_B          (fp32, this order)
//   v = v + hb*F;  x = x + hd*v;  v = c1*v + c2*xi(step0 + k);  x = x + hd*v
//   g_A = d log p_A / dx (x);  g_B = -dU_B / dx (x);  F = a * g_A + b * g_B;  v = v + hb*F
// g_A and g_B stay apart in registers: the next step's opening kick recombines them
// with its own a and b, so a step costs one evaluation of each force.  w starts from
// work[b] and goes back there, so a run cut into launches adds in the same order.
//
// Energies.  U_B is the target's own row sum (lj_row / eam_row_energy and the
// butterfly, as nfk_lj_potential / nfk_eam_potential).  u_A = -log p_A is summed in
// this kernel's own order: per lane m = sum over its particles c0 + q G, q ascending,
// and per particle over the components d ascending, of (dev / scale)^2; then the
// butterfly group_sum<G> over the row's lanes; u_A = -(-0.5f * (c2pi + m) - hld) with
// c2pi = (float)(n dim log 2 pi) and hld = (float)(n half_log_det).
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdio>

#include "../../include/nfk.h"
#include "nfk_systems_dev.h"
#include "nfk_rng.h"

namespace {

// the BAOAB constants and the record schedule of a call (nfk_langevin.hip's)
struct Sw {
    float hb, hd, c1, c2;
    int nsteps, record_every;
    uint64_t step0;
    int64_t frame0;  // step0 / record_every
    const float* lam;
    double inv_kT;
    float kT;
};

// the Einstein crystal A: centres [n, DIM]; niv = (float)(-1 / scale^2), lii = scale
struct EinA {
    const float* cen;
    float niv, lii, c2pi, hld, hb, lf;
    int box;
};

__device__ __forceinline__ int64_t sw_frame(const Sw& s, int k) {
    if (s.record_every <= 0) return -1;
    const uint64_t done = s.step0 + (uint64_t)k + 1;
    if (done % (uint64_t)s.record_every != 0) return -1;
    return (int64_t)(done / (uint64_t)s.record_every) - 1 - s.frame0;
}

__device__ __forceinline__ float ein_dev(float x, float c, const EinA& A) {
    return A.box ? einstein_dev<true>(x, c, A.hb, A.lf) : einstein_dev<false>(x, c, A.hb, A.lf);
}

// The noise of the lane's particles for one step (lv_noise of nfk_langevin.hip: the
// lane's own particles in ascending order, the butterfly, the division by n).
template <int G, int PPL>
__device__ __forceinline__ void sw_noise(const RngKey& key, uint64_t step, uint32_t row, int n, int c0,
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

// The targets.  force(): g = -dU_B/dx of the lane's particles from the row staged in
// srow, zeros for a row with ok == false; EAM's holds a __syncthreads, so every call
// sits in block-uniform control flow.  energy(): the lane's share of the row's sum;
// finish() makes U_B of the butterfly's result.
template <int DIM_>
struct LjSys {
    static constexpr int DIM = DIM_;
    LjConst k;
    template <int G, int PPL>
    __device__ __forceinline__ void force(bool ok, const float (&x)[PPL][3], float4* srow, int n, int c0,
                                          float (&g)[PPL][3]) const {
        float f[PPL][3];
#pragma unroll
        for (int q = 0; q < PPL; ++q) f[q][0] = f[q][1] = f[q][2] = 0.0f;
        if (ok) lj_row<G, PPL, DIM, true>(x, srow, n, c0, k, f);
#pragma unroll
        for (int q = 0; q < PPL; ++q)
#pragma unroll
            for (int d = 0; d < 3; ++d) g[q][d] = ok ? -f[q][d] : 0.0f;
    }
    template <int G, int PPL>
    __device__ __forceinline__ float energy(const float (&x)[PPL][3], const float4* srow, int n, int c0) const {
        float f[PPL][3];
        return lj_row<G, PPL, DIM, false>(x, srow, n, c0, k, f);
    }
    __device__ __forceinline__ float finish(float e) const { return e / 2.0f; }
};

struct EamSys {
    static constexpr int DIM = 3;
    EamConst k;
    const float4* rtab;
    const float4* ftab;
    template <int G, int PPL>
    __device__ __forceinline__ void force(bool ok, const float (&x)[PPL][3], float4* srow, int n, int c0,
                                          float (&g)[PPL][3]) const {
        eam_row_step_force<G, PPL>(ok, x, srow, n, c0, k, rtab, ftab, g);
    }
    template <int G, int PPL>
    __device__ __forceinline__ float energy(const float (&x)[PPL][3], const float4* srow, int n, int c0) const {
        return eam_row_energy<G, PPL>(x, srow, n, c0, k, rtab, ftab);
    }
    __device__ __forceinline__ float finish(float e) const { return e; }
};

// (u_A, U_B) of the row at x, staged in srow; every lane of the group gets both
template <class SYS, int G, int PPL>
__device__ __forceinline__ void sw_energies(const SYS& sys, const EinA& A, bool ok, const float (&x)[PPL][3],
                                            const float (&cen)[PPL][3], const float4* srow, int n, int c0,
                                            float& uA, float& uB) {
    float e = 0.0f, m = 0.0f;
    if (ok) e = sys.template energy<G, PPL>(x, srow, n, c0);
#pragma unroll
    for (int q = 0; q < PPL; ++q)
        if (ok && c0 + q * G < n) {
#pragma unroll
            for (int d = 0; d < SYS::DIM; ++d) {
                const float y = ein_dev(x[q][d], cen[q][d], A) / A.lii;
                m += y * y;
            }
        }
    uB = sys.finish(group_sum<G>(e));
    m = group_sum<G>(m);
    uA = -(-0.5f * (A.c2pi + m) - A.hld);
}

template <class SYS, int G, int PPL>
__global__ __launch_bounds__(256) void k_switch(const float* x_in, int64_t ldxi, const float* v_in, int64_t ldvi,
                                                float* x_out, int64_t ldxo, float* v_out, int64_t ldvo,
                                                float* __restrict__ en_out, int64_t batch, int n, Sw s, RngKey key,
                                                float* pos_rec, float* en_rec, double* work, EinA A, SYS sys) {
    extern __shared__ __attribute__((aligned(16))) float4 s_pos[];
    constexpr int DIM = SYS::DIM;
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
        float x[PPL][3], v[PPL][3], cen[PPL][3], gA[PPL][3], gB[PPL][3], z[PPL][4];
#pragma unroll
        for (int q = 0; q < PPL; ++q) {
            const int i = c0 + q * G;
            x[q][0] = x[q][1] = x[q][2] = 0.0f;
            v[q][0] = v[q][1] = v[q][2] = 0.0f;
            cen[q][0] = cen[q][1] = cen[q][2] = 0.0f;
            if (ok && i < n) {
                const float* px = x_in + b * ldxi + (int64_t)i * DIM;
                const float* pv = v_in + b * ldvi + (int64_t)i * DIM;
#pragma unroll
                for (int d = 0; d < DIM; ++d) {
                    x[q][d] = px[d];
                    v[q][d] = pv[d];
                    cen[q][d] = A.cen[i * DIM + d];
                }
                srow[i] = make_float4(x[q][0], x[q][1], x[q][2], 0.0f);
            }
        }
        __syncthreads();
        int cur = 0;
        sys.template force<G, PPL>(ok, x, srow, n, c0, gB);
#pragma unroll
        for (int q = 0; q < PPL; ++q)
#pragma unroll
            for (int d = 0; d < 3; ++d) gA[q][d] = einstein_dlp(ein_dev(x[q][d], cen[q][d], A), A.niv);
        double w = (work != nullptr && ok && c0 == 0) ? work[b] : 0.0;
        float uA = 0.0f, uB = 0.0f;
        bool have = false;  // (uA, uB) are those of the current x; kernel-uniform
        for (int st = 0; st < s.nsteps; ++st) {
            const float l0 = s.lam[s.step0 + (uint64_t)st], l1 = s.lam[s.step0 + (uint64_t)st + 1];
            if (l1 != l0) {  // kernel-uniform
                if (!have) sw_energies<SYS, G, PPL>(sys, A, ok, x, cen, srow + cur * other, n, c0, uA, uB);
                w = w + ((double)l1 - (double)l0) * ((double)uB * s.inv_kT - (double)uA);
            }
            const float ca = (1.0f - l1) * s.kT, cb = l1;
            sw_noise<G, PPL>(key, s.step0 + (uint64_t)st, row, n, c0, z);
#pragma unroll
            for (int q = 0; q < PPL; ++q)
#pragma unroll
                for (int d = 0; d < DIM; ++d) {
                    const float F = ca * gA[q][d] + cb * gB[q][d];
                    v[q][d] = v[q][d] + s.hb * F;
                    x[q][d] = x[q][d] + s.hd * v[q][d];
                    v[q][d] = s.c1 * v[q][d] + s.c2 * z[q][d];
                    x[q][d] = x[q][d] + s.hd * v[q][d];
                }
#pragma unroll
            for (int q = 0; q < PPL; ++q) {
                const int i = c0 + q * G;
                if (ok && i < n) srow[(cur ^ 1) * other + i] = make_float4(x[q][0], x[q][1], x[q][2], 0.0f);
            }
            __syncthreads();
            cur ^= 1;
            sys.template force<G, PPL>(ok, x, srow + cur * other, n, c0, gB);
#pragma unroll
            for (int q = 0; q < PPL; ++q)
#pragma unroll
                for (int d = 0; d < DIM; ++d) {
                    gA[q][d] = einstein_dlp(ein_dev(x[q][d], cen[q][d], A), A.niv);
                    const float F = ca * gA[q][d] + cb * gB[q][d];
                    v[q][d] = v[q][d] + s.hb * F;
                }
            have = false;
            const int64_t fr = sw_frame(s, st);
            if (fr >= 0 && pos_rec != nullptr) {  // kernel-uniform
                sw_energies<SYS, G, PPL>(sys, A, ok, x, cen, srow + cur * other, n, c0, uA, uB);
                have = true;
                if (ok) {
#pragma unroll
                    for (int q = 0; q < PPL; ++q) {
                        const int i = c0 + q * G;
                        if (i < n) {
                            float* px = pos_rec + (fr * batch + b) * width + (int64_t)i * DIM;
#pragma unroll
                            for (int d = 0; d < DIM; ++d) px[d] = x[q][d];
                        }
                    }
                    if (c0 == 0) {
                        en_rec[(fr * batch + b) * 2] = uA;
                        en_rec[(fr * batch + b) * 2 + 1] = uB;
                    }
                }
            }
        }
        if (!have) sw_energies<SYS, G, PPL>(sys, A, ok, x, cen, srow + cur * other, n, c0, uA, uB);
        if (ok) {
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
            if (c0 == 0) {
                en_out[b * 2] = uA;
                en_out[b * 2 + 1] = uB;
                if (work != nullptr) work[b] = w;
            }
        }
        __syncthreads();  // the next round overwrites the staged rows
    }
}

const int64_t ROWS_MAX = (int64_t)1 << 32;

// The checks of a switching call, in the manner of nfk_langevin.hip's check_lv; fills
// s, key and A.  0, or NFK_EINVAL after nfk_set_error: nothing is launched then.
int check_sw(const char* who, const void* x_in, int64_t ldxi, const void* v_in, int64_t ldvi, const void* x_out,
             int64_t ldxo, const void* v_out, int64_t ldvo, const void* en_out, int64_t batch, int32_t n,
             int32_t dim, int32_t nsteps, int64_t step0, int64_t row_base, int64_t seed, int32_t zero_mean,
             float hb, float hd, float c1, float c2, int32_t record_every, const void* pos_rec,
             const void* en_rec, const float* centers, int32_t natoms_A, int32_t dim_A, float scale,
             float half_log_det, int32_t has_box, double boxlength_A, const float* lam, int64_t lam_len,
             double inv_kT, float kT, const void* work, Sw& s, RngKey& key, EinA& A) {
    char buf[200];
    const char* why = nullptr;
    const int64_t width = (int64_t)n * dim;
    if (nsteps < 0) why = "nsteps below zero";
    else if (record_every < 0) why = "record_every below zero";
    else if ((pos_rec == nullptr) != (en_rec == nullptr)) why = "pos_rec and en_rec come together";
    else if (natoms_A != n) why = "the Einstein crystal's natoms must equal n";
    else if (dim_A != dim) why = "the Einstein crystal's dim must equal the target's";
    else if (!(scale > 0.0f)) why = "the Einstein crystal's scale must be positive";
    else if (!(inv_kT == inv_kT) || !(kT == kT)) why = "kT and inv_kT must be numbers";
    else if (seed < 0) why = "seed must be in [0, 2^63)";
    else if (step0 < 0) why = "step below zero";
    else if (batch < 0) why = "bad batch";
    else if (row_base < 0 || row_base > ROWS_MAX || batch > ROWS_MAX - row_base)
        why = "row_base + rows must stay below 2^32";
    else if (nsteps > 0 && lam == nullptr) why = "null schedule";
    else if (nsteps > 0 && (lam_len < 0 || step0 >= lam_len || (int64_t)nsteps >= lam_len - step0))
        why = "the schedule is too short: step0 + nsteps must be below lam_len";
    else if (batch > 0 && (!x_in || !v_in || !x_out || !v_out || !en_out || !centers)) why = "null pointer";
    else if (batch > 1 && (ldxi < width || ldvi < width || ldxo < width || ldvo < width))
        why = "leading dimension below the row width";
    else if (((uintptr_t)work) & 7) why = "work needs 8-byte alignment";
    if (why != nullptr) {
        std::snprintf(buf, sizeof(buf), "%s: %s", who, why);
        return nfk_set_error(buf);
    }
    s.hb = hb;
    s.hd = hd;
    s.c1 = c1;
    s.c2 = c2;
    s.nsteps = nsteps;
    s.record_every = record_every;
    s.step0 = (uint64_t)step0;
    s.frame0 = record_every > 0 ? step0 / record_every : 0;
    s.lam = lam;
    s.inv_kT = inv_kT;
    s.kT = kT;
    key = rng_key(seed, 0, row_base, zero_mean);
    A.cen = centers;
    A.niv = (float)(-1.0 / ((double)scale * (double)scale));
    A.lii = scale;
    A.c2pi = (float)((double)width * std::log(2.0 * M_PI));
    A.hld = (float)((double)n * (double)half_log_det);
    A.hb = (float)(0.5 * boxlength_A);
    A.lf = (float)boxlength_A;
    A.box = has_box ? 1 : 0;
    return 0;
}

// the launch geometry of k_lj_lv / k_eam_lv
struct Geo {
    int G, ppl;
    unsigned grid;
    size_t lds;
};

Geo geo_for(int64_t batch, int n) {
    Geo g;
    g.G = lanes_for(n);
    g.ppl = (n + 63) / 64;
    const int rpb = 4 * (64 / g.G);
    int64_t grid = (batch + rpb - 1) / rpb;
    if (grid > 16384) grid = 16384;
    g.grid = (unsigned)grid;
    g.lds = (size_t)2 * rpb * n * sizeof(float4);  // two buffers per row, <= 32 KiB (n <= 256)
    return g;
}

}  // namespace

// ---------------------------------------------------------------------------
// C ABI
// ---------------------------------------------------------------------------
#define SW_CHECK(who)                                                                                          \
    Sw s;                                                                                                      \
    RngKey key;                                                                                                \
    EinA A;                                                                                                    \
    if (check_sw(who, x_in, ldxi, v_in, ldvi, x_out, ldxo, v_out, ldvo, en_out, batch, n, dim, nsteps, step0,  \
                 row_base, seed, zero_mean, hb, hd, c1, c2, record_every, pos_rec, en_rec, centers, natoms_A,  \
                 dim_A, scale, half_log_det, has_box, boxlength_A, lam, lam_len, inv_kT, kT, work, s, key, A)) \
        return NFK_EINVAL;

#define SW_LAUNCH(SYS, GG, PP)                                                                                  \
    hipLaunchKernelGGL((k_switch<SYS, GG, PP>), dim3(geo.grid), dim3(256), geo.lds, st, x_in, ldxi, v_in, ldvi, \
                       x_out, ldxo, v_out, ldvo, en_out, batch, n, s, key, pos_rec, en_rec, work, A, sys)

#define SW_DISPATCH(SYS)                        \
    do {                                        \
        if (geo.ppl <= 1) {                     \
            NFK_W_DISPATCH(geo.G, SW_CALL1)     \
        } else if (geo.ppl == 2) {              \
            SW_LAUNCH(SYS, 64, 2);              \
        } else if (geo.ppl == 3) {              \
            SW_LAUNCH(SYS, 64, 3);              \
        } else {                                \
            SW_LAUNCH(SYS, 64, 4);              \
        }                                       \
    } while (0)

extern "C" int nfk_lj_switch(const float* x_in, int64_t ldxi, const float* v_in, int64_t ldvi, float* x_out,
                             int64_t ldxo, float* v_out, int64_t ldvo, float* en_out, int64_t batch,
                             int32_t nsteps, int64_t step0, int64_t row_base, int64_t seed, int32_t zero_mean,
                             float hb, float hd, float c1, float c2, int32_t record_every, float* pos_rec,
                             float* en_rec, int32_t n, int32_t dim, double boxlength, double sigma, double epsilon,
                             int32_t has_cutoff, double cutoff, int32_t shift, const float* centers,
                             int32_t natoms_A, int32_t dim_A, float scale, float half_log_det, int32_t has_box,
                             double boxlength_A, const float* lam, int64_t lam_len, double inv_kT, float kT,
                             double* work, nfk_stream_t stream) {
    if (!nfk_lj_supported(n, dim)) return nfk_set_error("nfk_lj_switch: shape not supported");
    if (has_cutoff && !(cutoff > 0.0)) return nfk_set_error("nfk_lj_switch: bad cutoff");
    SW_CHECK("nfk_lj_switch")
    if (batch == 0) return 0;
    hipStream_t st = (hipStream_t)stream;
    const Geo geo = geo_for(batch, n);
    if (dim == 3) {
        LjSys<3> sys;
        sys.k = lj_const(boxlength, sigma, epsilon, has_cutoff, cutoff, shift);
#define SW_CALL1(W) SW_LAUNCH(LjSys<3>, W, 1);
        SW_DISPATCH(LjSys<3>);
#undef SW_CALL1
    } else {
        LjSys<2> sys;
        sys.k = lj_const(boxlength, sigma, epsilon, has_cutoff, cutoff, shift);
#define SW_CALL1(W) SW_LAUNCH(LjSys<2>, W, 1);
        SW_DISPATCH(LjSys<2>);
#undef SW_CALL1
    }
    return launch_status("nfk_lj_switch");
}

extern "C" int nfk_eam_switch(const float* x_in, int64_t ldxi, const float* v_in, int64_t ldvi, float* x_out,
                              int64_t ldxo, float* v_out, int64_t ldvo, float* en_out, int64_t batch,
                              int32_t nsteps, int64_t step0, int64_t row_base, int64_t seed, int32_t zero_mean,
                              float hb, float hd, float c1, float c2, int32_t record_every, float* pos_rec,
                              float* en_rec, int32_t n, const float* rtab, int32_t nr, double dr,
                              const float* ftab, int32_t nrho, double drho, double f_end, double fp_end, double lx,
                              double ly, double lz, double rc, const float* centers, int32_t natoms_A,
                              int32_t dim_A, float scale, float half_log_det, int32_t has_box, double boxlength_A,
                              const float* lam, int64_t lam_len, double inv_kT, float kT, double* work,
                              nfk_stream_t stream) {
    if (!nfk_eam_supported(n)) return nfk_set_error("nfk_eam_switch: shape not supported");
    const int32_t dim = 3;
    SW_CHECK("nfk_eam_switch")
    EamSys sys;
    if (eam_setup("nfk_eam_switch", sys.k, rtab, nr, dr, ftab, nrho, drho, f_end, fp_end, lx, ly, lz, rc))
        return NFK_EINVAL;
    if (batch == 0) return 0;
    if (!rtab || !ftab) return nfk_set_error("nfk_eam_switch: null pointer");
    sys.rtab = (const float4*)rtab;
    sys.ftab = (const float4*)ftab;
    hipStream_t st = (hipStream_t)stream;
    const Geo geo = geo_for(batch, n);
#define SW_CALL1(W) SW_LAUNCH(EamSys, W, 1);
    SW_DISPATCH(EamSys);
#undef SW_CALL1
    return launch_status("nfk_eam_switch");
}
