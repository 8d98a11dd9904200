// nfk_eam.hip -- the embedded-atom energy of a periodic orthorhombic box from
// setfl tables (systems.py EAM) and its gradient, one launch per batch.
//   rho_i = sum_(j,s) f(r_ijs),  U = sum_i F(rho_i) + 1/2 sum_i sum_(j,s) z(r_ijs) / r_ijs
// over every periodic image within the cutoff (include/nfk.h).  Pairwise VALU
// kernels with nfk_systems.hip's conventions: -ffp-contract=off, every sum in a
// fixed order, no float atomics.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <cstdio>

#include "../../include/nfk.h"
#include "nfk_systems_dev.h"

namespace {

// The row layout of k_lj: a row occupies G lanes (64 / G rows per wave, 4 waves per
// block), lane c0 owns atoms c0 + q G, q < PPL (PPL > 1 only with G == 64), and the
// block's rows are staged in LDS as float4 per atom, read by broadcast in the j
// loop.  A row never leaves its wave.  The r-tables (32 B per interval) and the F
// table are read through the vector cache (an LDS-staged r-table measured twice as
// slow at large batches: DESIGN.md section 11.1).
// Forward: out[b] = sum_i (F(rho_i) + e_i / 2), the lanes' shares summed by the
// group butterfly.  Backward: a first (j, s) loop gives rho_i; the lane leaves
// F'(rho_i) in the .w of its atoms' LDS slots; after a barrier the second loop
// reads F'(rho_j) with x_j and each lane writes g[b] dU/dx_i of its own atoms.
// The second loop skips j == i: the self images' r does not depend on x_i.
template <int G, int PPL, bool BWD>
__global__ __launch_bounds__(256) void k_eam(const float* __restrict__ x, int64_t ldx,
                                             const float* __restrict__ g, float* out, int64_t ldo,
                                             int64_t batch, int n, const float4* __restrict__ rtab,
                                             const float4* __restrict__ ftab, EamConst k) {
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
                const float* p = x + b * ldx + (int64_t)i * 3;
                xi[q][0] = p[0];
                xi[q][1] = p[1];
                xi[q][2] = p[2];
                srow[i] = make_float4(xi[q][0], xi[q][1], xi[q][2], 0.0f);
            }
        }
        __syncthreads();
        float rho[PPL], e[PPL], f[PPL][3];
#pragma unroll
        for (int q = 0; q < PPL; ++q) rho[q] = e[q] = f[q][0] = f[q][1] = f[q][2] = 0.0f;
        if (ok)
            for (int j = 0; j < n; ++j) {
                const float4 pj = srow[j];
#pragma unroll
                for (int q = 0; q < PPL; ++q)
                    if (c0 + q * G < n) eam_pair<BWD ? 1 : 0>(xi[q], pj, 0.0f, k, rtab, rho[q], e[q], f[q]);
            }
        if (!BWD) {
            float u = 0.0f;
#pragma unroll
            for (int q = 0; q < PPL; ++q)
                if (ok && c0 + q * G < n) u += eam_embed<false>(rho[q], ftab, k) + 0.5f * e[q];
            u = group_sum<G>(u);
            if (ok && c0 == 0) out[b] = u;
        } else {
            float fpi[PPL];
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
            if (ok) {
                for (int j = 0; j < n; ++j) {
                    const float4 pj = srow[j];
#pragma unroll
                    for (int q = 0; q < PPL; ++q) {
                        const int i = c0 + q * G;
                        if (i < n && i != j)
                            eam_pair<2>(xi[q], pj, fpi[q] + pj.w, k, rtab, rho[q], e[q], f[q]);
                    }
                }
                const float gb = g[b];
#pragma unroll
                for (int q = 0; q < PPL; ++q) {
                    const int i = c0 + q * G;
                    if (i < n) {
                        float* p = out + b * ldo + (int64_t)i * 3;
                        p[0] = gb * f[q][0];
                        p[1] = gb * f[q][1];
                        p[2] = gb * f[q][2];
                    }
                }
            }
        }
        __syncthreads();  // the next round overwrites the staged rows
    }
}

template <bool BWD>
void eam_launch(const float* x, int64_t ldx, const float* g, float* out, int64_t ldo, int64_t batch, int n,
                const float* rtab, const float* ftab, const EamConst& k, hipStream_t st) {
    const int G = lanes_for(n);
    const int ppl = (n + 63) / 64;
    const unsigned grid = grid_for_rows(batch, G);
    const size_t lds = (size_t)(4 * (64 / G)) * n * sizeof(float4);  // <= 16 KiB (n <= 256)
#define EAM_CALL2(GG, PP)                                                                           \
    hipLaunchKernelGGL((k_eam<GG, PP, BWD>), dim3(grid), dim3(256), lds, st, x, ldx, g, out, ldo, batch, \
                       n, (const float4*)rtab, (const float4*)ftab, k)
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
}

int eam_check(const char* who, const void* x, const void* rtab, const void* ftab, int64_t ldx,
              int64_t batch, int n) {
    char buf[120];
    const char* why = nullptr;
    if (batch < 0) why = "bad batch";
    else if (!nfk_eam_supported(n)) why = "shape not supported";
    else if (batch > 0 && (!x || !rtab || !ftab)) why = "null pointer";
    else if ((((uintptr_t)rtab) | ((uintptr_t)ftab)) & 15) why = "tables need 16-byte alignment";
    else if (ldx < (int64_t)n * 3 && batch > 1) why = "leading dimension below the row width";
    if (!why) return 0;
    std::snprintf(buf, sizeof(buf), "%s: %s", who, why);
    return nfk_set_error(buf);
}

}  // namespace

extern "C" int nfk_eam_supported(int32_t n) { return (n >= 1 && n <= 256) ? 1 : 0; }

extern "C" int nfk_eam_potential(const float* x, int64_t ldx, float* out, int64_t batch, int32_t n,
                                 const float* rtab, int32_t nr, double dr, const float* ftab,
                                 int32_t nrho, double drho, double f_end, double fp_end, double lx,
                                 double ly, double lz, double rc, nfk_stream_t stream) {
    if (int rcode = eam_check("nfk_eam_potential", x, rtab, ftab, ldx, batch, n)) return rcode;
    EamConst k;
    if (eam_const(k, nr, dr, nrho, drho, f_end, fp_end, lx, ly, lz, rc))
        return nfk_set_error("nfk_eam_potential: bad tables, box or cutoff");
    if (batch == 0) return 0;
    if (!out) return nfk_set_error("nfk_eam_potential: null pointer");
    eam_launch<false>(x, ldx, nullptr, out, 0, batch, n, rtab, ftab, k, (hipStream_t)stream);
    return launch_status("nfk_eam_potential");
}

extern "C" int nfk_eam_potential_bwd(const float* x, int64_t ldx, const float* g, float* gx, int64_t ldgx,
                                     int64_t batch, int32_t n, const float* rtab, int32_t nr, double dr,
                                     const float* ftab, int32_t nrho, double drho, double f_end,
                                     double fp_end, double lx, double ly, double lz, double rc,
                                     nfk_stream_t stream) {
    if (int rcode = eam_check("nfk_eam_potential_bwd", x, rtab, ftab, ldx < ldgx ? ldx : ldgx, batch, n))
        return rcode;
    EamConst k;
    if (eam_const(k, nr, dr, nrho, drho, f_end, fp_end, lx, ly, lz, rc))
        return nfk_set_error("nfk_eam_potential_bwd: bad tables, box or cutoff");
    if (batch == 0) return 0;
    if (!g || !gx) return nfk_set_error("nfk_eam_potential_bwd: null pointer");
    eam_launch<true>(x, ldx, g, gx, ldgx, batch, n, rtab, ftab, k, (hipStream_t)stream);
    return launch_status("nfk_eam_potential_bwd");
}
