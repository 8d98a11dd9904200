// nfk_mbar.hip -- multistate free energies (the MBAR self-consistent equations
// behind the `emus` estimate of test.py:61-63 and the driver of test.py:74-88) as
// ONE launch that solves `problems` independent K-state problems to convergence
// and returns, per problem, the free energies f (gauge f_0 = 0), the iteration
// count and the K x K Gram matrix of the weights at f, from which the host
// forms the asymptotic covariance.  One workgroup per problem (256, 512 or 1024
// threads by N * K alone); nothing crosses workgroups, there are no atomics and
// no host sync inside the iteration.  Reduced energies are fp32 and are
// promoted once; every operation after that is fp64, -ffp-contract=off.
//
// One iteration at the current f:
//   pass A   per sample a_k = (log N_k + f_k) - u_nk, W_k = softmax_k(a) in
//            [0, 1]; S_k = sum_n W_nk and G_jk = sum_n W_nj W_nk (j <= k).
//   lane 0   two candidates: the self-consistent step f_sc = f - log(S / N),
//            re-gauged, and the Newton step f_nr = f - H_r^{-1} g_r with
//            g = S - N, H = diag(S) - G, rows and columns 1..K-1 (Cholesky; a
//            pivot that is not > 0 or a non-finite entry makes it invalid).
//   pass B   |S - N|^2 at both candidates.  Newton is taken iff it is valid
//            and its norm is strictly smaller: a NaN falls to the
//            self-consistent step.
//   stop     max_i |f'_i - f_i| < rtol max_i |f'_i| (from the first iteration
//            on), max_iterations, or a NaN iterate, which ends the loop at once
//            and is returned (nfk_bar's rule).
// Every loop exit compares a value that all lanes read from one LDS word, so
// the trip count is workgroup-uniform and bounded by max_iterations.
//
// Reductions are nfk_bar's: lane t of T owns samples t, t + T, ... in that
// order, in the staged form (energies gathered once into LDS, state-major
// [K][N]: a wave's reads of one state are stride-1) and in the streamed form
// (re-read through the index row every pass) alike; a wave reduces by a fixed
// xor butterfly, lane 0 of every wave writes its sums to LDS, and thread v adds
// sum v in wave order.  T follows N * K alone (K >= 6 stops at 512 threads: the
// K + K (K + 1) / 2 accumulators, 44 at K = 8, spill in the 128 registers of a
// 1,024-thread workgroup).  Two runs give the same bits.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdio>

#include "../../include/nfk.h"
#include "nfk_systems_dev.h"

namespace {

constexpr int kMbarMaxK = 8;
// nfk_bar's thresholds and caps, in fp32 energies (N * K)
constexpr int kMbarSmall = 2048;
constexpr int kMbarMid = 65536;
constexpr int kMbarStageCap = 32768;  // 128 KiB of the CU's 160 KiB LDS
constexpr int kMbarGridCap = 4096;
constexpr int kMbarWideK = 6;  // from this K on, no 1,024-thread form
static_assert(kMbarSmall < kMbarStageCap && kMbarStageCap < kMbarMid, "the forms meet inside one workgroup size");

struct MbarArgs {
    const float* u;
    const int32_t* idx;
    int64_t ldu, ldi, N, problems;
    double n[kMbarMaxK], logn[kMbarMaxK], f0[kMbarMaxK];
    double rtol;
    int32_t max_iterations;
    double* f;
    int32_t* iters;
    double* gram;
};

// NaN-propagating max (numpy's np.max): a NaN, once met, stays
__device__ __forceinline__ double nan_max(double m, double t) {
    return (t > m || t != t) ? t : m;
}

// G_jk, j <= k, in the accumulator vector: S[K] first, then the rows of the upper triangle
template <int K>
__host__ __device__ constexpr int gidx(int j, int k) {
    return K + j * K - j * (j - 1) / 2 + (k - j);
}

// W_k = exp(a_k - max a) / sum_k exp(a_k - max a), a_k = c_k - u_k
template <int K>
__device__ __forceinline__ void weights(const double (&u)[K], const double (&c)[K], double (&w)[K]) {
    double m = -INFINITY;
#pragma unroll
    for (int k = 0; k < K; ++k) {
        w[k] = c[k] - u[k];
        m = nan_max(m, w[k]);
    }
    double s = 0.0;
#pragma unroll
    for (int k = 0; k < K; ++k) {
        w[k] = exp(w[k] - m);
        s += w[k];
    }
    const double r = 1.0 / s;
#pragma unroll
    for (int k = 0; k < K; ++k) w[k] *= r;
}

// Sum NV values per thread over the workgroup into tot[NV]: xor butterfly in the
// wave, lane 0 of each wave to `part`, thread v adds sum v in wave order.  Ends
// in a barrier; the caller keeps one between a read of tot and the next call.
template <int NV, int NW>
__device__ __forceinline__ void block_sums(double (&acc)[NV], double (*part)[NV], double* tot) {
#pragma unroll
    for (int v = 0; v < NV; ++v) {
#pragma unroll
        for (int m = 32; m >= 1; m >>= 1) acc[v] += __shfl_xor(acc[v], m, 64);
    }
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
        for (int v = 0; v < NV; ++v) part[wave][v] = acc[v];
    }
    __syncthreads();
    if (threadIdx.x < NV) {
        double t = part[0][threadIdx.x];
#pragma unroll
        for (int w = 1; w < NW; ++w) t += part[w][threadIdx.x];
        tot[threadIdx.x] = t;
    }
    __syncthreads();
}

template <int K, int T, bool STAGED>
__global__ __launch_bounds__(T) void k_mbar(MbarArgs A) {
    constexpr int NW = T / 64, NG = K * (K + 1) / 2, NV = K + NG, R = K - 1;
    static_assert(2 * K <= NV && K * K <= T, "pass B and the gram store fit the pass A scratch");
    extern __shared__ __attribute__((aligned(16))) float s_u[];  // STAGED: [K][N]
    __shared__ double s_part[NW][NV];
    __shared__ double s_tot[NV];
    __shared__ double s_f[K], s_sc[K], s_nr[K];
    __shared__ int s_valid, s_stop;
    const int tid = threadIdx.x;
    const int64_t N = A.N;

    for (int64_t p = blockIdx.x; p < A.problems; p += gridDim.x) {
        const int32_t* ix = A.idx ? A.idx + p * A.ldi : nullptr;
        auto load = [&](int64_t n, double (&u)[K]) {
            if (STAGED) {
#pragma unroll
                for (int k = 0; k < K; ++k) u[k] = (double)s_u[k * N + n];
            } else {
                const float* r = A.u + (ix ? (int64_t)ix[n] : n) * A.ldu;
#pragma unroll
                for (int k = 0; k < K; ++k) u[k] = (double)r[k];
            }
        };
        // pass A at the f in s_f: S and the upper triangle of G into s_tot
        auto pass_a = [&]() {
            double c[K], acc[NV];
#pragma unroll
            for (int k = 0; k < K; ++k) c[k] = A.logn[k] + s_f[k];
#pragma unroll
            for (int v = 0; v < NV; ++v) acc[v] = 0.0;
            for (int64_t n = tid; n < N; n += T) {
                double u[K], w[K];
                load(n, u);
                weights<K>(u, c, w);
#pragma unroll
                for (int k = 0; k < K; ++k) acc[k] += w[k];
#pragma unroll
                for (int j = 0; j < K; ++j) {
#pragma unroll
                    for (int k = j; k < K; ++k) acc[gidx<K>(j, k)] += w[j] * w[k];
                }
            }
            block_sums<NV, NW>(acc, s_part, s_tot);
        };

        if (STAGED) {
            for (int64_t n = tid; n < N; n += T) {
                const float* r = A.u + (ix ? (int64_t)ix[n] : n) * A.ldu;
#pragma unroll
                for (int k = 0; k < K; ++k) s_u[k * N + n] = r[k];
            }
        }
        if (tid == 0) {
#pragma unroll
            for (int k = 0; k < K; ++k) s_f[k] = A.f0[k] - A.f0[0];
        }
        __syncthreads();  // publishes s_u and s_f

        for (int it = 0; it < A.max_iterations; ++it) {
            pass_a();
            if (tid == 0) {
                double S[K], f[K], sc[K], nr[K];
#pragma unroll
                for (int k = 0; k < K; ++k) {
                    S[k] = s_tot[k];
                    f[k] = s_f[k];
                    sc[k] = f[k] - log(S[k] / A.n[k]);
                }
                const double sc0 = sc[0];
#pragma unroll
                for (int k = 0; k < K; ++k) s_sc[k] = sc[k] - sc0;
                // H_r = diag(S) - G on states 1..K-1 = L L^T, then L y = g_r, L^T x = y
                double L[R][R], x[R];
                bool valid = true;
#pragma unroll
                for (int i = 0; i < R; ++i) {
#pragma unroll
                    for (int j = 0; j <= i; ++j) {
                        double h = (i == j ? S[i + 1] : 0.0) - s_tot[gidx<K>(j + 1, i + 1)];
#pragma unroll
                        for (int q = 0; q < j; ++q) h -= L[i][q] * L[j][q];
                        if (i == j) {
                            valid = valid && (h > 0.0);
                            L[i][i] = sqrt(h);
                        } else {
                            L[i][j] = h / L[j][j];
                        }
                    }
                }
#pragma unroll
                for (int i = 0; i < R; ++i) {
                    double y = S[i + 1] - A.n[i + 1];
#pragma unroll
                    for (int q = 0; q < i; ++q) y -= L[i][q] * x[q];
                    x[i] = y / L[i][i];
                }
#pragma unroll
                for (int i = R - 1; i >= 0; --i) {
                    double y = x[i];
#pragma unroll
                    for (int q = i + 1; q < R; ++q) y -= L[q][i] * x[q];
                    x[i] = y / L[i][i];
                }
                nr[0] = f[0];
#pragma unroll
                for (int k = 1; k < K; ++k) {
                    nr[k] = f[k] - x[k - 1];
                    valid = valid && (fabs(nr[k]) < INFINITY);  // false for NaN and +-inf
                }
#pragma unroll
                for (int k = 0; k < K; ++k) s_nr[k] = valid ? nr[k] : s_sc[k];
                s_valid = valid ? 1 : 0;
            }
            __syncthreads();
            // pass B: S at both candidates (an invalid Newton candidate repeats the other)
            {
                double csc[K], cnr[K], acc[NV];
#pragma unroll
                for (int k = 0; k < K; ++k) {
                    csc[k] = A.logn[k] + s_sc[k];
                    cnr[k] = A.logn[k] + s_nr[k];
                }
#pragma unroll
                for (int v = 0; v < NV; ++v) acc[v] = 0.0;
                for (int64_t n = tid; n < N; n += T) {
                    double u[K], w[K];
                    load(n, u);
                    weights<K>(u, csc, w);
#pragma unroll
                    for (int k = 0; k < K; ++k) acc[k] += w[k];
                    weights<K>(u, cnr, w);
#pragma unroll
                    for (int k = 0; k < K; ++k) acc[K + k] += w[k];
                }
                block_sums<NV, NW>(acc, s_part, s_tot);
            }
            if (tid == 0) {
                double n_sc = 0.0, n_nr = 0.0;
#pragma unroll
                for (int k = 0; k < K; ++k) {
                    const double a = s_tot[k] - A.n[k], b = s_tot[K + k] - A.n[k];
                    n_sc += a * a;
                    n_nr += b * b;
                }
                const bool take = s_valid && (n_nr < n_sc);
                double d = 0.0, m = 0.0;
                bool nan = false;
#pragma unroll
                for (int k = 0; k < K; ++k) {
                    const double fn = take ? s_nr[k] : s_sc[k];
                    d = nan_max(d, fabs(fn - s_f[k]));
                    m = nan_max(m, fabs(fn));
                    nan = nan || (fn != fn);
                    s_f[k] = fn;
                }
                const bool stop = nan || (d < A.rtol * m) || (it + 1 == A.max_iterations);
                s_stop = stop ? 1 : 0;
                if (stop) A.iters[p] = it + 1;
            }
            __syncthreads();
            if (s_stop) break;  // one LDS word: the exit is workgroup-uniform
        }

        pass_a();  // the Gram matrix at the returned f
        if (tid < K * K) {
            const int j = tid / K, k = tid % K;
            const int lo = j < k ? j : k, hi = j < k ? k : j;
            A.gram[p * (K * K) + tid] = s_tot[gidx<K>(lo, hi)];
        }
        if (tid < K) A.f[p * K + tid] = s_f[tid];
        __syncthreads();  // the next problem restages s_u and reuses the scratch words
    }
}

template <int K, int T>
void mbar_launch(const MbarArgs& a, unsigned grid, int64_t nk, hipStream_t st) {
    if (nk <= kMbarStageCap) {
        static bool attr = false;  // (every instance sets its dynamic-LDS cap once)
        if (!attr) {
            (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&k_mbar<K, T, true>),
                                      hipFuncAttributeMaxDynamicSharedMemorySize, kMbarStageCap * 4);
            attr = true;
        }
        hipLaunchKernelGGL((k_mbar<K, T, true>), dim3(grid), dim3(T), (size_t)nk * sizeof(float), st, a);
    } else {
        hipLaunchKernelGGL((k_mbar<K, T, false>), dim3(grid), dim3(T), 0, st, a);
    }
}

template <int K>
void mbar_dispatch(const MbarArgs& a, unsigned grid, hipStream_t st) {
    // K >= 6 stays at 512 threads: its K + K (K + 1) / 2 fp64 accumulators need more than
    // the 128 registers a lane of a 1,024-thread workgroup has (88 to 376 bytes of scratch)
    const int64_t nk = a.N * K;
    if (nk <= kMbarSmall) {
        mbar_launch<K, 256>(a, grid, nk, st);
    } else if (nk <= kMbarMid || K >= kMbarWideK) {
        mbar_launch<K, 512>(a, grid, nk, st);
    } else {
        if constexpr (K < kMbarWideK) mbar_launch<K, 1024>(a, grid, nk, st);
    }
}

}  // namespace

extern "C" int nfk_mbar_supported(int32_t K) { return K >= 2 && K <= kMbarMaxK; }

extern "C" int nfk_mbar_stage_cap(void) { return kMbarStageCap; }

extern "C" int nfk_mbar(const float* u, int64_t ldu, int64_t N, int32_t K, const int64_t* n_k, const int32_t* idx,
                        int64_t ldi, int64_t problems, const double* f0, int32_t max_iterations, double rtol,
                        double* f, int32_t* iters, double* gram, nfk_stream_t stream) {
    if (!nfk_mbar_supported(K)) return nfk_set_error("nfk_mbar: K must be 2..8");
    if (N < 1 || !n_k) return nfk_set_error("nfk_mbar: N must be at least 1 and n_k given");
    int64_t total = 0;
    for (int k = 0; k < K; ++k) {
        if (n_k[k] < 1) return nfk_set_error("nfk_mbar: every n_k must be at least 1");
        total += n_k[k];
    }
    if (total != N) return nfk_set_error("nfk_mbar: the n_k must sum to N");
    if (problems < 1) return nfk_set_error("nfk_mbar: problems must be at least 1");
    if (max_iterations < 1) return nfk_set_error("nfk_mbar: max_iterations must be at least 1");
    if (!(rtol >= 0.0)) return nfk_set_error("nfk_mbar: rtol must be a number >= 0");
    if (!u) return nfk_set_error("nfk_mbar: null energies");
    if (!f || !iters || !gram) return nfk_set_error("nfk_mbar: null f, iters or gram");
    if (problems > 1 && !idx) return nfk_set_error("nfk_mbar: problems > 1 needs idx");
    if (ldu < K || (idx && ldi < N)) return nfk_set_error("nfk_mbar: leading dimension below the row length");
    MbarArgs a;
    a.u = u;
    a.idx = idx;
    a.ldu = ldu;
    a.ldi = ldi;
    a.N = N;
    a.problems = problems;
    for (int k = 0; k < kMbarMaxK; ++k) {
        a.n[k] = k < K ? (double)n_k[k] : 1.0;
        a.logn[k] = std::log(a.n[k]);
        a.f0[k] = (k < K && f0) ? f0[k] : 0.0;
    }
    a.rtol = rtol;
    a.max_iterations = max_iterations;
    a.f = f;
    a.iters = iters;
    a.gram = gram;
    const unsigned grid = (unsigned)(problems < kMbarGridCap ? problems : kMbarGridCap);
    hipStream_t st = (hipStream_t)stream;
    switch (K) {
        case 2: mbar_dispatch<2>(a, grid, st); break;
        case 3: mbar_dispatch<3>(a, grid, st); break;
        case 4: mbar_dispatch<4>(a, grid, st); break;
        case 5: mbar_dispatch<5>(a, grid, st); break;
        case 6: mbar_dispatch<6>(a, grid, st); break;
        case 7: mbar_dispatch<7>(a, grid, st); break;
        default: mbar_dispatch<8>(a, grid, st); break;
    }
    return launch_status("nfk_mbar");
}
