// nfk_bar.hip -- the Bennett acceptance ratio of the applications layer
// (applications/src/bar.py:16-68) as ONE launch that solves `problems`
// independent self-consistent iterations to convergence, plus the two
// exponential averages fe_diff needs (test.py:67-68).  One workgroup per
// problem (256, 512 or 1024 threads by the problem's size); nothing crosses
// workgroups, there are no atomics and
// no host sync inside the iteration.  Work values are fp32 and are promoted
// once; every operation after that is fp64, -ffp-contract=off.
//
// Three deliberate deviations from the reference's text:
//   1. g(a) = -log(1 + e^a) is evaluated as -(max(a,0) + log1p(exp(-|a|))).
//      The reference's "stable" form shifts by min(a,0) (np.choose indexed by
//      its own condition) and overflows for |a| >~ 709; the two are the same
//      function and differ by rounding where the reference's is finite.
//   2. A NaN iterate ends the loop at once: it can never recover, and the value
//      returned is the NaN the reference returns after maximum_iterations.
//   3. Every loop exit compares a value that all lanes read from one LDS word,
//      so the trip count is workgroup-uniform and bounded by max_iterations;
//      no data-dependent path can spin.
//
// Each log-sum-exp is shifted by its largest term.  That term is the one of the
// smallest work value (g is non-increasing), so the max pass runs once, over the
// work values in the staging pass, and an iteration is one sum pass.
//
// Reductions: lane t of T owns elements t, t + T, ... in that order, in the staged
// form (work values gathered once into LDS) and in the streamed form (re-read
// through the index rows every pass) alike; a wave reduces by a fixed xor
// butterfly, the wave results go through LDS and are combined in wave order.
// T follows n_f + n_r alone.  Two runs, and the two forms, give the same bits.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdio>

#include "../../include/nfk.h"
#include "nfk_systems_dev.h"

namespace {

// Workgroup size by n_f + n_r alone (never by the form, so the two forms meet at
// the LDS cap with one size and one reduction tree): up to kBarSmall values 256
// threads (the cost is the reduction tree and the barriers), up to kBarMid 512,
// above it 1024 (16 waves, four per SIMD, cover the fp64 exp/log chains).
constexpr int kBarSmall = 2048;
constexpr int kBarMid = 65536;
constexpr int kBarStageCap = 32768;  // fp32 values: 128 KiB of the CU's 160 KiB LDS
constexpr int kBarGridCap = 4096;
static_assert(kBarSmall < kBarStageCap && kBarStageCap < kBarMid, "the forms meet inside one workgroup size");

struct BarArgs {
    const float* w_f;
    const float* w_r;
    const int32_t* idx_f;
    const int32_t* idx_r;
    int64_t n_f, n_r, ldif, ldir, problems;
    double delta0, rtol, M, log_nf, log_nr;
    int32_t max_iterations;
    double* out;
    int32_t* iters;
};

// g(a) = -log(1 + e^a), finite for every finite a
__device__ __forceinline__ double bar_g(double a) {
    return -(fmax(a, 0.0) + log1p(exp(-fabs(a))));
}

// NaN-propagating max (numpy's np.max): a NaN, once met, stays
__device__ __forceinline__ double nan_max(double m, double t) {
    return (t > m || t != t) ? t : m;
}

struct OpMax {
    static __device__ __forceinline__ double id() { return -INFINITY; }
    static __device__ __forceinline__ double op(double a, double b) { return nan_max(a, b); }
};
struct OpSum {
    static __device__ __forceinline__ double id() { return 0.0; }
    static __device__ __forceinline__ double op(double a, double b) { return a + b; }
};

// Reduce two values per thread over the workgroup: xor butterfly in the wave,
// then the wave results in wave order out of `part` (one barrier; the caller
// keeps a barrier between two uses of the same `part`).
template <class Op, int NW>
__device__ __forceinline__ void block_reduce2(double& a, double& b, double (*part)[2]) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
        a = Op::op(a, __shfl_xor(a, m, 64));
        b = Op::op(b, __shfl_xor(b, m, 64));
    }
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) {
        part[wave][0] = a;
        part[wave][1] = b;
    }
    __syncthreads();
    a = part[0][0];
    b = part[0][1];
#pragma unroll
    for (int w = 1; w < NW; ++w) {
        a = Op::op(a, part[w][0]);
        b = Op::op(b, part[w][1]);
    }
}

template <int T, bool STAGED>
__global__ __launch_bounds__(T) void k_bar(BarArgs A) {
    constexpr int kBarThreads = T, NW = T / 64;
    extern __shared__ __attribute__((aligned(16))) float s_w[];  // STAGED: wf[n_f] then wr[n_r]
    __shared__ double s_pa[NW][2], s_pb[NW][2];
    __shared__ double s_delta;
    __shared__ int s_stop;
    const int tid = threadIdx.x;
    const int64_t n_f = A.n_f, n_r = A.n_r;

    for (int64_t p = blockIdx.x; p < A.problems; p += gridDim.x) {
        const int32_t* ixf = A.idx_f ? A.idx_f + p * A.ldif : nullptr;
        const int32_t* ixr = A.idx_r ? A.idx_r + p * A.ldir : nullptr;
        auto load_f = [&](int64_t i) -> double {
            if (STAGED) return (double)s_w[i];
            return (double)A.w_f[ixf ? (int64_t)ixf[i] : i];
        };
        auto load_r = [&](int64_t i) -> double {
            if (STAGED) return (double)s_w[n_f + i];
            return (double)A.w_r[ixr ? (int64_t)ixr[i] : i];
        };

        // staging pass: gather (STAGED), the maxima (shifts of the exponential
        // averages) and the minima (they carry the iteration's shifts) of the work values
        double mf = OpMax::id(), mr = OpMax::id(), lf = OpMax::id(), lr = OpMax::id();
        for (int64_t i = tid; i < n_f; i += kBarThreads) {
            const float w = A.w_f[ixf ? (int64_t)ixf[i] : i];
            if (STAGED) s_w[i] = w;
            mf = nan_max(mf, (double)w);
            lf = nan_max(lf, -(double)w);
        }
        for (int64_t i = tid; i < n_r; i += kBarThreads) {
            const float w = A.w_r[ixr ? (int64_t)ixr[i] : i];
            if (STAGED) s_w[n_f + i] = w;
            mr = nan_max(mr, (double)w);
            lr = nan_max(lr, -(double)w);
        }
        block_reduce2<OpMax, NW>(mf, mr, s_pa);  // its barrier also publishes s_w
        block_reduce2<OpMax, NW>(lf, lr, s_pb);
        const double wmin_f = -lf, wmin_r = -lr;
        double sf = 0.0, sr = 0.0;
        for (int64_t i = tid; i < n_f; i += kBarThreads) sf += exp(load_f(i) - mf);
        for (int64_t i = tid; i < n_r; i += kBarThreads) sr += exp(load_r(i) - mr);
        block_reduce2<OpSum, NW>(sf, sr, s_pa);
        if (tid == 0) {
            A.out[p * 3 + 1] = (log(sf) + mf) - A.log_nf;
            A.out[p * 3 + 2] = (log(sr) + mr) - A.log_nr;
        }

        double delta = A.delta0;
        for (int k = 0; k < A.max_iterations; ++k) {
            // The max pass, hoisted: g is non-increasing, and so is g(M - w - D) - w
            // in w (its slope is sigmoid(a) - 1), so the largest term of either sum
            // is that of the smallest work value, found once above.  Every lane
            // evaluates the two shifts from the same words; a NaN work value is a
            // NaN minimum and a NaN shift, as it is a NaN maximum in a max pass.
            const double tf = bar_g((A.M + wmin_f) - delta);
            const double tr = bar_g((A.M - wmin_r) - delta) - wmin_r;
            // sum pass
            double af = 0.0, ar = 0.0;
            for (int64_t i = tid; i < n_f; i += kBarThreads)
                af += exp(bar_g((A.M + load_f(i)) - delta) - tf);
            for (int64_t i = tid; i < n_r; i += kBarThreads) {
                const double w = load_r(i);
                ar += exp((bar_g((A.M - w) - delta) - w) - tr);
            }
            block_reduce2<OpSum, NW>(af, ar, s_pb);
            if (tid == 0) {
                const double log_numer = (log(af) + tf) - A.log_nf;
                const double log_denom = (log(ar) + tr) - A.log_nr;
                const double next = log_denom - log_numer;
                const double rc = fabs((next - delta) / next);
                const bool stop = (next != next) || (k > 0 && rc < A.rtol) || (k + 1 == A.max_iterations);
                s_delta = next;
                s_stop = stop ? 1 : 0;
                if (stop) {
                    A.out[p * 3] = next;
                    A.iters[p] = k + 1;
                }
            }
            __syncthreads();
            delta = s_delta;
            if (s_stop) break;  // one LDS word: the exit is workgroup-uniform
        }
        __syncthreads();  // the next problem restages s_w and reuses the scratch words
    }
}

template <int T>
void bar_launch(const BarArgs& a, unsigned grid, int64_t n, hipStream_t st) {
    if (n <= kBarStageCap) {
        static bool attr = false;  // (every instance sets its dynamic-LDS cap once)
        if (!attr) {
            (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&k_bar<T, true>),
                                      hipFuncAttributeMaxDynamicSharedMemorySize, kBarStageCap * 4);
            attr = true;
        }
        hipLaunchKernelGGL((k_bar<T, true>), dim3(grid), dim3(T), (size_t)n * sizeof(float), st, a);
    } else {
        hipLaunchKernelGGL((k_bar<T, false>), dim3(grid), dim3(T), 0, st, a);
    }
}

}  // namespace

extern "C" int nfk_bar_stage_cap(void) { return kBarStageCap; }

extern "C" int nfk_bar(const float* w_f, int64_t n_f, const float* w_r, int64_t n_r, const int32_t* idx_f,
                       int64_t ldif, const int32_t* idx_r, int64_t ldir, int64_t problems, double delta0,
                       int32_t max_iterations, double rtol, double* out, int32_t* iters,
                       nfk_stream_t stream) {
    if (n_f < 1 || n_r < 1) return nfk_set_error("nfk_bar: n_f and n_r must be at least 1");
    if (problems < 1) return nfk_set_error("nfk_bar: problems must be at least 1");
    if (max_iterations < 1) return nfk_set_error("nfk_bar: max_iterations must be at least 1");
    if (!(rtol >= 0.0)) return nfk_set_error("nfk_bar: rtol must be a number >= 0");
    if (!w_f || !w_r) return nfk_set_error("nfk_bar: null work values");
    if (!out || !iters) return nfk_set_error("nfk_bar: null out or iters");
    if (problems > 1 && ((idx_f == nullptr) != (idx_r == nullptr)))
        return nfk_set_error("nfk_bar: idx_f and idx_r come together when problems > 1");
    if ((idx_f && ldif < n_f) || (idx_r && ldir < n_r))
        return nfk_set_error("nfk_bar: leading dimension below the row length");
    BarArgs a;
    a.w_f = w_f;
    a.w_r = w_r;
    a.idx_f = idx_f;
    a.idx_r = idx_r;
    a.n_f = n_f;
    a.n_r = n_r;
    a.ldif = ldif;
    a.ldir = ldir;
    a.problems = problems;
    a.delta0 = delta0;
    a.rtol = rtol;
    a.M = std::log((double)n_f / (double)n_r);
    a.log_nf = std::log((double)n_f);
    a.log_nr = std::log((double)n_r);
    a.max_iterations = max_iterations;
    a.out = out;
    a.iters = iters;
    const unsigned grid = (unsigned)(problems < kBarGridCap ? problems : kBarGridCap);
    hipStream_t st = (hipStream_t)stream;
    const int64_t n = n_f + n_r;
    if (n <= kBarSmall)
        bar_launch<256>(a, grid, n, st);
    else if (n <= kBarMid)
        bar_launch<512>(a, grid, n, st);
    else
        bar_launch<1024>(a, grid, n, st);
    return launch_status("nfk_bar");
}
