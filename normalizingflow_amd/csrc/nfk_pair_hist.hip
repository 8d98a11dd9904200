// nfk_pair_hist.hip -- the weighted pair-distance histogram of a batch of
// (periodic) configurations, the counts behind g(r):
//   hist[k] = sum_b w_b * #{ i < j : floor(r_ij(b) * nbins / r_max) == k, r_ij(b) < r_max }.
// x holds `batch` rows of n * dim fp32, w one fp64 weight per row (null: 1).
//
// Pair arithmetic, fp32: d = x_i - x_j per component; with a box the minimum
// image d - L * rint(d * (1 / L)) (any displacement, not only one box length);
// r = sqrt(sum d^2); the pair counts in bin k = (int)(r * (float)(nbins / r_max))
// iff r < (float)r_max and k < nbins.  A NaN or infinite r fails the first
// compare and lands in no bin; there is no status word.
//
// Mapping.  A wave takes one row at a time: the row is staged as float4 per
// particle in LDS, and the n (n - 1) / 2 pairs are walked as (i, i + k mod n),
// k = 1 .. n / 2 (for even n the last k only from i < n / 2), which visits every
// unordered pair once.  The wave's 64 lanes split into 64 / G groups of
// G = min(64, pow2ceil(n)) lanes: lane i0 of group s owns particles i0, i0 + G, ..
// and the offsets k = 1 + s, 1 + s + 64 / G, ..  Bin counts of a row are uint32 in
// the wave's own LDS histogram (ds_add_u32: integer adds commute, so the order
// of the lanes does not matter).  When the row is done the wave folds it into
// its fp64 LDS accumulator, acc[k] += w_b * (double)count[k], and clears the
// counts: nbins / 64 steps.  That is the only place a weight enters.
//
// Order.  Workgroup g of `parts` (a function of batch alone, nfk_pair_hist_parts)
// has four waves; wave v takes rows (t * parts + g) * 4 + v, t = 0, 1, ..  At the
// end the workgroup adds its four accumulators in wave order and stores partial g
// to the workspace [parts, nbins]; k_pair_hist_reduce, the second launch on the
// same stream, adds the partials in index order.  No floating-point atomics, no
// host sync; two runs give the same bits, and with unit weights every sum is an
// integer below 2^53, hence exact.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdio>

#include "../../include/nfk.h"
#include "nfk_systems_dev.h"

namespace {

constexpr int kPhMaxN = 256;
constexpr int kPhMaxBins = 1024;
constexpr int kPhThreads = 256;
// lanes that share a row and its histogram: 64, one wave per row.  256, the whole
// workgroup on one row with one histogram, measured 1.1x to 1.7x slower at every
// shape timed; the kernel is written for either.
constexpr int kPhTeam = 64;
constexpr int kPhRowsPerBlock = kPhThreads / kPhTeam;
constexpr int kPhMaxParts = 1024;  // four workgroups per CU
static_assert(kPhTeam == 64 || kPhTeam == 256, "a row is walked by one wave or by the workgroup");

struct PhArgs {
    const float* x;
    const double* w;
    int64_t ldx, batch;
    int n, dim, nbins, lg;  // lg = log2 of the lane group G
    float lf[3], il[3];     // (float)L_a, (float)(1 / L_a)
    float rmax, scale;      // (float)r_max, (float)(nbins / r_max)
    double* part;
};

template <int TEAM, bool BOX>
__global__ __launch_bounds__(kPhThreads) void k_pair_hist(PhArgs A) {
    extern __shared__ __attribute__((aligned(16))) float4 s_pos[];  // [RPB][n], then acc, then counts
    constexpr int RPB = kPhThreads / TEAM;
    const int n = A.n, nb = A.nbins;
    double* s_acc = reinterpret_cast<double*>(s_pos + RPB * n);  // [RPB][nbins]
    unsigned* s_cnt = reinterpret_cast<unsigned*>(s_acc + RPB * nb);  // [RPB][nbins]
    const int team = threadIdx.x / TEAM, tl = threadIdx.x % TEAM;
    float4* srow = s_pos + team * n;
    double* acc = s_acc + team * nb;
    unsigned* cnt = s_cnt + team * nb;
    for (int k = tl; k < nb; k += TEAM) {
        acc[k] = 0.0;
        cnt[k] = 0u;
    }
    const int G = 1 << A.lg;
    const int i0 = tl & (G - 1), k0 = 1 + (tl >> A.lg), kstep = TEAM >> A.lg;
    const int kmax = n >> 1;
    const int ilast = (n & 1) ? n : kmax;  // at k == kmax an even n counts i < n / 2 only
    // every team of the workgroup makes the same number of trips: the barriers are uniform
    for (int64_t r0 = (int64_t)blockIdx.x * RPB; r0 < A.batch; r0 += (int64_t)gridDim.x * RPB) {
        const int64_t b = r0 + team;
        const bool ok = b < A.batch;
        if (ok) {
            const float* xr = A.x + b * A.ldx;
            for (int i = tl; i < n; i += TEAM) {
                const float* p = xr + (int64_t)i * A.dim;
                srow[i] = make_float4(p[0], p[1], A.dim == 3 ? p[2] : 0.0f, 0.0f);
            }
        }
        __syncthreads();  // the staged rows (first trip: the cleared histograms too)
        if (ok) {
            for (int i = i0; i < n; i += G) {
                const float4 pi = srow[i];
                for (int k = k0; k <= kmax; k += kstep) {
                    if (k == kmax && i >= ilast) break;
                    int j = i + k;
                    j = j >= n ? j - n : j;
                    const float4 pj = srow[j];
                    float dx = pi.x - pj.x, dy = pi.y - pj.y, dz = pi.z - pj.z;
                    if (BOX) {
                        dx = dx - A.lf[0] * rintf(dx * A.il[0]);
                        dy = dy - A.lf[1] * rintf(dy * A.il[1]);
                        dz = dz - A.lf[2] * rintf(dz * A.il[2]);  // dim 2: lf[2] = 0, dz = 0
                    }
                    const float r = sqrtf(dx * dx + dy * dy + dz * dz);
                    if (r < A.rmax) {  // false for a NaN; r >= 0, so the cast below is the floor
                        const int bin = (int)(r * A.scale);
                        if (bin < nb) atomicAdd(&cnt[bin], 1u);
                    }
                }
            }
        }
        __syncthreads();  // the row's counts are complete
        if (ok) {
            const double wb = A.w ? A.w[b] : 1.0;
            for (int k = tl; k < nb; k += TEAM) {
                acc[k] += wb * (double)cnt[k];
                cnt[k] = 0u;
            }
        }
    }
    __syncthreads();
    for (int k = threadIdx.x; k < nb; k += kPhThreads) {
        double t = s_acc[k];
#pragma unroll
        for (int v = 1; v < RPB; ++v) t += s_acc[v * nb + k];
        A.part[(int64_t)blockIdx.x * nb + k] = t;
    }
}

// hist[k] = part[0][k] + part[1][k] + ... in index order; parts == 0 writes zeros
__global__ __launch_bounds__(256) void k_pair_hist_reduce(const double* __restrict__ part, int parts, int nb,
                                                          double* __restrict__ hist) {
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= nb) return;
    double t = 0.0;
#pragma unroll 8
    for (int p = 0; p < parts; ++p) t += part[(int64_t)p * nb + k];
    hist[k] = t;
}

}  // namespace

extern "C" int nfk_pair_hist_supported(int32_t n, int32_t dim, int32_t nbins) {
    return n >= 1 && n <= kPhMaxN && (dim == 2 || dim == 3) && nbins >= 1 && nbins <= kPhMaxBins;
}

extern "C" int64_t nfk_pair_hist_parts(int64_t batch) {
    if (batch <= 0) return 0;
    const int64_t g = (batch + kPhRowsPerBlock - 1) / kPhRowsPerBlock;
    return g < kPhMaxParts ? g : kPhMaxParts;
}

extern "C" int64_t nfk_pair_hist_workspace_elems(int64_t batch, int32_t nbins) {
    return nbins >= 1 ? nfk_pair_hist_parts(batch) * (int64_t)nbins : 0;
}

extern "C" int nfk_pair_hist(const float* x, int64_t ldx, const double* w, int64_t batch, int32_t n, int32_t dim,
                             double lx, double ly, double lz, double r_max, int32_t nbins, double* hist,
                             double* workspace, nfk_stream_t stream) {
    if (!nfk_pair_hist_supported(n, dim, nbins))
        return nfk_set_error("nfk_pair_hist: shape not supported (n 1..256, dim 2 or 3, nbins 1..1024)");
    if (batch < 0) return nfk_set_error("nfk_pair_hist: bad batch");
    if (!hist) return nfk_set_error("nfk_pair_hist: null hist");
    if (batch > 0 && (!x || !workspace)) return nfk_set_error("nfk_pair_hist: null x or workspace");
    if (!(r_max > 0.0) || !(r_max < INFINITY)) return nfk_set_error("nfk_pair_hist: r_max must be a number > 0");
    const double L[3] = {lx, ly, dim == 3 ? lz : lx};
    int npos = 0;
    double lmin = INFINITY;
    for (int a = 0; a < 3; ++a) {
        if (!(L[a] >= 0.0) || !(L[a] < INFINITY)) return nfk_set_error("nfk_pair_hist: bad box length");
        npos += L[a] > 0.0;
        lmin = L[a] < lmin ? L[a] : lmin;
    }
    if (npos != 0 && npos != 3)
        return nfk_set_error("nfk_pair_hist: the box lengths are all positive or all zero (no box)");
    if (npos && r_max > 0.5 * lmin) return nfk_set_error("nfk_pair_hist: r_max above half the shortest box length");
    if (ldx < (int64_t)n * dim && batch > 1) return nfk_set_error("nfk_pair_hist: ldx below the row width");
    hipStream_t st = (hipStream_t)stream;
    const int parts = (int)nfk_pair_hist_parts(batch);
    if (parts > 0) {
        PhArgs a;
        a.x = x;
        a.w = w;
        a.ldx = ldx;
        a.batch = batch;
        a.n = n;
        a.dim = dim;
        a.nbins = nbins;
        a.lg = 0;
        while ((1 << a.lg) < n && (1 << a.lg) < kPhTeam) ++a.lg;
        for (int c = 0; c < 3; ++c) {
            const bool on = npos && (c < dim);
            a.lf[c] = on ? (float)L[c] : 0.0f;
            a.il[c] = on ? (float)(1.0 / L[c]) : 0.0f;
        }
        a.rmax = (float)r_max;
        a.scale = (float)((double)nbins / r_max);
        a.part = workspace;
        // <= 16 KiB of positions, 32 KiB of accumulators, 16 KiB of counts
        const size_t lds = (size_t)kPhRowsPerBlock * ((size_t)n * sizeof(float4) + (size_t)nbins * 12);
        if (npos)
            hipLaunchKernelGGL((k_pair_hist<kPhTeam, true>), dim3((unsigned)parts), dim3(kPhThreads), lds, st, a);
        else
            hipLaunchKernelGGL((k_pair_hist<kPhTeam, false>), dim3((unsigned)parts), dim3(kPhThreads), lds, st, a);
        const int rc = launch_status("nfk_pair_hist");
        if (rc) return rc;
    }
    hipLaunchKernelGGL(k_pair_hist_reduce, dim3((unsigned)((nbins + 255) / 256)), dim3(256), 0, st, workspace, parts,
                       nbins, hist);
    return launch_status("nfk_pair_hist");
}
