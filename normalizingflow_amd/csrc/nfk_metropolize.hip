// nfk_metropolize.hip -- the Metropolis chain that uses a batch of flow samples
// as its proposals (applications/src/utils.py:82-99), `chains` independent
// chains of N proposals each in ONE launch.  Chain c reads the rows e[c, :]
// (reduced energies U/kT), lq[c, :] (log proposal densities, optional) and
// r[c, :] (uniforms in [0, 1)); step i proposes sample i:
//   d = e_cur - e[i];  with lq: d = (d + lq_cur) - lq[i]
//   accept iff r[i] < expf(d)          (k_hmc_accept's test; a NaN rejects)
// in fp32 without contraction, and on acceptance (e_cur, lq_cur, idx_cur)
// become (e[i], lq[i], base + i).
//
// One wave runs one chain, four waves form a workgroup, chains are spread
// grid-stride over the workgroups.  A wave takes 64 consecutive proposals at a
// time, one per lane.  Inside such a block e_cur cannot change before the first
// acceptance, so every pending lane evaluates its own test against the current
// state, a wave-wide ballot finds the first lane that accepts, the state moves
// to that lane's values (broadcast) and only the lanes after it stay pending;
// the loop ends when the ballot is empty: 1 + (acceptances in the block)
// rounds, at most 65.  Every decision is the arithmetic above on the operands
// the serial loop would use, so the result has the serial loop's bits.  The
// ballot is wave-uniform, so is every loop exit.  From the block's 64-bit
// accept mask each lane derives its own `state` entry (the highest accepted
// lane at or below it, else the state the block was entered with) and writes
// `state` and `accepted` coalesced.  No LDS, no atomics, nothing crosses
// workgroups; every result is an ordinary vector store by one lane.
#include <hip/hip_runtime.h>

#include <climits>
#include <cstdio>

#include "../../include/nfk.h"
#include "nfk_systems_dev.h"

// 1: the next block's e / lq / r are loaded before the current block resolves
#ifndef NFK_METRO_PREFETCH
#define NFK_METRO_PREFETCH 1
#endif

namespace {

constexpr int kMetroWaves = 4;
constexpr int kMetroGridCap = 4096;

struct MetroArgs {
    const float* e;
    const float* lq;
    const float* r;
    int64_t lde, ldq, ldr;
    int32_t* state;
    int64_t lds;
    uint8_t* accepted;
    int64_t lda;
    int32_t* naccept;
    float* e_cur;
    float* lq_cur;
    int32_t* idx_cur;
    int64_t chains, N;
    int32_t base, carry_in;
};

template <bool HASQ>
__global__ __launch_bounds__(kMetroWaves * 64) void k_metropolize(MetroArgs A) {
    const int lane = threadIdx.x & 63;
    const int64_t N = A.N;
    // lanes [0, lane]: lane 63 gives 2^64 - 1 (the shift wraps to 0)
    const uint64_t upto = (2ull << lane) - 1ull;
    for (int64_t c = (int64_t)blockIdx.x * kMetroWaves + (threadIdx.x >> 6); c < A.chains;
         c += (int64_t)gridDim.x * kMetroWaves) {
        const float* e = A.e + c * A.lde;
        const float* q = HASQ ? A.lq + c * A.ldq : nullptr;
        const float* r = A.r + c * A.ldr;
        float ec, qc = 0.0f;
        int32_t ic;
        if (A.carry_in) {
            ec = A.e_cur[c];
            if (HASQ) qc = A.lq_cur[c];
            ic = A.idx_cur[c];
        } else {  // the chain starts at proposal 0: step 0 compares it with itself
            ec = e[0];
            if (HASQ) qc = q[0];
            ic = A.base;
        }
        int32_t count = 0;
        float en = 0.0f, qn = 0.0f, rn = 0.0f;
        if (NFK_METRO_PREFETCH && lane < N) {
            en = e[lane];
            if (HASQ) qn = q[lane];
            rn = r[lane];
        }
        for (int64_t b0 = 0; b0 < N; b0 += 64) {
            const int64_t i = b0 + lane;
            const bool valid = i < N;
            float ei = 0.0f, qi = 0.0f, ri = 0.0f;
            if (NFK_METRO_PREFETCH) {
                ei = en;
                qi = qn;
                ri = rn;
                if (i + 64 < N) {
                    en = e[i + 64];
                    if (HASQ) qn = q[i + 64];
                    rn = r[i + 64];
                }
            } else if (valid) {
                ei = e[i];
                if (HASQ) qi = q[i];
                ri = r[i];
            }
            uint64_t pending = __ballot(valid);
            uint64_t mask = 0;
            for (;;) {
                float d = ec - ei;
                if (HASQ) d = (d + qc) - qi;
                const bool a = ((pending >> lane) & 1ull) && (ri < expf(d));  // a NaN compares false
                const uint64_t m = __ballot(a);
                if (m == 0) break;  // wave-uniform
                const int f = __ffsll((unsigned long long)m) - 1;
                ec = __shfl(ei, f, 64);
                if (HASQ) qc = __shfl(qi, f, 64);
                mask |= 1ull << f;
                pending &= ~((2ull << f) - 1ull);  // lanes after f; f = 63 leaves none
            }
            const int32_t i0 = A.base + (int32_t)b0;
            if (valid) {
                const uint64_t below = mask & upto;
                if (A.state) A.state[c * A.lds + i] = below ? i0 + 63 - __clzll((long long)below) : ic;
                if (A.accepted) A.accepted[c * A.lda + i] = (uint8_t)((mask >> lane) & 1ull);
            }
            if (mask) ic = i0 + 63 - __clzll((long long)mask);
            count += __popcll(mask);
        }
        if (lane == 0) {
            if (A.naccept) A.naccept[c] += count;
            if (A.e_cur) {
                A.e_cur[c] = ec;
                if (HASQ) A.lq_cur[c] = qc;
                A.idx_cur[c] = ic;
            }
        }
    }
}

}  // namespace

extern "C" int nfk_metropolize(const float* e, int64_t lde, const float* lq, int64_t ldq, const float* r,
                               int64_t ldr, int64_t chains, int64_t N, int32_t base, int32_t carry_in,
                               float* e_cur, float* lq_cur, int32_t* idx_cur, int32_t* state, int64_t lds,
                               uint8_t* accepted, int64_t lda, int32_t* naccept, nfk_stream_t stream) {
    if (chains < 0 || N < 0) return nfk_set_error("nfk_metropolize: bad sizes");
    if (base < 0 || (int64_t)base + N > (int64_t)INT_MAX)
        return nfk_set_error("nfk_metropolize: base must be >= 0 and base + N fit int32");
    if (chains == 0 || N == 0) return 0;
    if (!e || !r) return nfk_set_error("nfk_metropolize: null pointer");
    if ((e_cur == nullptr) != (idx_cur == nullptr))
        return nfk_set_error("nfk_metropolize: e_cur and idx_cur come together");
    if (e_cur ? (lq == nullptr) != (lq_cur == nullptr) : lq_cur != nullptr)
        return nfk_set_error("nfk_metropolize: lq and lq_cur come together");
    if (carry_in && !e_cur) return nfk_set_error("nfk_metropolize: carry_in needs e_cur and idx_cur");
    if (chains > 1 && (lde < N || ldr < N || (lq && ldq < N) || (state && lds < N) || (accepted && lda < N)))
        return nfk_set_error("nfk_metropolize: leading dimension below the row length");
    MetroArgs a;
    a.e = e;
    a.lq = lq;
    a.r = r;
    a.lde = lde;
    a.ldq = ldq;
    a.ldr = ldr;
    a.state = state;
    a.lds = lds;
    a.accepted = accepted;
    a.lda = lda;
    a.naccept = naccept;
    a.e_cur = e_cur;
    a.lq_cur = lq_cur;
    a.idx_cur = idx_cur;
    a.chains = chains;
    a.N = N;
    a.base = base;
    a.carry_in = carry_in ? 1 : 0;
    const int64_t groups = (chains + kMetroWaves - 1) / kMetroWaves;
    const unsigned grid = (unsigned)(groups < kMetroGridCap ? groups : kMetroGridCap);
    hipStream_t st = (hipStream_t)stream;
    if (lq)
        hipLaunchKernelGGL((k_metropolize<true>), dim3(grid), dim3(kMetroWaves * 64), 0, st, a);
    else
        hipLaunchKernelGGL((k_metropolize<false>), dim3(grid), dim3(kMetroWaves * 64), 0, st, a);
    return launch_status("nfk_metropolize");
}
