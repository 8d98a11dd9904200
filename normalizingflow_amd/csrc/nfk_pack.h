// nfk_pack.h -- the fp16-split weight-pack format: what every packer writes
// and every fused kernel reads.  The pack kernels (and which records follow
// the header, in which order) stay with their kernel families.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace nfk_fused {

// ---------------------------------------------------------------------------
// Packed weights ("pack"): a header block, then a stream of phase records.
// A record is a run of 1-KiB blocks (64 lanes x 16 B, one wave-instruction of
// global_load_lds each) followed by one bias block (float[16 tiles][16 rows]).
//   header (1 block): hdr[0..2] = max|W1|, max|W2|, max|W3| (uint bits, from
//            the pack's reduction); float hdr[3..5] = the factors undoing the
//            fp16 pre-scaling, 2^s putting max|W| of a Linear in [2^14, 2^15);
//            every other word 0 unless a variant says otherwise:
//              NSF (k_pack, k_pack_frames): hdr[3] = 2^-s1, hdr[4] = 2^-(s2+14),
//                hdr[5] = 2^-(s3+14).  The layer-1 bias is left unscaled: x is
//                scaled per sample, so the kernel adds the bias after unscaling.
//              AR / CL (k_ar_pack, k_ars_pack, k_cl_pack): the layer-1 input is
//                split at 2^14 like every activation and its bias is pre-scaled
//                by 2^(s1+14): hdr[3] = 2^-(s1+14).  The AR forms carry
//                init_param[3K-1] from hdr[8].
//              RealNVP (k_rnvp_pack): 12 Linears m = (2 pair + net) 3 + layer:
//                hdr[m] = max|W_m|, hdr[16 + m] = 2^-s_m for layer 0 (bias
//                unscaled, as NSF), 2^-(s_m+14) for layers 1, 2.
//   f16 blocks (v_mfma_f32_16x16x32_f16, two-way split): k-blocks x NT tiles
//            x {hi, lo}: lane l of block (kb, t, p) holds part p of
//            2^s W[row(t, l&15)][32kb + 8(l>>4) + j], j = 0..7, where hi = f16(v),
//            lo = f16(v - hi) and 2^s puts max|W| in [2^14, 2^15)
//   tail (T1 only: H = 32 KBH + R, 0 < R <= 4, one v_mfma_f32_16x16x16_f16
//            per tile): one block per 2 tiles; lane l's 16 B hold tile 2g's
//            then tile 2g + 1's fragment, 4 halves over the tail features
//            32 KBH + 0..3 of row(t, l&15): k-group l>>4 = {hi, hi, lo, 0} of 2^s W, against
//            the B groups {a_hi, a_lo, a_hi, -} (tail_word, act_operands): the
//            same three split products as the k-blocks, in one f16 MFMA
//   layer 1: KB1 = ceil(n_lo/32) f16 k-blocks (x is scaled per sample, by a power of two), bias unscaled
//   layer 2: KBH f16 k-blocks (+ tail blocks), bias pre-scaled by 2^(s2+14)
//   per 16-coordinate chunk: W logits (K tiles), H logits (K tiles), D logits
//            (K-1 tiles), same form; row i of tile t = parameter t of coordinate 16c+i
// Hidden feature permutation: row i of hidden tile t < 2 KBH computes feature
//   f(t, i) = 32(t>>1) + 8(i>>2) + 4(t&1) + (i&3),
// so accumulator register r of tiles 2kb, 2kb+1 of lane l are exactly
// elements j = r, 4 + r of the next product's B fragment for k-block kb
// (k = 32kb + 8(l>>4) + j) -- activations never leave registers.  With a
// tail, tile 2 KBH holds features 32 KBH + r in register r of every lane
// group (rows duplicated): the B operand of the tail step needs all R in
// each lane.
// wide = 1 (nfk_fused_wide.h): the output layer in 8-coordinate chunks whose
//   W/H/D records have ceil(K/2) tiles; row i of tile t = parameter
//   2t + (i&1) of coordinate 8c + 2(i>>2) + ((i>>1)&1), so lane group q holds
//   two coordinates with all their parameters in registers 2h, 2h+1 of the
//   tiles (half the accumulators of the 16-coordinate form).
constexpr int kHdrWords = 256;       // the header block
constexpr int kHdrMax = 0;           // + layer: max|W| as uint bits
constexpr int kHdrUnscale = 3;       // + layer: float unscale factor
constexpr int kHdrInit = 8;          // AR: init_param[3K-1]
constexpr int kHdrRnvpUnscale = 16;  // RealNVP: + m (maxima at kHdrMax + m)

// hidden feature computed by row i (0..15) of hidden tile t (>= H: padding)
__host__ __device__ inline int hid_feature(int t, int i, int kbh) {
    if (t < 2 * kbh) return 32 * (t >> 1) + 8 * (i >> 2) + 4 * (t & 1) + (i & 3);
    return 32 * kbh + (i & 3);  // the tail tile: every lane group holds the tail features
}

// power-of-two exponent s with max|W| 2^s in [2^14, 2^15) (0 for an all-zero or non-finite Linear)
__device__ inline int nfk_scale_exp(float maxw) {
    if (!(maxw > 0.0f) || !(maxw < 3.0e38f)) return 0;
    int e;
    frexpf(maxw, &e);  // maxw = m 2^e, m in [0.5, 1)
    return 15 - e;
}

// f16 pair (v0, v1) of split part p (0 = hi, 1 = lo) as one packed word
__device__ __forceinline__ uint32_t nfk_f16_part_pair(float v0, float v1, int part) {
    const _Float16 h0 = (_Float16)v0, h1 = (_Float16)v1;
    const _Float16 r0 = part ? (_Float16)(v0 - (float)h0) : h0;
    const _Float16 r1 = part ? (_Float16)(v1 - (float)h1) : h1;
    return (uint32_t)__builtin_bit_cast(uint16_t, r0) | ((uint32_t)__builtin_bit_cast(uint16_t, r1) << 16);
}

// ---- row accessors: rows.val(t, r, k) = the unscaled weight of row r of tile
// t at contraction index k (0 outside the Linear), rows.bias(t, r) its bias.
// Layer-1 column maps: the input column of contraction index k, -1 past the inputs.
struct ColPlain {  // NSF_CL: the lower coordinates in lo_in order
    int n;
    __device__ int operator()(int k) const { return k < n ? k : -1; }
};
struct ColPerm {  // RealNVP: input coordinate of k-slot 32 kb + 8 q + j of a layer-1 B fragment
    int n;
    __device__ int operator()(int k) const {
        const int kb = k >> 5, q = (k >> 3) & 3, j = k & 7, c = 32 * kb + 16 * (j >> 2) + 4 * q + (j & 3);
        return c < n ? c : -1;
    }
};
struct ColTrig {  // NSF_AR conditioner i: canonical trig order k = 2j + {cos, sin} of cat(cos, sin) columns
    int i;
    __device__ int operator()(int k) const { return k < 2 * i ? (k & 1) * i + (k >> 1) : -1; }
};

// a hidden Linear [H][n_in] (+ bias [H]) through hid_feature; t1 = 2 (AR's
// 16-feature half tile 2 KBH): row r there is feature 32 KBH + r
template <class ColF>
struct HidRows {
    const float *W, *b;
    int H, n_in, kbh, t1;
    ColF col;
    __device__ int feature(int t, int r) const {
        return (t1 == 2 && t == 2 * kbh) ? 32 * kbh + r : hid_feature(t, r, kbh);
    }
    __device__ float val(int t, int r, int k) const {
        const int f = feature(t, r), c = col(k);
        return (f < H && c >= 0) ? W[(int64_t)f * n_in + c] : 0.0f;
    }
    __device__ float bias(int t, int r) const {
        const int f = feature(t, r);
        return f < H ? b[f] : 0.0f;
    }
};
// layer 2: Linear(H, H)
__device__ inline HidRows<ColPlain> hid_rows(const float* W, const float* b, int H, int kbh, int t1) {
    return HidRows<ColPlain>{W, b, H, H, kbh, t1, ColPlain{H}};
}

// output Linear: row 16 t + r of a tile = row r0 + 16 t + r of W [.][H], for the first n rows
struct OutRows {
    const float *W, *b;
    int64_t r0;
    int n, H;
    __device__ float val(int t, int r, int k) const {
        const int p = 16 * t + r;
        return (p < n && k < H) ? W[(r0 + p) * H + k] : 0.0f;
    }
    __device__ float bias(int t, int r) const {
        const int p = 16 * t + r;
        return p < n ? b[r0 + p] : 0.0f;
    }
};

// Word wl (0..255) of tail block g of the tiles [T0, ..) of an nt-tile record
// (the 16x16x16 f16 A fragments of tiles T0 + 2g and T0 + 2g + 1, interleaved
// per lane: words 4l, 4l + 1 the first, 4l + 2, 4l + 3 the second): lane l of
// tile t holds halves j = 0..3 = contraction indices kbase + j of row l & 15,
// as the hi part in k-groups 0 and 1, the lo part in k-group 2, zero in k-group 3.
template <class Rows>
__device__ uint32_t tail_word(int g, int wl, int nt, int T0, int kbase, float sc, const Rows& rows) {
    const int t = T0 + 2 * g + ((wl & 3) >> 1), lane = wl >> 2, j = 2 * (wl & 1), q = lane >> 4;
    if (t >= nt || q == 3) return 0u;
    return nfk_f16_part_pair(rows.val(t, lane & 15, kbase + j) * sc, rows.val(t, lane & 15, kbase + j + 1) * sc,
                             q == 2 ? 1 : 0);
}

// Word wl of block blk of a sub-record holding tiles [T0, T0 + ns) of an
// nt-tile record over a kbn-k-block contraction: the f16 blocks, then (t1 = 1)
// its tail blocks over contraction indices 32 kbn + 0..3 and the bias block
// [tile][row] of the sub-record's own tiles, pre-scaled by bsc; 0 in the
// padding behind.  A whole record is ns = nt, T0 = 0.  Block order and word
// layout are those gemm_h reads (nfk_fused_impl.h).
template <class Rows>
__device__ uint32_t record_word(int ns, int blk, int wl, int kbn, int t1, int nt, int T0, float sc, float bsc,
                                const Rows& rows) {
    const int nf = kbn * ns * 2, ntg = t1 == 1 ? (ns + 1) / 2 : 0;
    auto bias_word = [&]() {  // the sub-record's own tiles (gemm_h BREL)
        const int tt = wl >> 4, t = T0 + tt;
        return __float_as_uint(tt < ns && t < nt ? rows.bias(t, wl & 15) * bsc : 0.0f);
    };
    if (t1 == 2 && blk >= nf) {
        // 16-feature tail: the bias block first, then per tile {A1, A2}: lane l
        // (row l & 15, lane group g = l >> 4) element j of A1 = lo (j < 4) / hi
        // (j >= 4) weight of feature 32 kbn + 4 g + (j & 3), of A2 = hi (j < 4) / 0;
        // against B1 = {hi, lo} and B2 = {hi, 0} of the half tile's 4 rows
        if (blk == nf) return bias_word();
        const int tt = blk - nf - 1;
        if (tt >= 2 * ns) return 0u;
        const int t = T0 + (tt >> 1), which = tt & 1;
        if (t >= nt) return 0u;
        const int lane = wl >> 2, g = lane >> 4, row = lane & 15, jp = 2 * (wl & 3);
        _Float16 hv[2];
#pragma unroll
        for (int e = 0; e < 2; ++e) {
            const int j = jp + e;
            const float w = rows.val(t, row, 32 * kbn + 4 * g + (j & 3)) * sc;
            const _Float16 wh = (_Float16)w;
            if (which == 0)
                hv[e] = j < 4 ? (_Float16)(w - (float)wh) : wh;
            else
                hv[e] = j < 4 ? wh : (_Float16)0.0f;
        }
        return (uint32_t)__builtin_bit_cast(uint16_t, hv[0]) | ((uint32_t)__builtin_bit_cast(uint16_t, hv[1]) << 16);
    }
    if (blk < nf) {
        const int part = blk & 1, idx = blk >> 1, kb = idx / ns, t = T0 + (idx - kb * ns);
        if (t >= nt) return 0u;
        const int lane = wl >> 2, j = 2 * (wl & 3), k0 = 32 * kb + 8 * (lane >> 4) + j;
        return nfk_f16_part_pair(rows.val(t, lane & 15, k0) * sc, rows.val(t, lane & 15, k0 + 1) * sc, part);
    }
    if (blk < nf + ntg) return tail_word(blk - nf, wl, nt, T0, 32 * kbn, sc, rows);
    if (blk == nf + ntg) return bias_word();
    return 0u;  // padding to the slot's blocks
}

// ---- max|W| of a pack's Linears: grid-stride loop, wave butterfly, atomicMax
// of the bit patterns (non-negative floats order like their bit patterns, so
// the result is exact and order-independent); dst zeroed before the launch
__device__ inline void nfk_absmax(const float* w, int64_t n, unsigned int* dst) {
    float mx = 0.0f;
    for (int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; g < n; g += (int64_t)gridDim.x * blockDim.x)
        mx = fmaxf(mx, fabsf(w[g]));
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) mx = fmaxf(mx, __shfl_xor(mx, off, 64));
    if ((threadIdx.x & 63) == 0) atomicMax(dst, __float_as_uint(mx));
}
// the three Linears of one conditioner in one pass, into hdr[kHdrMax + 0..2]
__device__ inline void nfk_absmax3(const float* w1, int64_t n1, const float* w2, int64_t n2, const float* w3,
                                   int64_t n3, float* pack) {
    float m1 = 0.0f, m2 = 0.0f, m3 = 0.0f;
    for (int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; g < n1 + n2 + n3;
         g += (int64_t)gridDim.x * blockDim.x) {
        if (g < n1)
            m1 = fmaxf(m1, fabsf(w1[g]));
        else if (g < n1 + n2)
            m2 = fmaxf(m2, fabsf(w2[g - n1]));
        else
            m3 = fmaxf(m3, fabsf(w3[g - n1 - n2]));
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        m1 = fmaxf(m1, __shfl_xor(m1, off, 64));
        m2 = fmaxf(m2, __shfl_xor(m2, off, 64));
        m3 = fmaxf(m3, __shfl_xor(m3, off, 64));
    }
    if ((threadIdx.x & 63) == 0) {
        unsigned int* h = reinterpret_cast<unsigned int*>(pack) + kHdrMax;
        atomicMax(h, __float_as_uint(m1));
        atomicMax(h + 1, __float_as_uint(m2));
        atomicMax(h + 2, __float_as_uint(m3));
    }
}

// ---- the scales of a three-Linear pack, from the maxima in its header
struct PackScales {
    int s1, s2, s3;
    float sc1, sc2, sc3;  // weights: 2^s
    float bs1, bs2, bs3;  // biases: 2^(s+14); bs1 = 1 where the layer-1 bias stays unscaled (NSF)
};
__device__ inline PackScales pack_scales(const float* pack, bool l1_bias_unscaled) {
    const unsigned int* hdr = reinterpret_cast<const unsigned int*>(pack) + kHdrMax;
    PackScales p;
    p.s1 = nfk_scale_exp(__uint_as_float(hdr[0]));
    p.s2 = nfk_scale_exp(__uint_as_float(hdr[1]));
    p.s3 = nfk_scale_exp(__uint_as_float(hdr[2]));
    p.sc1 = ldexpf(1.0f, p.s1), p.sc2 = ldexpf(1.0f, p.s2), p.sc3 = ldexpf(1.0f, p.s3);
    p.bs1 = l1_bias_unscaled ? 1.0f : ldexpf(1.0f, p.s1 + 14);
    p.bs2 = ldexpf(1.0f, p.s2 + 14), p.bs3 = ldexpf(1.0f, p.s3 + 14);
    return p;
}

// header word g in [kHdrUnscale, kHdrWords) (words 0-2 hold the maxima): the
// unscale factors, init_param (AR; null otherwise), zeros
__device__ inline void write_header_word(uint32_t* out, int g, const PackScales& p, bool l1_bias_unscaled,
                                         const float* init = nullptr, int n_init = 0) {
    if (g == kHdrUnscale) out[g] = __float_as_uint(ldexpf(1.0f, l1_bias_unscaled ? -p.s1 : -(p.s1 + 14)));
    else if (g == kHdrUnscale + 1) out[g] = __float_as_uint(ldexpf(1.0f, -(p.s2 + 14)));
    else if (g == kHdrUnscale + 2) out[g] = __float_as_uint(ldexpf(1.0f, -(p.s3 + 14)));
    else if (g >= kHdrInit && g < kHdrInit + n_init) out[g] = __float_as_uint(init[g - kHdrInit]);
    else if (g > kHdrUnscale + 2 && g < kHdrWords) out[g] = 0u;
}

}  // namespace nfk_fused
