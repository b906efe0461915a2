// Scoring tail (eval_ppl.py's loss, per tenant): one row of 16-bit logits and a label -> -log softmax(row)[label] and the row's log-sum-exp.
// include/bitdelta_hip.h (bd_srv_token_nll) is the definition; tests/nll_ref.py restates it in fp64.
//
// Bandwidth-bound: thousands of independent 64 KB rows, 4 (+4) bytes out per row.  One 256-thread block per row.  Up to V = 32768 the block
// holds its WHOLE row in registers (NV <= 16 sixteen-byte loads per thread, all issued before the first use), so the maximum, the sum and the
// label cost one trip to memory; a longer row is read twice (maximum, then sum), four loads in flight.  The row is never staged in LDS
// (64 bytes of LDS hold the cross-wave partials) and nothing spills.
//
// Arithmetic, and why a value is a pure function of (row, label):
//   m        = the row's maximum (fmax: exact, order-free);
//   per 16-byte vector: e_i = exp2((l_i - m) * log2 e) (v_exp_f32), the eight e_i summed pairwise in fp32 IN A FIXED ORDER inside one thread,
//              the vector's sum truncated to 2^-40 fixed point (<= 2^43);
//   S        = the INTEGER sum of those words over the thread, the wave and the block (order-free; < 2^63 for V <= 2^22);
//   ln S     = log(double(S) * 2^-40) in fp64 on one thread; lse = float(m + ln S); nll = float(ln S + (m - l_label)), both sums in fp64.
// Which vector an element belongs to is fixed by its column alone (vectors start at multiples of 8), so neither R, the row's index, the stride,
// the neighbours nor the kernel form (NV) can move a bit.  Error of ln S: each e_i carries <= 2^-24 (|l_i - m| + 3) relative (the product's
// rounding scales with the exponent; v_exp_f32 ~1 ulp), the pairwise sum 3 * 2^-24, the truncation V/8 * 2^-40 absolute against S >= 1.  Weighted
// by the softmax, sum_i p_i (m - l_i) = H(p) - ln S <= ln V, so |d ln S| <= 2^-24 (ln V + 6) + V * 2^-43: 1.0e-6 at V = 32000, 1.4e-6 at 2^22,
// inside the 2^-19 the tests allow before the result's own fp32 rounding (2^-24 relative).  (m - l_label) is formed in fp64: exact for fp16, to 2^-53 for bf16.
// A NaN reaches S through l - m, the product, v_exp_f32 and the adds (IEEE propagation; no fast-math) and is caught per vector as sum != sum;
// +inf makes m = +inf, nothing finite makes m = -inf; each of the three gives NaN.  -inf next to a finite m is exp2(-inf) = 0.
#pragma once
#include "bd_common.h"

namespace bd {

constexpr int NLL_NV_MAX = 16;                      // register-resident form: V <= 256 threads * 8 * NLL_NV_MAX = 32768
constexpr int NLL_V_MAX = 1 << 22;                  // V * 2^40 (every mass 1.0) + 2^43 must stay below 2^63

template <int DT> struct NllNinf2 { static constexpr uint32_t v = DT == DT_BF16 ? 0xff80ff80u : 0xfc00fc00u; };   // -inf in both halves

// row[c .. c + 7] with every element at or past V replaced by -inf (weight 0, never the maximum of a row that has a finite value, no NaN).  The
// load itself always lies inside the row's stride: c < V rounds up to at most sl (sl % 8 == 0, sl >= V); a vector wholly past V re-reads vector 0.
template <int DT>
__device__ __forceinline__ u32x4_t nll_load8(const unsigned short* __restrict__ row, int V, int c) {
    u32x4_t v = *(const u32x4_t*)(row + (c < V ? c : 0));
    if (c + 8 > V) {
#pragma unroll
        for (int d = 0; d < 4; ++d) {
            const uint32_t keep = (c + 2 * d < V ? 0xffffu : 0u) | (c + 2 * d + 1 < V ? 0xffff0000u : 0u);
            v[d] = (v[d] & keep) | (NllNinf2<DT>::v & ~keep);
        }
    }
    return v;
}

template <int DT> __device__ __forceinline__ float nll_max8(u32x4_t v, float m) {
#pragma unroll
    for (int d = 0; d < 4; ++d) m = fmaxf(m, fmaxf(half_bits_to_f32<DT>(v[d] & 0xffffu), half_bits_to_f32<DT>(v[d] >> 16)));
    return m;
}

// sum_i exp(l_i - m) of one vector: pairwise, fixed order
template <int DT> __device__ __forceinline__ float nll_expsum8(u32x4_t v, float m) {
    float p[4];
#pragma unroll
    for (int d = 0; d < 4; ++d) {
        const float a = __builtin_amdgcn_exp2f((half_bits_to_f32<DT>(v[d] & 0xffffu) - m) * 1.44269504f);
        const float b = __builtin_amdgcn_exp2f((half_bits_to_f32<DT>(v[d] >> 16) - m) * 1.44269504f);
        p[d] = a + b;
    }
    return (p[0] + p[1]) + (p[2] + p[3]);
}

struct NllLds {
    float mx[4];
    unsigned long long sum[4];
    int bad[4];
};

// NV >= 1: the row's vectors tid + 256 j, j < NV, live in registers (V <= 2048 NV).  NV == 0: any V, two passes over global memory.
template <int DT, int NV>
__global__ void __launch_bounds__(256) token_nll_kernel(const unsigned short* __restrict__ logits, long long sl, int V,
                                                        const long long* __restrict__ labels, float* __restrict__ nll, float* __restrict__ lse) {
    __shared__ NllLds s;
    const int tid = threadIdx.x, r = blockIdx.x;
    const unsigned short* __restrict__ row = logits + (long long)r * sl;
    const long long y = labels[r];
    const bool scored = y >= 0 && y < (long long)V;
    float ly = 0.f;
    if (tid == 0 && scored) ly = half_bits_to_f32<DT>(row[y]);
    constexpr int NR = NV > 0 ? NV : 1;
    u32x4_t v[NR];
    // ---- the maximum
    float m = -__builtin_inff();
    if constexpr (NV > 0) {
#pragma unroll
        for (int j = 0; j < NV; ++j) v[j] = nll_load8<DT>(row, V, (tid + 256 * j) * 8);
#pragma unroll
        for (int j = 0; j < NV; ++j) m = nll_max8<DT>(v[j], m);
    } else {
        for (long long c = tid * 8; c < V; c += 4 * 2048) {
            u32x4_t w[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) w[j] = nll_load8<DT>(row, V, (int)(c + 2048 * j < V ? c + 2048 * j : V));   // past the row: all -inf
#pragma unroll
            for (int j = 0; j < 4; ++j) m = nll_max8<DT>(w[j], m);
        }
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) m = fmaxf(m, __shfl_xor(m, off, 64));
    if ((tid & 63) == 0) s.mx[tid >> 6] = m;
    __syncthreads();
    m = fmaxf(fmaxf(s.mx[0], s.mx[1]), fmaxf(s.mx[2], s.mx[3]));                                  // block-uniform
    // ---- the sum (skipped, block-uniformly, when the maximum already says NaN)
    const bool finite_max = m > -__builtin_inff() && m < __builtin_inff();
    unsigned long long acc = 0ull;
    int bad = 0;
    if (finite_max) {
        if constexpr (NV > 0) {
#pragma unroll
            for (int j = 0; j < NV; ++j) {
                const float e = nll_expsum8<DT>(v[j], m);
                bad |= e != e;
                acc += (unsigned long long)(e * 0x1p40f);
            }
        } else {
            for (long long c = tid * 8; c < V; c += 4 * 2048) {
                u32x4_t w[4];
#pragma unroll
                for (int j = 0; j < 4; ++j) w[j] = nll_load8<DT>(row, V, (int)(c + 2048 * j < V ? c + 2048 * j : V));
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const float e = nll_expsum8<DT>(w[j], m);
                    bad |= e != e;
                    acc += (unsigned long long)(e * 0x1p40f);
                }
            }
        }
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) {
            acc += __shfl_xor(acc, off, 64);
            bad |= __shfl_xor(bad, off, 64);
        }
        if ((tid & 63) == 0) { s.sum[tid >> 6] = acc; s.bad[tid >> 6] = bad; }
        __syncthreads();
    }
    if (tid == 0) {
        float out_lse = __builtin_nanf(""), out_nll = __builtin_nanf("");
        if (finite_max && !(s.bad[0] | s.bad[1] | s.bad[2] | s.bad[3])) {
            const unsigned long long S = (s.sum[0] + s.sum[1]) + (s.sum[2] + s.sum[3]);
            const double ln_s = log((double)S * 0x1p-40);
            out_lse = (float)((double)m + ln_s);
            out_nll = (float)(ln_s + ((double)m - (double)ly));                                   // a label on -inf: +inf
        }
        nll[r] = scored ? out_nll : 0.f;
        if (lse) lse[r] = out_lse;
    }
}

}  // namespace bd
