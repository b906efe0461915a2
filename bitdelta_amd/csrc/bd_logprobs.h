// Per-token log-probabilities and top-n alternatives: one row of 16-bit logits, a token and a count -> the token's log softmax and the top_n largest
// logits (ids and log softmax values).  include/bitdelta_hip.h (bd_srv_token_logprobs) is the definition; tests/logprobs_ref.py restates it in fp64.
//
// One 256-thread block per row.  It joins the two kernels before it: the maximum and the fixed-point sum are bd_token_nll.h's (nll_load8 /
// nll_max8 / nll_expsum8 per aligned 8-vector, integer sums in 2^-40 fixed point, ln S in fp64), so lp(y) is -nll of bd_srv_token_nll bit for
// bit; the top_n-th largest VALUE is found by bd_serving.h's exact radix select (sample_key, high byte then low byte inside the boundary bin,
// integer LDS counts, sample_select).  Up to V = 32768 the row lives in registers and is read from memory once; a longer row is swept from
// global memory once per pass (sample_sweep, four loads in flight).  The row is never staged in LDS and nothing spills.
//
// The list.  After the two histogram passes the block knows kthr, the key of the top_n-th largest element, `above` < top_n, the count of
// strictly larger keys, and cnt_b, the count of elements whose key IS kthr.  need = top_n - above of the boundary-valued elements belong to the
// list, the ones with the lowest indices.  cnt_b == need (no plateau straddles the boundary: the usual row): one pass gathers every key >= kthr
// into LDS slots handed out by an integer LDS counter -- any order, the sort below fixes it.  cnt_b > need: the pass gathers key > kthr only,
// and `need` block-wide minimum-index rounds (each: every thread's lowest boundary index above the last one taken, a shuffle + LDS integer
// minimum) append the plateau's first members; at most 20 rounds, each one pass over registers (or over the row, beyond 32768).  The <= 20
// candidates are then ranked by (key descending, index ascending) -- all distinct, so a candidate's rank is the count of candidates before it,
// and lane i writes its own entry to its rank.  Nothing depends on which thread came first: every count that decides a result is an integer.
//
// -inf has the lowest key of a row that passed the NaN / +inf check, so it enters the list only when fewer than top_n values are finite, in
// index order.  Columns at or past V are never counted (V % 8 == 0: a vector is wholly inside the row or wholly outside).
#pragma once
#include "bd_serving.h"
#include "bd_token_nll.h"

namespace bd {

constexpr int LP_TOP_MAX = 20;

struct LpLds {
    unsigned long long cand[LP_TOP_MAX];    // (0xffff - key) << 32 | index: ascending = the list's order
    int ncand;
    int rmin[2][4];                         // the minimum-index rounds' cross-wave partials, double-buffered: one barrier per round
};

// f(c, v) for every 16-byte vector v = row[c .. c + 7], c < V: from the registers (NV >= 1, vectors tid + 256 j) or from global memory (NV == 0)
template <int NV, int NR, class F>
__device__ __forceinline__ void lp_sweep(const u32x4_t (&v)[NR], const unsigned short* __restrict__ row, int V, F&& f) {
    if constexpr (NV > 0) {
#pragma unroll
        for (int j = 0; j < NV; ++j) {
            const int c = ((int)threadIdx.x + 256 * j) * 8;
            if (c < V) f(c, v[j]);
        }
    } else {
        sample_sweep(row, V, f);
    }
}

// One row.  All 256 threads of the block call it (it has barriers); row, V, y, top_n and the output pointers are block-uniform.
// lp: one float; top_id / top_lp: top_n entries each (not touched when top_n == 0).
template <int DT, int NV>
__device__ __forceinline__ void logprobs_row(const unsigned short* __restrict__ row, int V, long long y, int top_n, float* __restrict__ lp,
                                             int* __restrict__ top_id, float* __restrict__ top_lp) {
    __shared__ NllLds s;
    __shared__ SampleLds h;
    __shared__ LpLds q;
    const int tid = threadIdx.x;
    const bool in_range = y >= 0 && y < (long long)V;
    float ly = 0.f;
    if (tid == 0 && in_range) ly = half_bits_to_f32<DT>(row[y]);
    constexpr int NR = NV > 0 ? NV : 1;
    u32x4_t v[NR];
    if constexpr (NV > 0) {
#pragma unroll
        for (int j = 0; j < NV; ++j) v[j] = nll_load8<DT>(row, V, (tid + 256 * j) * 8);
    }
    // ---- the maximum (bd_srv_token_nll's m)
    float m = -__builtin_inff();
    lp_sweep<NV>(v, row, V, [&](int, u32x4_t w) { m = nll_max8<DT>(w, m); });
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) m = fmaxf(m, __shfl_xor(m, off, 64));
    if ((tid & 63) == 0) s.mx[tid >> 6] = m;
    if (tid == 0) q.ncand = 0;
    __syncthreads();
    m = fmaxf(fmaxf(s.mx[0], s.mx[1]), fmaxf(s.mx[2], s.mx[3]));                                  // block-uniform
    // ---- the sum (bd_srv_token_nll's S: per aligned 8-vector in fp32, integers from there on)
    const bool finite_max = m > -__builtin_inff() && m < __builtin_inff();
    unsigned long long acc = 0ull;
    int bad = 0;
    if (finite_max) {
        lp_sweep<NV>(v, row, V, [&](int, u32x4_t w) {
            const float e = nll_expsum8<DT>(w, m);
            bad |= e != e;
            acc += (unsigned long long)(e * 0x1p40f);
        });
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) {
            acc += __shfl_xor(acc, off, 64);
            bad |= __shfl_xor(bad, off, 64);
        }
        if ((tid & 63) == 0) { s.sum[tid >> 6] = acc; s.bad[tid >> 6] = bad; }
        __syncthreads();
    }
    const bool ok = finite_max && !(s.bad[0] | s.bad[1] | s.bad[2] | s.bad[3]);                    // block-uniform (s.bad is read only when written)
    if (!ok) {                                                          // a NaN, a +inf or nothing finite
        if (tid == 0) *lp = __builtin_nanf("");
        if (tid < top_n) { top_id[tid] = -1; top_lp[tid] = __builtin_nanf(""); }
        return;
    }
    double ln_s = 0.0;
    if (tid < 64) {                                                     // (wave 0 writes every result; one fp64 logarithm per lane, in lockstep)
        const unsigned long long S = (s.sum[0] + s.sum[1]) + (s.sum[2] + s.sum[3]);
        ln_s = log((double)S * 0x1p-40);
    }
    if (tid == 0) *lp = in_range ? (float)(((double)ly - (double)m) - ln_s) : __builtin_nanf("");
    if (top_n <= 0) return;
    // ---- the key of the top_n-th largest element: high byte, then low byte inside the boundary bin
    h.hist[tid] = 0;
    __syncthreads();
    lp_sweep<NV>(v, row, V, [&](int, u32x4_t w) {
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            atomicAdd(&h.hist[sample_key(w[e] & 0xffffu) >> 8], 1ull);
            atomicAdd(&h.hist[sample_key(w[e] >> 16) >> 8], 1ull);
        }
    });
    __syncthreads();
    sample_select(h, 0ull, (unsigned long long)top_n, 0.f);
    const uint32_t hb = (uint32_t)h.sel[0];
    const unsigned long long above_hb = h.sel[1];
    h.hist[tid] = 0;
    __syncthreads();
    lp_sweep<NV>(v, row, V, [&](int, u32x4_t w) {
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const uint32_t k0 = sample_key(w[e] & 0xffffu), k1 = sample_key(w[e] >> 16);
            if ((k0 >> 8) == hb) atomicAdd(&h.hist[k0 & 0xffu], 1ull);
            if ((k1 >> 8) == hb) atomicAdd(&h.hist[k1 & 0xffu], 1ull);
        }
    });
    __syncthreads();
    sample_select(h, above_hb, (unsigned long long)top_n, 0.f);
    const uint32_t kthr = (hb << 8) | (uint32_t)h.sel[0];
    const int above = (int)h.sel[1];                                    // keys > kthr: 0 .. top_n - 1
    const int need = top_n - above;                                     // boundary-valued members of the list: 1 .. top_n
    const bool plateau = h.hist[h.sel[0]] > (unsigned long long)need;   // more boundary-valued elements than places: the lowest indices win
    // ---- gather: every key above the boundary, and the boundary's own when all of them belong
    const uint32_t kmin = plateau ? kthr + 1u : kthr;
    lp_sweep<NV>(v, row, V, [&](int c, u32x4_t w) {
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const uint32_t k = sample_key((w[e >> 1] >> (16 * (e & 1))) & 0xffffu);
            if (k >= kmin) {
                const int slot = atomicAdd(&q.ncand, 1);
                if (slot < LP_TOP_MAX) q.cand[slot] = (unsigned long long)(0xffffu - k) << 32 | (unsigned)(c + e);
            }
        }
    });
    if (plateau) {
        int last = -1;
        for (int r = 0; r < need; ++r) {                                // block-uniform trip count
            int best = 0x7fffffff;
            lp_sweep<NV>(v, row, V, [&](int c, u32x4_t w) {
                if (c + 7 <= last || c >= best) return;
#pragma unroll
                for (int e = 7; e >= 0; --e) {
                    const uint32_t k = sample_key((w[e >> 1] >> (16 * (e & 1))) & 0xffffu);
                    if (k == kthr && c + e > last) best = c + e;        // (descending e: the vector's lowest index is kept)
                }
            });
#pragma unroll
            for (int off = 32; off >= 1; off >>= 1) { const int o = __shfl_xor(best, off, 64); best = o < best ? o : best; }
            if ((tid & 63) == 0) q.rmin[r & 1][tid >> 6] = best;
            __syncthreads();
            const int a = q.rmin[r & 1][0], b = q.rmin[r & 1][1], c2 = q.rmin[r & 1][2], d = q.rmin[r & 1][3];
            const int ab = a < b ? a : b, cd = c2 < d ? c2 : d;
            last = ab < cd ? ab : cd;                                   // block-uniform; always a real index: cnt_b > need of them exist
            if (tid == 0 && above + r < LP_TOP_MAX) q.cand[above + r] = (unsigned long long)(0xffffu - kthr) << 32 | (unsigned)last;
        }
    }
    __syncthreads();
    // ---- rank and write: lane i owns candidate i; its place is the count of candidates that sort before it
    if (tid < top_n) {
        const unsigned long long mine = q.cand[tid];
        int rank = 0;
        for (int j = 0; j < top_n; ++j) rank += q.cand[j] < mine ? 1 : 0;
        const uint32_t bits = sample_key_bits(0xffffu - (uint32_t)(mine >> 32));
        top_id[rank] = (int)(uint32_t)mine;
        top_lp[rank] = (float)(((double)half_bits_to_f32<DT>(bits) - (double)m) - ln_s);
    }
}

// R independent rows (n == nullptr): row r, token tok[r] -> lp[r], top_id / top_lp[r, 0 .. top_n).
// The step's form (n != nullptr), launched behind the step-end kernel: tenant t whose count n[t] moved past lp_n[t] has just emitted tok[t] at
// out[t, n[t] - 1]; its entry goes to [t, n[t] - 1] of the [T, cap(, top_n)] buffers and lp_n[t] follows n[t].  A tenant whose count did not move
// (inactive, or never admitted) leaves before reading its row.  Only the tenant's own block touches its entries and its counter.
template <int DT, int NV>
__global__ void __launch_bounds__(256) token_logprobs_kernel(const unsigned short* __restrict__ logits, long long sl, int V,
                                                             const long long* __restrict__ tok, const long long* __restrict__ n,
                                                             long long* __restrict__ lp_n, float* __restrict__ lp, int* __restrict__ top_id,
                                                             float* __restrict__ top_lp, int cap, int top_n) {
    const int r = blockIdx.x;
    long long e = r, n1 = 0;
    if (n) {
        n1 = n[r];
        if (n1 == lp_n[r]) return;                                      // uniform over the block: the counter is written behind barriers only
        const long long j = n1 - 1;
        if (j < 0 || j >= cap) {                                        // nothing to keep, but the counter follows
            __syncthreads();
            if (threadIdx.x == 0) lp_n[r] = n1;
            return;
        }
        e = (long long)r * cap + j;
    }
    logprobs_row<DT, NV>(logits + (long long)r * sl, V, tok[r], top_n, lp + e, top_id + e * top_n, top_lp + e * top_n);
    if (n && threadIdx.x == 0) lp_n[r] = n1;
}

}  // namespace bd
