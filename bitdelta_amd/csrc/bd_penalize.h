// Repetition / presence / frequency penalties and a per-request logit bias: one row of 16-bit logits, the row's token history, four floats and a
// short bias list -> the penalised row in the logits' dtype.  include/bitdelta_hip.h (bd_srv_penalize_rows) is the definition;
// tests/penalty_ref.py restates it on CPU tensors.
//
// Elementwise, so unlike the sampling and log-probability kernels nothing is reduced over the row and a row is spread over SEVERAL blocks:
// grid = (ceil(V / 2048), rows), 256 threads, one aligned 8-vector per thread: a 16-byte load of logits, the matching 16 bytes of history, one
// 16-byte store.  The four parameters of the row are one 16-byte load at a block-uniform address.  V % 8 == 0, so a vector lies wholly inside
// the row or wholly outside; the last block of a row masks the vectors at or past V (they neither load nor store).
//
// The bias list (<= 64 pairs per row, list order matters: a repeated id is added twice, in that order) is found without V x nb comparisons and
// without LDS: lane j of EVERY wave loads pair j (the loads are issued next to the row's, from a few hundred bytes that stay in L2), one
// comparison per lane tells whether the id lies among the 512 elements of its wave, and a ballot gives the wave its hit list -- usually empty,
// and in list order because the set bits are taken from the lowest up.  Each hit is broadcast from its lane and added by the one lane that owns
// the element.  No barrier: a wave never waits for another.
//
// The step form counts: the thread that owns element tok[t] of an active tenant adds one to the element's count (saturating at 32767) before
// the penalties read it and stores the new history word with one 2-byte store; no other history element is written.  An inactive tenant's
// blocks leave before any load.  Every output element is a pure function of (l[v], hist[v], tok[t] == v, pen, bias list): no atomics, no
// dependence on thread or block order.  Each fp32 operation is rounded on its own (no contraction into an fma).
#pragma once
#include "bd_common.h"

namespace bd {

constexpr int PEN_BIAS_MAX = 64;           // BD_LOGIT_BIAS_MAX: one pair per lane of a wave
constexpr int PEN_BLOCK_ELEMS = 256 * 8;   // elements of a row per block

// STEP: bd_srv_step_penalize (tok / active read, hist counted and written); otherwise bd_srv_penalize_rows (every row live, hist read only).
template <int DT, bool STEP>
__global__ void __launch_bounds__(256) penalize_kernel(const unsigned short* __restrict__ logits, long long sl, int V,
                                                       unsigned short* __restrict__ out, long long so, unsigned short* __restrict__ hist,
                                                       long long sh, const long long* __restrict__ tok, const unsigned char* __restrict__ active,
                                                       const float* __restrict__ pen, const int* __restrict__ bias_id,
                                                       const float* __restrict__ bias_val, int nb) {
#pragma clang fp contract(off)                                          // every fp32 operation below is rounded on its own
    const int t = blockIdx.y;
    if (STEP && !active[t]) return;                                     // block-uniform: nothing of an inactive tenant is read or written
    const int lane = threadIdx.x & 63;
    const int c = (int)blockIdx.x * PEN_BLOCK_ELEMS + (int)threadIdx.x * 8;                  // this thread's elements: c .. c + 7
    const bool live = c < V;
    // ---- every load up front: the row's vectors, the parameters, this lane's pair of the bias list
    u32x4_t lv = {0u, 0u, 0u, 0u}, hv = {0u, 0u, 0u, 0u};
    if (live) {
        lv = *reinterpret_cast<const u32x4_t*>(logits + (long long)t * sl + c);
        hv = *reinterpret_cast<const u32x4_t*>(hist + (long long)t * sh + c);
    }
    const f32x4_t pv = *reinterpret_cast<const f32x4_t*>(pen + 4 * (long long)t);
    int bid = -1;
    float bval = 0.f;
    if (lane < nb) {
        bid = bias_id[(long long)t * nb + lane];
        bval = bias_val[(long long)t * nb + lane];
    }
    // ---- device values the host could not have written are neutralised
    const float r = pv[0], r_inv = pv[1];
    const bool rep = r > 0.f && r < __builtin_inff();                   // (a NaN fails both)
    const float presence = pv[2] == pv[2] ? pv[2] : 0.f, frequency = pv[3] == pv[3] ? pv[3] : 0.f;
    long long y = -1;
    if (STEP) y = tok[t];
    // the counted element, when this thread owns it (live: a token at or past V is in nobody's vector, so nothing is counted or stored for it)
    const int yi = (live && y >= c && y < (long long)c + 8) ? (int)(y - c) : -1;
    float x[8];
    uint32_t newh = 0u;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        const uint32_t h = (hv[e >> 1] >> (16 * (e & 1))) & 0xffffu;
        int cnt = (int)(h & 0x7fffu);
        bool seen = h != 0u;
        if (STEP && e == yi) {                                          // the token fed in this step: counted before the penalties read it
            cnt = cnt < 0x7fff ? cnt + 1 : 0x7fff;
            seen = true;
            newh = (h & 0x8000u) | (uint32_t)cnt;
        }
        float v = half_bits_to_f32<DT>((lv[e >> 1] >> (16 * (e & 1))) & 0xffffu);
        if (seen && rep) v = v > 0.f ? v * r_inv : v * r;
        const float fc = frequency * (float)cnt;                         // one product, one subtraction: two roundings
        v = v - fc;
        if (cnt > 0) v = v - presence;
        x[e] = v;
    }
    if (STEP && yi >= 0) hist[(long long)t * sh + c + yi] = (unsigned short)newh;            // the one history element this launch writes for t
    // ---- the bias list: this wave's hits in list order (the wave's 64 vectors are the elements w0 .. w0 + 511)
    const int w0 = c - lane * 8;
    const int wend = w0 + 512 < V ? w0 + 512 : V;
    unsigned long long hits = __ballot(bid >= w0 && bid < wend);        // wave-uniform; an id outside [0, V) matches no wave
    while (hits) {
        const int j = __ffsll((long long)hits) - 1;
        hits &= hits - 1;
        const int id = __shfl(bid, j, 64);
        const float b = __shfl(bval, j, 64);
        const int e = id - c;
#pragma unroll
        for (int k = 0; k < 8; ++k)
            if (e == k) x[k] = x[k] + b;
    }
    if (!live) return;
    u32x4_t ov;
#pragma unroll
    for (int e = 0; e < 4; ++e) ov[e] = f32_to_half_bits<DT>(x[2 * e]) | (f32_to_half_bits<DT>(x[2 * e + 1]) << 16);
    *reinterpret_cast<u32x4_t*>(out + (long long)t * so + c) = ov;
}

}  // namespace bd
