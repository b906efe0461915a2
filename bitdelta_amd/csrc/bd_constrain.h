// A request's output restricted to a token automaton: one row of 16-bit logits, the row's automaton state, the state's sorted edge tokens, its
// accepting byte and the request's stop ids -> the row with every token the state does not allow set to -inf, and the transition that follows
// the chosen token.  include/bitdelta_hip.h (bd_srv_constrain_rows, bd_srv_step_constrain_advance) is the definition;
// tests/constraint_ref.py restates it in plain Python.
//
// The mask is elementwise, so -- like the penalty kernel -- a row is spread over SEVERAL blocks: grid = (ceil(V / 2048), rows), 256 threads, one
// aligned 8-vector per thread: one 16-byte load of logits, one 16-byte store.  V % 8 == 0, so a vector lies wholly inside the row or wholly
// outside; threads at or past V leave at once (nothing below crosses lanes, and there is no barrier).  No float is ever made of a logit: a kept
// element is the loaded 16 bits, a masked one the dtype's -inf pattern.
//
// Membership costs no V x E comparisons: state[r], off[state] and off[state + 1] are block-uniform (loads at uniform addresses, which the
// compiler issues as scalar loads), then each thread finds the lower bound of its first index c in the state's sorted slice -- log2(edges)
// dependent 4-byte loads out of a few KB that stay in L2 -- and compares the at most 8 entries from there against c .. c + 7.  Those 8 loads
// are unconditional (the index is clamped to the slice's last entry, which sets a bit twice at worst), so they are issued together.  The stop
// ids, read only in an accepting state, are at most 64 loads at uniform addresses and one comparison each.
//
// Everything the kernel indexes with comes from device memory, so everything is clamped: a state outside [0, S) masks nothing, slice bounds are
// clamped into [0, E], an edge token outside [c, c + 8) -- negative or >= V included -- sets no bit.  The mask launch only READS the state:
// several blocks share a row.  The state moves in a launch of its own behind the step end (constrain_advance_kernel: one thread per tenant,
// bd_srv_step_logprobs' counter discipline).
#pragma once
#include "bd_common.h"

namespace bd {

constexpr int CON_BLOCK_ELEMS = 256 * 8;   // elements of a row per block
constexpr int CON_STATES_MAX = 1 << 16;    // BD_CONSTRAINT_STATES_MAX
constexpr int CON_EDGES_MAX = 1 << 20;     // BD_CONSTRAINT_EDGES_MAX
constexpr int CON_STOP_MAX = 64;           // BD_CONSTRAINT_STOP_MAX
constexpr int CON_ADVANCE_T_MAX = 1024;    // one block, one thread per tenant

template <int DT> struct NegInf2 { static constexpr uint32_t v = (DT == DT_BF16) ? 0xFF80FF80u : 0xFC00FC00u; };   // -inf in both halves

// the edge slice [b, e) of state s, 0 <= s < S, clamped into [0, E] (off is device data)
__device__ __forceinline__ void con_slice(const int* __restrict__ off_row, int s, int E, int& b, int& e) {
    b = off_row[s];
    e = off_row[s + 1];
    b = b < 0 ? 0 : (b > E ? E : b);
    e = e < b ? b : (e > E ? E : e);
}

// the first index in [b, e) whose token is >= key (e when there is none)
__device__ __forceinline__ int con_lower_bound(const int* __restrict__ et, int b, int e, int key) {
    while (b < e) {
        const int m = b + ((e - b) >> 1);
        if (et[m] < key) b = m + 1; else e = m;
    }
    return b;
}

// STEP: bd_srv_step_constrain (active read; an inactive tenant's blocks leave before any load); otherwise bd_srv_constrain_rows.
template <int DT, bool STEP>
__global__ void __launch_bounds__(256) constrain_kernel(const unsigned short* __restrict__ logits, long long sl, int V,
                                                        unsigned short* __restrict__ out, long long so, const int* __restrict__ state,
                                                        const int* __restrict__ off, const int* __restrict__ edge_tok,
                                                        const unsigned char* __restrict__ accepting, int S, int E,
                                                        const long long* __restrict__ stop_ids, int ns, const unsigned char* __restrict__ active) {
    const int t = blockIdx.y;
    if (STEP && !active[t]) return;                                     // block-uniform: nothing of an inactive tenant is read or written
    const int c = (int)blockIdx.x * CON_BLOCK_ELEMS + (int)threadIdx.x * 8;                  // this thread's elements: c .. c + 7
    if (c >= V) return;
    const u32x4_t lv = *reinterpret_cast<const u32x4_t*>(logits + (long long)t * sl + c);
    const int s = state[t];                                             // block-uniform, like everything derived from it up to the search
    uint32_t keep = 0xffu;                                              // bit k: element c + k keeps its bits
    if (s >= 0 && s < S) {
        keep = 0u;
        int b, e;
        con_slice(off + (long long)t * (S + 1), s, E, b, e);
        if (b < e) {
            const int* __restrict__ et = edge_tok + (long long)t * E;
            const int lo = con_lower_bound(et, b, e, c);
            int tk[8];
#pragma unroll
            for (int k = 0; k < 8; ++k) tk[k] = et[lo + k < e ? lo + k : e - 1];             // unconditional: all eight in flight together
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                const uint32_t d = (uint32_t)tk[k] - (uint32_t)c;      // < 8 exactly for a token in c .. c + 7 (c + 8 <= V <= 2^22)
                if (d < 8u) keep |= 1u << d;
            }
        }
        if (accepting[(long long)t * S + s]) {
            for (int j = 0; j < ns; ++j) {
                const unsigned long long d = (unsigned long long)stop_ids[(long long)t * ns + j] - (unsigned long long)c;   // (-1: an empty slot)
                if (d < 8ull) keep |= 1u << (uint32_t)d;
            }
        }
    }
    u32x4_t ov;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const uint32_t m = ((keep >> (2 * q)) & 1u ? 0x0000ffffu : 0u) | ((keep >> (2 * q + 1)) & 1u ? 0xffff0000u : 0u);
        ov[q] = (lv[q] & m) | (NegInf2<DT>::v & ~m);
    }
    *reinterpret_cast<u32x4_t*>(out + (long long)t * so + c) = ov;
}

// bd_srv_step_constrain_advance: thread t follows tenant t's token of this step.  Integer work, total on any device values.  (A template, so that
// it is emitted where the entry point asks for it, behind the kernels that existed -- a plain __global__ function is emitted where the header is
// included, and every kernel behind it moves: see the note above bd_srv_prefill_attention_cached in bd_api.hip.)
template <int MAX_T>
__global__ void __launch_bounds__(MAX_T) constrain_advance_kernel(const long long* __restrict__ tok, const long long* __restrict__ n,
                                                                  long long* __restrict__ c_n, int* __restrict__ state,
                                                                  const int* __restrict__ off, const int* __restrict__ edge_tok,
                                                                  const int* __restrict__ edge_next,
                                                                  const unsigned char* __restrict__ accepting, int S, int E,
                                                                  unsigned char* __restrict__ active, unsigned char* __restrict__ done, int T) {
    const int t = threadIdx.x;
    if (t >= T) return;
    const long long nt = n[t];
    if (nt == c_n[t]) return;                                           // the tenant emitted nothing in this step: nothing of it is touched
    c_n[t] = nt;
    int s = state[t];
    if (s < 0 || s >= S) return;                                        // no constraint (or a value the host could not have written)
    const int* __restrict__ o = off + (long long)t * (S + 1);
    int b, e;
    con_slice(o, s, E, b, e);
    const long long y = tok[t];
    if (b < e && y >= 0 && y <= 0x7fffffffll) {
        const int* __restrict__ et = edge_tok + (long long)t * E;
        const int i = con_lower_bound(et, b, e, (int)y);
        if (i < e && et[i] == (int)y) {
            const int nx = edge_next[(long long)t * E + i];
            if (nx >= 0 && nx < S) {
                s = nx;
                state[t] = s;
            }
        }
    }
    con_slice(o, s, E, b, e);
    if (b == e && accepting[(long long)t * S + s] && active[t]) {       // a final state: the constraint is complete
        active[t] = 0;
        done[t] |= 8;
    }
}

}  // namespace bd
