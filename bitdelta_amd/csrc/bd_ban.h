// Hard bans that depend on what a request has already written: one row of 16-bit logits, the row's history (the conversation's real tokens,
// then this turn's emitted tokens), its no-repeat n-gram size, its bad-word table, its minimum turn length and its stop ids -> the row with
// every banned token set to -inf and every other element's 16 bits kept.  include/bitdelta_hip.h (bd_srv_ban_rows) is the definition;
// tests/ban_ref.py restates it in plain Python.
//
// The mask is elementwise, so -- like the penalty and constraint kernels -- a row is spread over SEVERAL blocks: grid = (ceil(V / 2048), rows),
// 256 threads, one aligned 8-vector per thread: one 16-byte load of logits, one 16-byte store.  What is banned is NOT elementwise: it is found
// by one pass over the row's own history.  Every block makes that pass itself -- at most Lc + out_cap integers that stay in L2 -- and keeps
// only the bans that fall into its own 2048-element slice, as bits of a 256-byte LDS bitmap (LDS atomic OR).  That costs redundant reads and
// removes every dependency between blocks: no global atomic, no two blocks write one address, one barrier pair inside the block.
//   n-gram    the tail of g - 1 tokens is staged once in LDS; threads stride over the start i of a candidate and compare the LAST tail token
//             first, so nearly every candidate is rejected after one load
//   bad words one thread per table row, the last context token first
//   early stop one thread per stop id
// No float is ever made of a logit: a kept element is the loaded 16 bits, a banned one the dtype's -inf pattern.
//
// Everything the kernel indexes with comes from device memory, so everything is clamped: ctx_len into [0, Lc], n into [0, out_cap], a g outside
// 0 .. 8 is off, a length outside 0 .. W is an empty slot, a banned id outside [0, V) sets no bit.  History elements are compared as 64-bit
// integers (ctx is widened), so an element of `out` that is no int32 simply equals nothing a table or ctx can hold.
#pragma once
#include "bd_common.h"
#include "bd_constrain.h"

namespace bd {

constexpr int BAN_BLOCK_ELEMS = 256 * 8;   // elements of a row per block
constexpr int BAN_NGRAM_MAX = 8;           // BD_BAN_NGRAM_MAX
constexpr int BAN_WORDS_MAX = 64;          // BD_BAN_WORDS_MAX
constexpr int BAN_WORD_LEN_MAX = 32;       // BD_BAN_WORD_LEN_MAX
constexpr int BAN_STOP_MAX = 64;           // BD_BAN_STOP_MAX

// history element i of a row, 0 <= i < cl + nn: ctx below cl, then the turn's tokens through their own row
__device__ __forceinline__ long long ban_hist(const int* __restrict__ ctx_row, const long long* __restrict__ tok_row, int cl, int i) {
    return i < cl ? (long long)ctx_row[i] : tok_row[i - cl];
}

// token y is banned: its bit in this block's slice [base, base + 2048), when it lies there and below V
__device__ __forceinline__ void ban_set(uint32_t* bm, long long y, int base, int V) {
    const long long d = y - (long long)base;
    if (d >= 0 && d < (long long)BAN_BLOCK_ELEMS && y < (long long)V) atomicOr(&bm[(int)d >> 5], 1u << ((int)d & 31));
}

// STEP: bd_srv_step_ban (active read; an inactive tenant's blocks leave before any load); otherwise bd_srv_ban_rows.  n == NULL: no turn
// tokens yet (admission), toks is then not read.
template <int DT, bool STEP>
__global__ void __launch_bounds__(256) ban_kernel(const unsigned short* __restrict__ logits, long long sl, int V, unsigned short* __restrict__ out,
                                                  long long so, const int* __restrict__ ctx, int Lc, const int* __restrict__ ctx_len,
                                                  const long long* __restrict__ toks, long long s_tok, int tok_cap,
                                                  const long long* __restrict__ n, const int* __restrict__ ban_ngram,
                                                  const int* __restrict__ ban_tok, const int* __restrict__ ban_len, int Q, int W,
                                                  const int* __restrict__ ban_min, const long long* __restrict__ stop_ids, int ns,
                                                  const unsigned char* __restrict__ active) {
    __shared__ uint32_t bm[BAN_BLOCK_ELEMS / 32];
    __shared__ long long tail[BAN_NGRAM_MAX];
    const int t = blockIdx.y;
    if (STEP && !active[t]) return;                                     // block-uniform: nothing of an inactive tenant is read or written
    const int tid = threadIdx.x;
    const int base = (int)blockIdx.x * BAN_BLOCK_ELEMS;
    // block-uniform scalars, clamped
    int cl = ctx_len[t];
    cl = cl < 0 ? 0 : (cl > Lc ? Lc : cl);
    int nn = 0;
    if (n != nullptr) {
        const long long nv = n[t];
        nn = nv < 0 ? 0 : (nv > (long long)tok_cap ? tok_cap : (int)nv);
    }
    const int m = cl + nn;                                              // the history's length (Lc + out_cap < 2^31: checked on the host)
    int g = ban_ngram[t];
    if (g < 1 || g > BAN_NGRAM_MAX) g = 0;
    const int* __restrict__ ctx_row = ctx + (long long)t * Lc;
    const long long* __restrict__ tok_row = toks + (long long)t * s_tok;
    if (tid < BAN_BLOCK_ELEMS / 32) bm[tid] = 0u;
    if (g > 1 && m >= g - 1 && tid < g - 1) tail[tid] = ban_hist(ctx_row, tok_row, cl, m - g + 1 + tid);
    __syncthreads();
    // 1. no-repeat n-gram: every earlier occurrence of the last g - 1 tokens bans the token that followed it
    if (g >= 1 && m >= g - 1) {
        for (int i = tid; i <= m - g; i += 256) {
            bool same = true;
            for (int k = g - 2; k >= 0 && same; --k) same = ban_hist(ctx_row, tok_row, cl, i + k) == tail[k];
            if (same) ban_set(bm, ban_hist(ctx_row, tok_row, cl, i + g - 1), base, V);
        }
    }
    // 2. bad words: a sequence whose first L - 1 tokens end the history bans its last token (L == 1: always)
    for (int q = tid; q < Q; q += 256) {
        const int L = ban_len[(long long)t * Q + q];
        if (L < 1 || L > W || m < L - 1) continue;
        const int* __restrict__ w = ban_tok + ((long long)t * Q + q) * W;
        bool same = true;
        for (int j = L - 2; j >= 0 && same; --j) same = ban_hist(ctx_row, tok_row, cl, m - L + 1 + j) == (long long)w[j];
        if (same) ban_set(bm, (long long)w[L - 1], base, V);
    }
    // 3. early stop: the turn is shorter than its minimum, so no stop id may be chosen
    if (nn < ban_min[t]) {
        for (int j = tid; j < ns; j += 256) ban_set(bm, stop_ids[(long long)t * ns + j], base, V);       // (-1: an empty slot)
    }
    __syncthreads();
    const int c = base + tid * 8;                                       // this thread's elements: c .. c + 7
    if (c >= V) return;
    const u32x4_t lv = *reinterpret_cast<const u32x4_t*>(logits + (long long)t * sl + c);
    const uint32_t banned = (bm[tid >> 2] >> ((tid & 3) * 8)) & 0xffu;  // bit k: element c + k is banned
    u32x4_t ov;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const uint32_t keep = ((banned >> (2 * q)) & 1u ? 0u : 0x0000ffffu) | ((banned >> (2 * q + 1)) & 1u ? 0u : 0xffff0000u);
        ov[q] = (lv[q] & keep) | (NegInf2<DT>::v & ~keep);
    }
    *reinterpret_cast<u32x4_t*>(out + (long long)t * so + c) = ov;
}

}  // namespace bd
