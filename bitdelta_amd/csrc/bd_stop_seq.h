// A request stopped at a token SEQUENCE, and the number of trailing tokens that may still become one: behind the step end, per tenant, the last
// W tokens of this turn's output against the tenant's table of up to Q sequences of up to W ids.  include/bitdelta_hip.h
// (bd_srv_step_stop_sequences) is the definition; tests/stop_seq_ref.py restates it in plain Python.
//
// One block per tenant (grid = T): tenants share nothing, a tenant's block is the only one that touches its words (the step end's discipline),
// and every tenant's answer arrives after ONE tenant's latency -- a single block for all would walk T x Q x W pairs with at most 1024 threads.
// A block whose tenant emitted nothing in this step (n[t] == ss_n[t]) leaves after two loads at uniform addresses.
//
// The block has one thread per (sequence q, length k) pair: thread q * 32 + (k - 1), so Q * 32 threads rounded up to whole waves, 512 at the
// maximum, of which those with k > W idle (a fixed pitch of 32 keeps q and k a shift and a mask: a division by W would go through the
// floating-point reciprocal).  The window
// -- the last W tokens of out[t, 0:n], read through the row stride, 8 bytes each -- the table row and the lengths are each read ONCE from
// global memory, one element per thread, into LDS (2.2 KB at the maxima); a slot in front of the turn's first token, or a token that is no
// int32 >= 0, becomes -1 there and matches nothing.  Thread (q, k) then compares seq[q, 0:k] with the window's last k tokens out of LDS: the
// table word is the same for all k of a sequence (a broadcast), the window words of consecutive k lie in consecutive banks.  k == len_q makes
// the pair a HIT candidate, k < len_q a HOLD candidate; the lowest q and the largest k come from two butterfly reductions inside each wave
// and one pass of thread 0 over the at most 8 wave results.  No atomics, no floating point, no scratch, plain vector stores.
//
// Everything the kernel indexes with comes from device memory: n outside 0 .. out_cap compares nothing (hit -1, hold 0) and no element of
// `out` is addressed; a length outside 0 .. W counts as 0; a negative table entry matches nothing.
#pragma once
#include "bd_common.h"

namespace bd {

constexpr int SS_Q_MAX = 16;      // BD_STOP_SEQ_MAX
constexpr int SS_W_MAX = 32;      // BD_STOP_SEQ_LEN_MAX
constexpr int SS_T_MAX = 65535;

// (A template, so that it is emitted where the entry point asks for it, behind the kernels that existed: see the note above
// bd_srv_prefill_attention_cached in bd_api.hip.)
template <int MAX_Q, int MAX_W>
__global__ void __launch_bounds__(MAX_Q * MAX_W) stop_sequences_kernel(const long long* __restrict__ out, long long s_out, int out_cap,
                                                                       const long long* __restrict__ n, long long* __restrict__ ss_n,
                                                                       const int* __restrict__ seq_tok, const int* __restrict__ seq_len, int Q,
                                                                       int W, int* __restrict__ hit, int* __restrict__ hold,
                                                                       unsigned char* __restrict__ active, unsigned char* __restrict__ done) {
    __shared__ int win[MAX_W];                  // win[i] = y[n - W + i]: the window's LAST token is win[W - 1]
    __shared__ int tab[MAX_Q * MAX_W];
    __shared__ int len[MAX_Q];
    __shared__ int w_hit[MAX_Q * MAX_W / 64], w_hold[MAX_Q * MAX_W / 64];
    const int t = blockIdx.x, tid = threadIdx.x;
    const long long nt = n[t];
    if (nt == ss_n[t]) return;                                          // block-uniform: the tenant emitted nothing, nothing of it is touched
    const bool inside = nt >= 0 && nt <= (long long)out_cap;            // otherwise nothing can be compared
    const int ni = inside ? (int)nt : 0;
    if (tid < W) {
        const int j = ni - W + tid;                                     // index into the turn's tokens; j < ni <= out_cap
        int v = -1;
        if (j >= 0) {
            const long long y = out[(long long)t * s_out + j];
            if (y >= 0 && y <= 0x7fffffffll) v = (int)y;
        }
        win[tid] = v;
    }
    const int q = tid / MAX_W, c = tid % MAX_W;                         // (powers of two: a shift and a mask, no division by W)
    if (q < Q && c < W) tab[tid] = seq_tok[((long long)t * Q + q) * W + c];
    if (tid < Q) {
        const int l = seq_len[(long long)t * Q + tid];
        len[tid] = (l < 0 || l > W) ? 0 : l;
    }
    __syncthreads();                                                    // (every thread has read ss_n[t] by now: thread 0 writes it below)
    int my_hit = 0x7fffffff, my_hold = 0;
    if (q < Q) {
        const int k = c + 1, l = len[q];
        if (k <= l && k <= ni) {                                        // (l <= W, so the threads with c >= W stay out)
            bool same = true;
            for (int j = 0; j < k; ++j) {
                const int s = tab[q * MAX_W + j];
                same = same && s >= 0 && s == win[W - k + j];
            }
            if (same) {
                if (k == l) my_hit = q; else my_hold = k;
            }
        }
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        const int oh = __shfl_xor(my_hit, off, 64), ok = __shfl_xor(my_hold, off, 64);
        my_hit = oh < my_hit ? oh : my_hit;
        my_hold = ok > my_hold ? ok : my_hold;
    }
    if ((tid & 63) == 0) { w_hit[tid >> 6] = my_hit; w_hold[tid >> 6] = my_hold; }
    __syncthreads();
    if (tid == 0) {
        const int waves = ((int)blockDim.x + 63) >> 6;
        for (int w = 1; w < waves; ++w) {
            my_hit = w_hit[w] < my_hit ? w_hit[w] : my_hit;
            my_hold = w_hold[w] > my_hold ? w_hold[w] : my_hold;
        }
        const bool is_hit = my_hit != 0x7fffffff;
        ss_n[t] = nt;
        hit[t] = is_hit ? my_hit : -1;
        hold[t] = is_hit ? 0 : my_hold;
        if (is_hit) {
            active[t] = 0;
            done[t] = (unsigned char)(done[t] | 16);
        }
    }
}

}  // namespace bd
