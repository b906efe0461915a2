// Tail truncation by the row's own statistics: one row of 16-bit logits, its temperature and (min_p, typical_p, epsilon_cutoff, eta_cutoff) ->
// the row with every dropped element set to -inf and every kept element's 16 bits unchanged.  include/bitdelta_hip.h (bd_srv_truncate_rows) is
// the definition; tests/truncation_ref.py restates it in fp64.
//
// One 256-thread block per row.  Up to V = 32768 the row is read from memory ONCE and lives in registers (bd_logprobs.h's lp_sweep); a longer
// row is swept from global memory once per pass.  Nothing is staged in LDS but the cross-wave partials and one 256-bin histogram; nothing spills.
// A row pays only for what it asks:
//   nothing set, a greedy temperature       the copy, no arithmetic
//   min_p alone                             the maximum and the mask pass: theta = ln min_p, no sums
//   epsilon                                 + Z, the sum of the masses (bd_serving.h's sample_mass: 2^-40 fixed point, an INTEGER sum)
//   eta or typical_p                        + mu = sum p x, as the integer sum of w (-x) in 2^-40 fixed point in the same pass
//   typical_p                               + the select on the key |x - mu|: four passes, one per byte of a 32-bit fixed-point key (most
//                                             significant first), each a mass histogram in LDS (integer atomics) and bd_serving.h's sample_select
// The three threshold filters are one bound theta on x = (l - m) / tau, formed once per row in fp64 from the integer sums.  No floating-point
// atomics anywhere: every sum that decides a threshold is an integer sum, so the kept set is a pure function of the row and the five numbers,
// whatever the order of threads, the row's index, the stride or the form (rows / step, registers / sweep).
//
// x of the row's maximum is exactly 0 and theta <= 0, so the maximum always passes the thresholds.  A FINITE element whose x is -inf in fp32
// -- (l - m) / tau overflows at a tiny tau, or l - m itself does on a bf16 row that spans more than FLT_MAX, where the fp64 restatement
// still holds a finite x -- is treated as what it is to any arithmetic of this width: mass 0 and the lowest select key (the largest
// distance), so every filter that is on drops it, as the restatement does (its mass there is far below 2^-40 too).  -inf elements take no
// part and stay -inf.  A row with a NaN or +inf, or without a finite element, is copied: the step end's greedy rule decides it.  Device values the host could not have written are neutralised: a parameter that
// is NaN or outside its open side is off (min_p <= 0, typical_p outside (0, 1), epsilon <= 0, eta <= 0), min_p >= 1 keeps the maximum only.
#pragma once
#include "bd_logprobs.h"

namespace bd {

struct TruncLds {
    float mx[4];
    int flag[4];
    unsigned long long z[4], sx[4];
};

// The select key of an element: its distance |x - mu| in 2^-27 fixed point, inverted, so that a SMALLER distance is a LARGER key and
// sample_select's "mass of the strictly larger keys" is the mass of the strictly more typical elements.  Fixed point, not the float's bits: an
// element that weighs anything has x >= -40 ln 2 (its mass is at least one 2^-40 word) and so has mu, hence a distance below 27.8 < 32 -- the
// key's top byte is floor(8 |x - mu|), which spreads a row over dozens of histogram bins where the float's exponent byte would put nearly all
// of it into three or four (LDS atomics to one address serialise).  2^-27 is finer than the fp32 rounding of x itself wherever |x| > 0.06.  A
// distance of 32 or more (mass 0, or x = -inf) gets the lowest key.
__device__ __forceinline__ uint32_t trunc_key(float x, float mu) { return ~(uint32_t)fminf(fabsf(x - mu) * 0x1p27f, 4294967040.f); }

// Between two passes over a register-resident row: the compiler must not carry a pass' per-element values (x, the masses, the keys: hundreds of
// registers at NV = 16) into the next pass instead of forming them again from the 16-bit row, which is what fits.
template <int NR>
__device__ __forceinline__ void trunc_forget(u32x4_t (&v)[NR]) {
#pragma unroll
    for (int j = 0; j < NR; ++j) asm volatile("" : "+v"(v[j]));
}

// active == nullptr: bd_srv_truncate_rows (R live rows); otherwise bd_srv_step_truncate (an inactive tenant's block leaves before any load).
// NV >= 1: the row's vectors tid + 256 j, j < NV, live in registers (V <= 2048 NV).  NV == 0: any V, every pass sweeps global memory; out must
// then not overlap logits (it never may).
template <int DT, int NV>
__global__ void __launch_bounds__(256) truncate_kernel(const unsigned short* __restrict__ logits, long long sl, int V,
                                                       unsigned short* __restrict__ out, long long so, const float* __restrict__ tau,
                                                       const float* __restrict__ params, const unsigned char* __restrict__ active) {
    __shared__ TruncLds s;
    __shared__ SampleLds h;
    const int t = blockIdx.x, tid = threadIdx.x;
    if (active != nullptr && !active[t]) return;                        // block-uniform: nothing of an inactive tenant is read or written
    const unsigned short* __restrict__ row = logits + (long long)t * sl;
    unsigned short* __restrict__ orow = out + (long long)t * so;
    const float ta = tau[t];
    const float mp = params[4 * (long long)t], ty = params[4 * (long long)t + 1], ep = params[4 * (long long)t + 2],
                et = params[4 * (long long)t + 3];
    const bool mp_on = mp > 0.f, ty_on = ty > 0.f && ty < 1.f, ep_on = ep > 0.f, et_on = et > 0.f;      // (a NaN compares false: off)
    const bool thr_on = mp_on || ep_on || et_on;
    const bool live = (thr_on || ty_on) && ta > 0.f && ta < __builtin_inff();
    constexpr int NR = NV > 0 ? NV : 1;
    u32x4_t v[NR] = {};                                                 // (NV == 0: never read, only handed on)
    if constexpr (NV > 0) {
#pragma unroll
        for (int j = 0; j < NV; ++j) {
            const int c = (tid + 256 * j) * 8;                          // V % 8 == 0: a vector is wholly inside the row or wholly outside
            if (c < V) v[j] = *reinterpret_cast<const u32x4_t*>(row + c);
            else v[j] = u32x4_t{NllNinf2<DT>::v, NllNinf2<DT>::v, NllNinf2<DT>::v, NllNinf2<DT>::v};
        }
    }
    const auto copy = [&]() { lp_sweep<NV>(v, row, V, [&](int c, u32x4_t w) { *reinterpret_cast<u32x4_t*>(orow + c) = w; }); };
    if (!live) { copy(); return; }                                      // nothing asked, or a greedy request
    // ---- the maximum, and whether the row holds a NaN or +inf
    float m = -__builtin_inff();
    int special = 0;
    lp_sweep<NV>(v, row, V, [&](int, u32x4_t w) {
#pragma unroll
        for (int d = 0; d < 4; ++d) {
            const float lo = half_bits_to_f32<DT>(w[d] & 0xffffu), hi = half_bits_to_f32<DT>(w[d] >> 16);
            special |= (!(lo < __builtin_inff())) | (!(hi < __builtin_inff()));
            m = fmaxf(m, fmaxf(lo, hi));
        }
    });
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        m = fmaxf(m, __shfl_xor(m, off, 64));
        special |= __shfl_xor(special, off, 64);
    }
    if ((tid & 63) == 0) { s.mx[tid >> 6] = m; s.flag[tid >> 6] = special; }
    __syncthreads();
    m = fmaxf(fmaxf(s.mx[0], s.mx[1]), fmaxf(s.mx[2], s.mx[3]));         // block-uniform
    special = s.flag[0] | s.flag[1] | s.flag[2] | s.flag[3] | !(m > -__builtin_inff());
    if (special) { copy(); return; }                                    // the step end's greedy rule decides such a row
    // ---- Z and mu: integer sums of 2^-40 fixed-point words
    const bool need_mu = et_on || ty_on, need_z = ep_on || need_mu;
    double ln_z = 0.0, mu = 0.0;
    if (need_z) {
        unsigned long long z = 0ull, sx = 0ull;
        trunc_forget(v);
        lp_sweep<NV>(v, row, V, [&](int, u32x4_t w) {
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                const float l = half_bits_to_f32<DT>((w[e >> 1] >> (16 * (e & 1))) & 0xffffu);
                z += sample_mass(l, m, ta);
                if (need_mu) {
                    const float x = (l - m) / ta, wt = __expf(x);
                    if (wt > 0.f) sx += (unsigned long long)(wt * -x * 0x1p40f);       // (x = -inf has wt = 0: no 0 * inf)
                }
            }
        });
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) {
            z += __shfl_xor(z, off, 64);
            sx += __shfl_xor(sx, off, 64);
        }
        if ((tid & 63) == 0) { s.z[tid >> 6] = z; s.sx[tid >> 6] = sx; }
        __syncthreads();
        const unsigned long long Z = (s.z[0] + s.z[1]) + (s.z[2] + s.z[3]), SX = (s.sx[0] + s.sx[1]) + (s.sx[2] + s.sx[3]);
        ln_z = log((double)Z * 0x1p-40);                                // Z >= 2^40: the maximum's own mass
        mu = -((double)SX / (double)Z);
    }
    // ---- the three thresholds as one bound on x (every thread forms the same fp64 value from the same integers)
    double theta = -(double)__builtin_inff();
    if (mp_on) theta = log((double)mp);
    if (ep_on) theta = fmax(theta, log((double)ep) + ln_z);
    if (et_on) {
        const double le = log((double)et), hh = ln_z - mu;             // ln min(eta, sqrt(eta) exp(-H)) = min(ln eta, ln eta / 2 - H)
        theta = fmax(theta, fmin(le, 0.5 * le - hh) + ln_z);
    }
    const float th = theta > 0.0 ? 0.f : (float)theta;
    // ---- typical_p: the key of the least typical kept element, one byte of the fixed-point key per pass
    const float muf = (float)mu;
    uint32_t kthr = 0u;
    if (ty_on) {
        unsigned long long above = 0ull, target = 0ull;
#pragma unroll
        for (int b = 3; b >= 0; --b) {
            h.hist[tid] = 0ull;
            __syncthreads();
            trunc_forget(v);
            lp_sweep<NV>(v, row, V, [&](int, u32x4_t w) {
#pragma unroll
                for (int e = 0; e < 8; ++e) {
                    const float l = half_bits_to_f32<DT>((w[e >> 1] >> (16 * (e & 1))) & 0xffffu);
                    const unsigned long long ms = sample_mass(l, m, ta);
                    if (ms == 0ull) continue;                           // (weighs nothing in any bin)
                    const uint32_t k = trunc_key((l - m) / ta, muf);
                    const uint32_t head = b == 3 ? 0u : k >> (b == 3 ? 0 : 8 * (b + 1));      // the bytes already decided (kthr so far)
                    if (head == kthr) atomicAdd(&h.hist[(k >> (8 * b)) & 0xffu], ms);
                }
            });
            __syncthreads();
            sample_select(h, above, target, b == 3 ? ty : 0.f);
            kthr = (kthr << 8) | (uint32_t)h.sel[0];
            above = h.sel[1];
            if (b == 3) target = h.sel[3];
        }
    }
    // ---- the kept set: the intersection; typical_p is ignored for a row on which it does not meet the thresholds' set
    bool use_ty = ty_on;
    if (ty_on && thr_on) {
        int any = 0;
        trunc_forget(v);
        lp_sweep<NV>(v, row, V, [&](int, u32x4_t w) {
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                const float l = half_bits_to_f32<DT>((w[e >> 1] >> (16 * (e & 1))) & 0xffffu);
                const float x = (l - m) / ta;
                any |= (l > -__builtin_inff() && x >= th && trunc_key(x, muf) >= kthr) ? 1 : 0;
            }
        });
        use_ty = __syncthreads_or(any) != 0;
    }
    trunc_forget(v);
    lp_sweep<NV>(v, row, V, [&](int c, u32x4_t w) {
        u32x4_t ov;
#pragma unroll
        for (int d = 0; d < 4; ++d) {
            uint32_t keep = 0u;
#pragma unroll
            for (int q = 0; q < 2; ++q) {
                const float x = (half_bits_to_f32<DT>((w[d] >> (16 * q)) & 0xffffu) - m) / ta;
                if (x >= th && (!use_ty || trunc_key(x, muf) >= kthr)) keep |= 0xffffu << (16 * q);
            }
            ov[d] = (w[d] & keep) | (NllNinf2<DT>::v & ~keep);
        }
        *reinterpret_cast<u32x4_t*>(orow + c) = ov;
    });
}

}  // namespace bd
