// The KV cache in OCP e4m3 (one byte per element): decode attention, the prefill's append, and the expansion `extend` reads.
// include/bitdelta_hip.h (bd_srv_decode_attention_kv8) is the definition: byte = e4m3_rne(clamp(float(x) * inv_scale, -448, 448)), value =
// float(byte) * scale, one fp32 scale (and its host-computed reciprocal) per (tenant, kv head).  gfx950 converts in hardware, two elements per
// instruction: v_cvt_pk_f32_fp8 (exact) and v_cvt_pk_fp8_f32 (round to nearest even).
//
//   decode_attn_kv8_kernel      RoPE(q, k_new) -> quantise k_new / v_new -> append -> softmax(q.K^T / sqrt(d)) . V over the BYTES, new token included
//   rope_kv_append_kv8_kernel   rope_kv_append_kernel with both cache writes quantised (qkv itself stays 16-bit for the whole-prompt attention)
//   kv8_expand_kernel           rows [r0, r1) of one layer's byte caches -> round16(float(byte) * scale) in a 16-bit scratch
//
// Geometry of the decode kernel, and why:
//   * a cache row is 128 bytes = ONE cache line.  Lane (kq = l >> 4, d8 = l & 15) reads 8 bytes = dims 8*d8 .. +7 of row l0 + kq: 16 lanes per
//     row, 4 rows per wave instruction, 32 rows per block iteration -- the row walk, the split bounds (whole iterations of 32 rows) and the DPP
//     row sum of the 16-bit kernel carry over, so a position has the same owner split in both kernels.  16 dims per lane (16-byte loads, 8 rows
//     per wave instruction) would need 16 * G query floats + 16 * G accumulators per lane: 256 VGPRs at G = 8, the whole budget of a 512-thread
//     block, and the row sum would cross DPP rows.  8-byte loads keep G = 8 at the 16-bit kernel's register count.
//   * a wave instruction moves 512 bytes, not 1024, so the ring is TWICE as deep in iterations for the same bytes in flight: DEPTH 4 up to 2048
//     cache rows, 8 beyond (16-bit: 2 / 4).  A slot is 2 + 2 data registers instead of 4 + 4: the deeper ring costs no register.
//   * score and PV work stays on the VALU for every G: 8 * G query floats and accumulators per lane as before; the conversion is cheaper than
//     the 16-bit kernel's (one v_cvt_pk_f32_fp8 per TWO elements).  A 16x16x32 MFMA form for G = 4 / 8 would pad G to 16 query rows and needs
//     K / V transposed through LDS per iteration; it is the lever left if the launch proves VALU-bound at long caches (profiles/kv8_decode_step.txt).
//   * k_scale rides in the pre-scaled q (q_lds = rope(q) / sqrt(d) * k_scale), v_scale multiplies the normalised output once: the loop sees raw
//     bytes.  No kernel divides by a scale: the reciprocals are arguments.
//   * scalar and ragged launches are ONE instantiation: `active` may be NULL (scalar: every block reads pos[0]), which is a kernel argument, so
//     the choice is scalar arithmetic on addresses -- no branch and no dependent load in front of the ring in either form.  Both forms keep the
//     range guard: a position outside [0, Lc) writes zeros and appends nothing.
#pragma once
#include "bd_serving.h"

namespace bd {

typedef float kv8_f32x2_t __attribute__((ext_vector_type(2)));
constexpr float KV8_MAX = 448.f;

// the explicit fp32 clamp in front of the conversion (whether v_cvt_pk_fp8_f32 saturates is a mode bit); written as compares so that NaN stays NaN
__device__ __forceinline__ float kv8_clamp(float y) { return y > KV8_MAX ? KV8_MAX : (y < -KV8_MAX ? -KV8_MAX : y); }
// four values -> four bytes, value i in byte i
__device__ __forceinline__ uint32_t kv8_quant4(float a, float b, float c, float d, float inv) {
    const int lo = __builtin_amdgcn_cvt_pk_fp8_f32(kv8_clamp(a * inv), kv8_clamp(b * inv), 0, false);
    return (uint32_t)__builtin_amdgcn_cvt_pk_fp8_f32(kv8_clamp(c * inv), kv8_clamp(d * inv), lo, true);
}
__device__ __forceinline__ uint32_t kv8_quant1(float a, float inv) {
    const float y = kv8_clamp(a * inv);
    return (uint32_t)__builtin_amdgcn_cvt_pk_fp8_f32(y, y, 0, false) & 0xffu;
}
// eight 16-bit values (four dwords) -> eight bytes
template <int DT> __device__ __forceinline__ u32x2_t kv8_quant8(u32x4_t v, float inv) {
    u32x2_t o;
#pragma unroll
    for (int d = 0; d < 2; ++d)
        o[d] = kv8_quant4(half_bits_to_f32<DT>(v[2 * d] & 0xffffu), half_bits_to_f32<DT>(v[2 * d] >> 16),
                          half_bits_to_f32<DT>(v[2 * d + 1] & 0xffffu), half_bits_to_f32<DT>(v[2 * d + 1] >> 16), inv);
    return o;
}
// four bytes of a dword -> four floats (exact)
__device__ __forceinline__ void kv8_dequant4(uint32_t w, float* f) {
    const kv8_f32x2_t a = __builtin_amdgcn_cvt_pk_f32_fp8((int)w, false), b = __builtin_amdgcn_cvt_pk_f32_fp8((int)w, true);
    f[0] = a[0]; f[1] = a[1]; f[2] = b[0]; f[3] = b[1];
}

struct AttnKv8Params {
    const unsigned short* qkv;     // [T, (H + 2*KVH) * 128], as AttnParams
    const unsigned short* cos;     // [Lmax, 128], or [T, Lmax, 128] at tenant stride s_tab
    const unsigned short* sin;
    unsigned char* kc;             // e4m3 bytes [T, KVH, Lc, 128]
    unsigned char* vc;
    const float* k_scale;          // [T, KVH] fp32, and the host-computed reciprocals
    const float* v_scale;
    const float* k_inv;
    const float* v_inv;
    unsigned char* valid;          // [T, Lc]
    const long long* pos;          // one device scalar, or [T] when `active` is given
    const unsigned char* active;   // NULL = the scalar form
    unsigned short* out;           // [T, H * 128]
    int T, H, KVH, Lc;
    long long s_qkv, s_out;
    float scale;                   // 1 / sqrt(head_dim)
    float* ws;                     // split partials and tickets: decode_attn_kernel's layout and contract
    unsigned* tickets;
    int nsplit;
    long long s_tab;
};

template <int DT, int G, int DEPTH, int MAXS>
__global__ void __launch_bounds__(512) decode_attn_kv8_kernel(const AttnKv8Params p) {
    constexpr int HD = 128, NWV = 8, RPI = 4 * NWV;
    __shared__ float q_lds[G][HD];              // rotated queries, pre-scaled by k_scale / sqrt(d)
    __shared__ float kn_lds[HD], vn_lds[HD];    // the new token's key / value AS ITS BYTES READ BACK (what the next step will see)
    __shared__ float m_lds[NWV][G], s_lds[NWV][G];
    __shared__ float a_lds[NWV][G][HD];
    __shared__ int s_last;
    const int t = blockIdx.x / p.KVH, kvh = blockIdx.x % p.KVH;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    // position, activity byte and the four scales: uniform loads from addresses made of kernel arguments and blockIdx, issued together.  The
    // scalar form reads pos[0] and, in place of the activity byte, a word it ignores (the position's own low word: an address that is valid).
    const bool ragged = p.active != nullptr;
    const long long pt = p.pos[ragged ? t : 0];
    const uintptr_t ab = ragged ? (uintptr_t)(p.active + t) : (uintptr_t)p.pos;
    typedef const __attribute__((address_space(4))) uint32_t* const_word_ptr;         // (nothing writes pos / active during the launch)
    const uint32_t aw = *(const_word_ptr)(ab & ~(uintptr_t)3) >> (8 * (ab & 3));
    const float ks = p.k_scale[blockIdx.x], vs = p.v_scale[blockIdx.x], kinv = p.k_inv[blockIdx.x], vinv = p.v_inv[blockIdx.x];
    const bool act = !ragged || (aw & 0xffu) != 0;
    const bool in_cache = pt >= 0 && pt < p.Lc;
    const long long pos = in_cache ? pt : 0;                                         // clamped for addressing; the guard is tested behind the ring
    const unsigned short* row = p.qkv + (long long)t * p.s_qkv;
    const unsigned short* cs = p.cos + t * p.s_tab + pos * HD;
    const unsigned short* sn = p.sin + t * p.s_tab + pos * HD;
    unsigned char* kbase = p.kc + ((long long)t * p.KVH + kvh) * p.Lc * HD;
    unsigned char* vbase = p.vc + ((long long)t * p.KVH + kvh) * p.Lc * HD;
    const unsigned char* vld = p.valid + (long long)t * p.Lc;
    const int kq = lane >> 4, d8 = lane & 15;
    const int slot = 4 * wave + kq;
    const long long nrows_all = pos + 1;
    const long long per_split = ((nrows_all + p.nsplit - 1) / p.nsplit + RPI - 1) / RPI * RPI;
    const long long l_lo = (long long)blockIdx.y * per_split, l_hi = l_lo + per_split < nrows_all ? l_lo + per_split : nrows_all;
    const bool owns_new = l_lo <= pos && pos < l_hi;

    // (the validity byte stays raw and is tested where the row is used, as in decode_attn_kernel)
    struct Rows { u32x2_t kk, vv; uint32_t vb; bool in; };
    auto load_row = [&](long long l, Rows& r) {
        const bool in = l < pos && l < l_hi;              // row `pos` comes from LDS; every address is clamped into rows the block may read
        const long long lc = in ? l : 0;
        r.kk = *(const u32x2_t*)(kbase + lc * HD + 8 * d8);
        r.vv = *(const u32x2_t*)(vbase + lc * HD + 8 * d8);
        r.vb = vld[lc];
        r.in = in;
    };
    // ---- phase 0 inputs first, the ring behind them, the arithmetic after both (decode_attn_kernel's order and its reasons)
    const int i0 = min((int)threadIdx.x, G * HD - 1), g0 = i0 / HD, d0 = threadIdx.x % HD, dp0 = d0 < HD / 2 ? d0 + HD / 2 : d0 - HD / 2;
    const unsigned short* qrow0 = row + (long long)(kvh * G + g0) * HD;
    const unsigned short* krow = row + (long long)(p.H + kvh) * HD;
    const unsigned short rq_x = qrow0[d0], rq_r = qrow0[dp0], r_cs = cs[d0], r_sn = sn[d0];
    const unsigned short rk_x = krow[d0], rk_r = krow[dp0], r_vn = row[(long long)(p.H + p.KVH + kvh) * HD + d0];
    asm volatile("" ::: "memory");
    __builtin_amdgcn_sched_barrier(0);
    Rows ring[DEPTH];
#pragma unroll
    for (int u = 0; u < DEPTH; ++u) load_row(l_lo + (long long)u * RPI + slot, ring[u]);
    asm volatile("" ::: "memory");                       // (keeps the ring's loads in front of the branch)
    if (!(in_cache && act)) {                            // uniform over the block, and over the splits of its (tenant, kv head) pair
        if (blockIdx.y == 0)
            for (int i = threadIdx.x; i < G * HD; i += 64 * NWV) p.out[(long long)t * p.s_out + (long long)kvh * G * HD + i] = 0;
        return;
    }

    // ---- phase 0: RoPE of the G query heads and of the new key (rounded as the 16-bit kernel rounds), quantise, append
    auto rope_bits = [&](unsigned short xb, unsigned short xrb, unsigned short cb, unsigned short sb) {
        const float a = round16<DT>(half_bits_to_f32<DT>(xb) * half_bits_to_f32<DT>(cb));
        return round16<DT>(a + half_bits_to_f32<DT>(xrb) * half_bits_to_f32<DT>(sb));
    };
    auto rope = [&](const unsigned short* v, int d) { return rope_bits(v[d], v[d < HD / 2 ? d + HD / 2 : d - HD / 2], cs[d], sn[d]); };
    const float qs = p.scale * ks;
    if ((int)threadIdx.x < G * HD) q_lds[g0][d0] = rope_bits(rq_x, rq_r, r_cs, r_sn) * qs;
    for (int i = threadIdx.x + 64 * NWV; i < G * HD; i += 64 * NWV) {          // (G = 8: the second half of the query heads)
        const int g = i / HD, d = i % HD;
        q_lds[g][d] = rope(row + (long long)(kvh * G + g) * HD, d) * qs;
    }
    if (owns_new && threadIdx.x >= 64 * NWV - HD) {      // the last two waves: one element each
        const int d = d0;
        const uint32_t kb = kv8_quant1(rope_bits(rk_x, rk_r, r_cs, r_sn), kinv), vb = kv8_quant1(half_bits_to_f32<DT>(r_vn), vinv);
        kn_lds[d] = __builtin_amdgcn_cvt_pk_f32_fp8((int)kb, false)[0];
        vn_lds[d] = __builtin_amdgcn_cvt_pk_f32_fp8((int)vb, false)[0];
        kbase[pos * HD + d] = (unsigned char)kb;
        vbase[pos * HD + d] = (unsigned char)vb;
        if (d == 0 && kvh == 0) p.valid[(long long)t * p.Lc + pos] = 1;
    }
    __syncthreads();
    float q[G][8];
#pragma unroll
    for (int g = 0; g < G; ++g)
#pragma unroll
        for (int e = 0; e < 8; ++e) q[g][e] = q_lds[g][8 * d8 + e];
    float m[G], s[G], acc[G][8];
#pragma unroll
    for (int g = 0; g < G; ++g) {
        m[g] = -1e30f; s[g] = 0.f;
#pragma unroll
        for (int e = 0; e < 8; ++e) acc[g][e] = 0.f;
    }
    auto score_row = [&](const float (&kf)[8], const float (&vf)[8], bool valid_row) {
        float scv[G];
#pragma unroll
        for (int g = 0; g < G; ++g) {
            float sc = 0.f;
#pragma unroll
            for (int e = 0; e < 8; ++e) sc += q[g][e] * kf[e];
            scv[g] = row16_sum(sc);
        }
#pragma unroll
        for (int g = 0; g < G; ++g) {
            const float sc = scv[g];
            if (valid_row) {                                                         // uniform within the 16 lanes of a row
                const float mn = fmaxf(m[g], sc), f = __expf(m[g] - mn), pw = __expf(sc - mn);
                s[g] = s[g] * f + pw;
#pragma unroll
                for (int e = 0; e < 8; ++e) acc[g][e] = acc[g][e] * f + pw * vf[e];
                m[g] = mn;
            }
        }
    };
    const long long niter = l_hi > l_lo ? (l_hi - l_lo + RPI - 1) / RPI : 0;   // uniform over the block
    for (long long it0 = 0; it0 < niter; it0 += DEPTH) {
#pragma unroll
        for (int u = 0; u < DEPTH; ++u) {
            const long long l = l_lo + (it0 + u) * RPI + slot;
            float kf[8], vf[8];
            bool use = ring[u].in && ring[u].vb != 0;
            if (l == pos && owns_new) {
                use = true;
#pragma unroll
                for (int e = 0; e < 8; ++e) { kf[e] = kn_lds[8 * d8 + e]; vf[e] = vn_lds[8 * d8 + e]; }
            } else {
                kv8_dequant4(ring[u].kk[0], kf); kv8_dequant4(ring[u].kk[1], kf + 4);
                kv8_dequant4(ring[u].vv[0], vf); kv8_dequant4(ring[u].vv[1], vf + 4);
            }
            score_row(kf, vf, use);
            load_row(l + (long long)DEPTH * RPI, ring[u]);                   // refill this slot DEPTH iterations ahead
        }
    }
    // merge the 4 row slots of the wave, then the 8 waves through LDS (decode_attn_kernel's order: the split partials have its layout)
#pragma unroll
    for (int o = 16; o <= 32; o <<= 1) {
#pragma unroll
        for (int g = 0; g < G; ++g) {
            const float mo = __shfl_xor(m[g], o, 64), so = __shfl_xor(s[g], o, 64);
            const float mn = fmaxf(m[g], mo), f1 = __expf(m[g] - mn), f2 = __expf(mo - mn);
            s[g] = s[g] * f1 + so * f2;
#pragma unroll
            for (int e = 0; e < 8; ++e) acc[g][e] = acc[g][e] * f1 + __shfl_xor(acc[g][e], o, 64) * f2;
            m[g] = mn;
        }
    }
    if (kq == 0) {
#pragma unroll
        for (int g = 0; g < G; ++g) {
            if (d8 == 0) { m_lds[wave][g] = m[g]; s_lds[wave][g] = s[g]; }
#pragma unroll
            for (int e = 0; e < 8; ++e) a_lds[wave][g][8 * d8 + e] = acc[g][e];
        }
    }
    __syncthreads();
    for (int i = threadIdx.x; i < G * HD; i += 64 * NWV) {
        const int g = i / HD, d = i % HD;
        float mm = -1e30f;
#pragma unroll
        for (int j = 0; j < NWV; ++j) mm = fmaxf(mm, m_lds[j][g]);
        float ssum = 0.f, a = 0.f;
#pragma unroll
        for (int j = 0; j < NWV; ++j) {
            const float f = __expf(m_lds[j][g] - mm);
            ssum += s_lds[j][g] * f;
            a += a_lds[j][g][d] * f;
        }
        if (p.nsplit == 1) {
            p.out[(long long)t * p.s_out + (long long)(kvh * G + g) * HD + d] = (unsigned short)f32_to_half_bits<DT>(a / ssum * vs);
        } else {                                         // partial of this split: un-normalised accumulator (in byte units), running max, sum
            float* w = p.ws + (((long long)blockIdx.x * p.nsplit + blockIdx.y) * G + g) * (HD + 2);
            attn_ws_store(&w[d], a);
            if (d == 0) { attn_ws_store(&w[HD], mm); attn_ws_store(&w[HD + 1], ssum); }
        }
    }
    if (p.nsplit == 1) return;
    // in-launch merge: decode_attn_kernel's protocol (agent-scope relaxed atomics, vmcnt(0) + barrier -> ticket -> the last block merges in
    // split order and puts the ticket back to zero), so the result does not depend on which block arrives last
    __builtin_amdgcn_s_waitcnt(0x0f70);               // vmcnt(0)
    __syncthreads();
    if (threadIdx.x == 0)
        s_last = __hip_atomic_fetch_add(&p.tickets[blockIdx.x], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == (unsigned)(p.nsplit - 1);
    __syncthreads();
    if (!s_last) return;
    for (int i = threadIdx.x; i < G * HD; i += 64 * NWV) {
        const int g = i / HD, d = i % HD;
        const float* w = p.ws + ((long long)blockIdx.x * p.nsplit * G + g) * (HD + 2);
        float mv[MAXS], sv[MAXS], av[MAXS];              // every partial of this element is fetched first, then merged in split order
#pragma unroll
        for (int c = 0; c < MAXS; ++c) {
            const float* wc = w + (long long)min(c, p.nsplit - 1) * G * (HD + 2);
            mv[c] = attn_ws_load(&wc[HD]);
            sv[c] = attn_ws_load(&wc[HD + 1]);
            av[c] = attn_ws_load(&wc[d]);
        }
        float mm = -1e30f;
#pragma unroll
        for (int c = 0; c < MAXS; ++c) if (c < p.nsplit) mm = fmaxf(mm, mv[c]);
        float ssum = 0.f, a = 0.f;
#pragma unroll
        for (int c = 0; c < MAXS; ++c) {
            if (c < p.nsplit) {
                const float f = __expf(mv[c] - mm);
                ssum += sv[c] * f;
                a += av[c] * f;
            }
        }
        p.out[(long long)t * p.s_out + (long long)(kvh * G + g) * HD + d] = (unsigned short)f32_to_half_bits<DT>(a / ssum * vs);
    }
    if (threadIdx.x == 0) __hip_atomic_store(&p.tickets[blockIdx.x], 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// rope_kv_append_kernel with an 8-bit cache: the same RoPE of the q and k heads in place in the 16-bit qkv (bit for bit), the rotated k rows and
// the v rows quantised on their way to the caches.  One block per token row.  A k thread owns dims d0 .. d0 + 7 and their partners at + 64: two
// 8-byte stores; a v thread owns 16 dims: 32 bytes in, one 16-byte store.
template <int DT>
__global__ void __launch_bounds__(256) rope_kv_append_kv8_kernel(unsigned short* __restrict__ x, const unsigned short* __restrict__ cos_t,
                                                                 const unsigned short* __restrict__ sin_t, long long s_tab,
                                                                 unsigned char* __restrict__ kc, unsigned char* __restrict__ vc,
                                                                 const float* __restrict__ k_inv, const float* __restrict__ v_inv, int H, int KVH,
                                                                 long long sx, int seq, int pos0, int Lc) {
    const int r = blockIdx.x, t = r / seq;
    const long long pos = pos0 + (r - t * seq);
    const unsigned short* cs = cos_t + t * s_tab + pos * 128;
    const unsigned short* sn = sin_t + t * s_tab + pos * 128;
    unsigned short* row = x + (long long)r * sx;
    const int nrope = (H + KVH) * 8, ntot = nrope + KVH * 8;
    for (int i = threadIdx.x; i < ntot; i += 256) {
        if (i >= nrope) {                                               // v head (i - nrope) / 8, dims 16 * ((i - nrope) % 8) .. + 15
            const int j = i - nrope, hv = j >> 3, d0 = (j & 7) * 16;
            const unsigned short* src = row + (long long)(H + KVH + hv) * 128 + d0;
            const float inv = v_inv[t * KVH + hv];
            const u32x2_t lo = kv8_quant8<DT>(*(const u32x4_t*)src, inv), hi = kv8_quant8<DT>(*(const u32x4_t*)(src + 8), inv);
            *(u32x4_t*)(vc + (((long long)t * KVH + hv) * Lc + pos) * 128 + d0) = u32x4_t{lo[0], lo[1], hi[0], hi[1]};
            continue;
        }
        const int h = i >> 3, d0 = (i & 7) * 8;
        unsigned short* px = row + h * 128;
        const u32x4_t lo = *(const u32x4_t*)(px + d0), hi = *(const u32x4_t*)(px + 64 + d0);
        const u32x4_t cl = *(const u32x4_t*)(cs + d0), ch = *(const u32x4_t*)(cs + 64 + d0);
        const u32x4_t sl = *(const u32x4_t*)(sn + d0), sh = *(const u32x4_t*)(sn + 64 + d0);
        u32x4_t ol, oh;
#pragma unroll
        for (int d = 0; d < 4; ++d) {
            uint32_t rl = 0, rh = 0;
#pragma unroll
            for (int e = 0; e < 2; ++e) {
                const int shf = 16 * e;
                const float a = half_bits_to_f32<DT>((lo[d] >> shf) & 0xffffu), b = half_bits_to_f32<DT>((hi[d] >> shf) & 0xffffu);
                const float c0 = half_bits_to_f32<DT>((cl[d] >> shf) & 0xffffu), c1 = half_bits_to_f32<DT>((ch[d] >> shf) & 0xffffu);
                const float s0 = half_bits_to_f32<DT>((sl[d] >> shf) & 0xffffu), s1 = half_bits_to_f32<DT>((sh[d] >> shf) & 0xffffu);
                rl |= f32_to_half_bits<DT>(round16<DT>(a * c0) + b * s0) << shf;
                rh |= f32_to_half_bits<DT>(round16<DT>(b * c1) + a * s1) << shf;
            }
            ol[d] = rl; oh[d] = rh;
        }
        *(u32x4_t*)(px + d0) = ol;
        *(u32x4_t*)(px + 64 + d0) = oh;
        if (h >= H) {
            const float inv = k_inv[t * KVH + (h - H)];
            unsigned char* pk = kc + (((long long)t * KVH + (h - H)) * Lc + pos) * 128;
            *(u32x2_t*)(pk + d0) = kv8_quant8<DT>(ol, inv);
            *(u32x2_t*)(pk + 64 + d0) = kv8_quant8<DT>(oh, inv);
        }
    }
}

// Rows [r0, r1) of one layer's byte caches [NTH = T * KVH, Lc, 128] -> round16(float(byte) * scale) at the same rows of a 16-bit scratch of the same
// shape: what bd_srv_prefill_attention_cached reads when a chunk continues an fp8 conversation.  blockIdx.y: 0 = keys, 1 = values.  A thread
// turns 16 bytes into two full 16-byte stores; rows outside the range are not touched.  No LDS.
template <int DT>
__global__ void __launch_bounds__(256) kv8_expand_kernel(const unsigned char* __restrict__ kc, const unsigned char* __restrict__ vc,
                                                         const float* __restrict__ k_scale, const float* __restrict__ v_scale,
                                                         unsigned short* __restrict__ k16, unsigned short* __restrict__ v16, int nth, int Lc, int r0,
                                                         int r1) {
    const bool isv = blockIdx.y != 0;
    const unsigned char* src = isv ? vc : kc;
    unsigned short* dst = isv ? v16 : k16;
    const long long gid = (long long)blockIdx.x * 256 + threadIdx.x, rowi = gid >> 3;
    const int c = (int)(gid & 7), nr = r1 - r0;
    if (rowi >= (long long)nth * nr) return;
    const int th = (int)(rowi / nr), r = r0 + (int)(rowi % nr);
    const float sc = (isv ? v_scale : k_scale)[th];
    const long long off = ((long long)th * Lc + r) * 128 + 16 * c;
    const u32x4_t b = *(const u32x4_t*)(src + off);
    u32x4_t o[2];
#pragma unroll
    for (int d = 0; d < 4; ++d) {
        float f[4];
        kv8_dequant4(b[d], f);
        o[d >> 1][2 * (d & 1)] = f32_to_half_bits<DT>(f[0] * sc) | (f32_to_half_bits<DT>(f[1] * sc) << 16);
        o[d >> 1][2 * (d & 1) + 1] = f32_to_half_bits<DT>(f[2] * sc) | (f32_to_half_bits<DT>(f[3] * sc) << 16);
    }
    *(u32x4_t*)(dst + off) = o[0];
    *(u32x4_t*)(dst + off + 8) = o[1];
}

}  // namespace bd
