// Fused binary-delta Linear over the INT8 base weight for M >= 2 rows per batch entry (prefill, extend, chunks, scoring):
//
//   Y[b,m,n] = round( wscale[n] * sum_k X[b,m,k] CB[n,k]  +  alpha[b,g(n)] * sum_k X[b,m,k] S_b[k,n]  [+ Y_in[b,m,n]] )
//
// bd_binary_linear_decode_w8's formula (bd_gemv_stream.h, WT = 2) on the SAME bytes: the base operand is the tile-major decode copy
// W8'[n/16][k/128][h][16 c][4 g][j][8] (quant.tile_weight_int8), so an int8 model keeps ONE copy of its base.  bd_gemm_fx.h takes a
// row-major 16-bit W through LDS; the decode kernel is a GEMV stream whose waves split k.  Here:
//   * v_mfma_f32_16x16x32 with the WEIGHT as the A operand: D[output column][activation row].  The byte layout already is that operand's
//     order -- lane (c, g) of a 16-column tile owns 16 contiguous bytes of run h, its k-octets of steps 2 h and 2 h + 1 -- so the base goes
//     global -> registers -> widen_i8x8 -> MFMA and never touches LDS; a wave's load instruction reads one contiguous 1-KiB run.
//   * a workgroup is NW waves over a [16 RB rows] x [16 NW columns] output tile.  Wave w owns ONE column tile (n0 + 16 w) and ALL RB row
//     blocks: a widened fragment (12 VALU) and an expanded sign fragment (8 VALU) feed RB MFMAs each.
//   * X goes through LDS once per workgroup, already in fragment order: in iteration `it` wave w fetches MFMA step w & 3 of its share of the
//     row blocks (all of them with 4 waves, half with 8; lane (c, g): the octet k = 128 it + 32 (w & 3) + 8 g of row 16 rb + c, 64 contiguous
//     bytes per row and instruction) and writes it as the 1-KiB run [rb][step][lane]; every wave then reads fragment (rb, s) as one
//     conflict-free ds_read_b128 run.  Two stages, one barrier per iteration: stage (it + 1) & 1 is written after the barrier that ended
//     its last reads and read after the next one.
//   * signs come in the reference layout P[K/32, N]: lane (c, g) loads ONE word per iteration (word row 4 it + g, column c: 64-byte runs).
//     The MFMA wants byte g of word row 4 it + s in step s, so the four lane groups of a column exchange bytes (a 4 x 4 byte transpose over
//     lanes c, c + 16, c + 32, c + 48: four ds_bpermute per tile and iteration); the lane's transposed word then feeds its four steps through
//     expand_signs8, as in bd_gemm_mfma.h.  Base and delta keep separate accumulators: wscale multiplies the finished base sum once.
//   * the byte loads, the sign words and the X fragments of iteration it + 1 are issued before the MFMAs of iteration it (a two-deep
//     register ring, unrolled by two so no register is copied); hipcc's in-order vmcnt counting keeps them in flight across the MFMAs.
//   * rows past M are clamped on load and skipped on store; a column tile past N (N % 16 == 0: whole tiles) is clamped on load and
//     skipped on store.  No workspace, no split-k, no atomics: the result is a pure function of the inputs and the launch captures as it is.
// Plans (w8_plan in bd_api.hip): M <= 16 / 32 / 64 -> RB = 1 / 2 / 4 with NW = 4 (64 columns per workgroup: N/64 x B workgroups for a
// few-token extend); above, RB = 8 and NW = 8 (128 x 128: 64 accumulator registers per wave, two waves per SIMD, 8 MFMAs per fragment).
#pragma once
#include "bd_gemv_stream.h"

namespace bd {

struct W8Params {
    const unsigned short* X;   // [B, M, K]
    const int8_t* W8;          // tile-major bytes
    const float* wscale;       // [N]
    const uint32_t* P;         // [B or 1, K/32, N]
    const float* alpha;        // [B or 1, G]
    void* C;                   // [B, M, N]
    int M, N, K, gsz, tiles_m;
    long long sXb, sXm, sPb, sAlb, sCb, sCm;
    int out_f32, accumulate;
    int vec;                   // every output row is aligned for one 4-column store (8 bytes, fp32: 16)
};

template <int DT, int RB, int NW>
__global__ void __launch_bounds__(64 * NW) gemm_w8_kernel(const W8Params p) {
    static_assert((NW == 4 || NW == 8) && (RB * 4) % NW == 0, "4 waves stage every row block, 8 waves half of them each");
    constexpr int SB = RB * 4 / NW;               // row blocks a wave stages
    constexpr int XSTAGE = RB * 4 * 1024;         // [RB row blocks][4 steps][64 lanes] 16-byte fragments
    __shared__ __attribute__((aligned(16))) char xs[2 * XSTAGE];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int c = lane & 15, g = lane >> 4;
    const int b = blockIdx.y;
    const int tile_m = blockIdx.x % p.tiles_m, grp = blockIdx.x / p.tiles_m;      // row tiles fastest: neighbours share the byte stream
    const int m0 = tile_m * 16 * RB;
    const int nit = p.K >> 7, ntile = p.N >> 4;
    const int tile = grp * NW + wave;             // this wave's column tile
    const int xstep = wave & 3, xrb0 = (wave >> 2) * SB;      // what this wave stages: MFMA step xstep of row blocks xrb0 .. xrb0 + SB - 1

    const char* xsrc[SB];
#pragma unroll
    for (int i = 0; i < SB; ++i) {
        const int r = min(m0 + 16 * (xrb0 + i) + c, p.M - 1);
        xsrc[i] = (const char*)p.X + ((long long)b * p.sXb + (long long)r * p.sXm) * 2 + (32 * xstep + 8 * g) * 2;
    }
    const int tl = min(tile, ntile - 1);
    const char* wsrc = (const char*)p.W8 + (size_t)tl * nit * 2048 + c * 64 + g * 16;
    const uint32_t* psrc = p.P + (long long)b * p.sPb + (size_t)g * p.N + tl * 16 + c;

    f32x4_t accW[RB], accS[RB];
#pragma unroll
    for (int rb = 0; rb < RB; ++rb) { accW[rb] = f32x4_t{0.f, 0.f, 0.f, 0.f}; accS[rb] = f32x4_t{0.f, 0.f, 0.f, 0.f}; }

    struct Stage { u32x4_t w[2]; uint32_t s; };
    auto issue = [&](Stage& st, u32x4_t (&xr)[SB], int it) {
        const char* src = wsrc + (size_t)it * 2048;
        st.w[0] = *(const u32x4_t*)src;
        st.w[1] = *(const u32x4_t*)(src + 1024);
        st.s = psrc[(size_t)it * 4 * p.N];
#pragma unroll
        for (int i = 0; i < SB; ++i) xr[i] = *(const u32x4_t*)(xsrc[i] + (size_t)it * 256);
    };
    auto stage_x = [&](const u32x4_t (&xr)[SB], int buf) {
#pragma unroll
        for (int i = 0; i < SB; ++i) *(u32x4_t*)(xs + buf * XSTAGE + (((xrb0 + i) * 4 + xstep) * 64 + lane) * 16) = xr[i];
    };
    auto compute = [&](const Stage& st, int buf) {
        // the lane's transposed sign word (byte s = signs of step s), inverted, each 16-bit half replicated for expand_signs8
        uint32_t tw = 0;
#pragma unroll
        for (int s = 0; s < 4; ++s) tw |= ((__shfl(st.s, c + 16 * s, 64) >> (8 * g)) & 0xffu) << (8 * s);
        tw = ~tw;
        const uint32_t rep[2] = {(tw & 0xffffu) * 0x10001u, (tw >> 16) * 0x10001u};
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            u32x4_t xf[RB];
#pragma unroll
            for (int rb = 0; rb < RB; ++rb) xf[rb] = *(const u32x4_t*)(xs + buf * XSTAGE + ((rb * 4 + s) * 64 + lane) * 16);
            const u32x4_t wf = widen_i8x8<DT>(st.w[s >> 1][2 * (s & 1)], st.w[s >> 1][2 * (s & 1) + 1]);
            const u32x4_t sf = expand_signs8(rep[s >> 1], 4 * (s & 1), One2<DT>::v);
#pragma unroll
            for (int rb = 0; rb < RB; ++rb) {
                accW[rb] = mfma16<DT>(wf, xf[rb], accW[rb]);
                accS[rb] = mfma16<DT>(sf, xf[rb], accS[rb]);
            }
        }
    };
    // one k-iteration: prefetch it + 1 into the other ring slot, run the MFMAs of `it`, hand the next X stage to LDS
    auto step = [&](const Stage& cur, Stage& nxt, int it) {
        const bool more = it + 1 < nit;           // (workgroup-uniform)
        u32x4_t xr[SB];
        if (more) issue(nxt, xr, it + 1);
        compute(cur, it & 1);
        if (more) stage_x(xr, (it + 1) & 1);
        __syncthreads();
    };

    Stage st0, st1;
    {
        u32x4_t xr[SB];
        issue(st0, xr, 0);
        stage_x(xr, 0);
        __syncthreads();
    }
    for (int it = 0; it < nit; it += 2) {
        step(st0, st1, it);
        if (it + 1 < nit) step(st1, st0, it + 1);
    }

    // ---- out = wscale[n] * accW + alpha[g(n)] * accS (+ Y_in), one rounding.  Lane (c, g): row 16 rb + c, columns 4 g .. 4 g + 3 of the tile
    const float* al = p.alpha + (long long)b * p.sAlb;
    if (tile < ntile) {                           // (wave-uniform)
        const int n = tile * 16 + 4 * g;
        const f32x4_t ws = *(const f32x4_t*)(p.wscale + n);
        float a[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) a[e] = al[(n + e) / p.gsz];
#pragma unroll
        for (int rb = 0; rb < RB; ++rb) {
            const int m = m0 + 16 * rb + c;
            if (m >= p.M) continue;
            f32x4_t v = scale_base(accW[rb], ws);
#pragma unroll
            for (int e = 0; e < 4; ++e) v[e] = scale_then_add(accS[rb][e], a[e], v[e]);
            const long long off = (long long)b * p.sCb + (long long)m * p.sCm + n;
            if (p.out_f32) {
                float* dst = (float*)p.C + off;
                if (p.vec) {
                    if (p.accumulate) v += *(const f32x4_t*)dst;
                    *(f32x4_t*)dst = v;
                } else {
#pragma unroll
                    for (int e = 0; e < 4; ++e) dst[e] = p.accumulate ? v[e] + dst[e] : v[e];
                }
            } else {
                unsigned short* dst = (unsigned short*)p.C + off;
                if (p.vec) {
                    if (p.accumulate) {
                        const u32x2_t cin = *(const u32x2_t*)dst;
#pragma unroll
                        for (int e = 0; e < 4; ++e) v[e] += half_bits_to_f32<DT>((cin[e >> 1] >> (16 * (e & 1))) & 0xffffu);
                    }
                    u32x2_t o;
                    o[0] = (f32_to_half_bits<DT>(v[0]) & 0xffffu) | (f32_to_half_bits<DT>(v[1]) << 16);
                    o[1] = (f32_to_half_bits<DT>(v[2]) & 0xffffu) | (f32_to_half_bits<DT>(v[3]) << 16);
                    *(u32x2_t*)dst = o;
                } else {
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        const float r = p.accumulate ? v[e] + half_bits_to_f32<DT>(dst[e]) : v[e];
                        dst[e] = (unsigned short)f32_to_half_bits<DT>(r);
                    }
                }
            }
        }
    }
}

}  // namespace bd
