// Fused binary-delta Linear over the 4-BIT GPTQ base weight for M >= 2 rows per batch entry (prefill, extend, chunks, scoring):
//
//   Y[b,m,n] = round( sum_k X[b,m,k] Wdq[n,k]  +  alpha[b,g(n)] * sum_k X[b,m,k] S_b[k,n]  [+ Y_in[b,m,n]] )
//   Wdq[n,k] = dtype( fp16( (q[n,k] - z[group(k),n]) * scale[group(k),n] ) )
//
// bd_binary_linear_decode_q4's formula (bd_gemv_stream.h, WT = 3) on the SAME operands: the tile-major nibbles W4'[n/16][k/128][16 c][4 g][4 s]
// (quant.tile_weight_gptq4) and the packed (scale, 1024 + z) dwords [n/16][k/G][16 c] (quant.pack_gptq4_params), so a 4-bit model keeps ONE
// copy of its base.  Wdq is bit for bit what the reference's dequantisation leaves in the model (dequant_q4x8); no scale is left for the
// epilogue.  The skeleton is gemm_w8_kernel's (bd_gemm_w8.h): v_mfma_f32_16x16x32 with the WEIGHT as the A operand, D[output column][activation
// row]; X staged once per workgroup through LDS in fragment order, two stages, one barrier per iteration; one sign word per lane, tile and
// iteration with the 4 x 4 byte exchange across lane groups; a two-slot register prefetch; clamped loads and skipped stores at the edges; no
// workspace, no split-k, no atomics, no scratch.  What the format changes:
//   * a wave's weight stage of one column tile is ONE 16-byte load per lane -- lane (c, g) reads dwords [c][g][0..3] of the contiguous 1-KiB
//     block of (tile, iteration): its k-octets k = 128 it + 32 s + 8 g of MFMA steps s = 0 .. 3, nibbles interleaved as dequant_q4x8 wants
//     them -- 4 registers against int8's 8 and 16-bit's 16.  The base goes global -> registers -> dequant_q4x8 -> MFMA and never touches LDS.
//   * the group parameters ride with the stage: one dword per lane and tile, (tile, it / (G / 128), c) -- G % 128 == 0, a stage lies in one
//     group; the division is a scalar multiply-high by a host-made magic number (0 = G is 128), as in the decode kernel.  v_perm_b32 splits it
//     into the packed pairs zz = (1024 + z, 1024 + z) and ss = (scale, scale).
//   * TW = 2: with the registers the small stage leaves free a wave owns TWO adjacent column tiles (32 columns, both sign words of a lane in
//     one 128-byte run) and 2 x RB x 2 accumulators.  Every wave reads the whole X stage from LDS whatever it owns, so one 16-byte fragment
//     read now feeds FOUR MFMAs (two base, two delta) instead of two, and a workgroup of NW waves shares one X stage among 2 NW column tiles:
//     half the LDS reads, half the X staging and half the barriers per output element.  128 accumulator registers at RB = 8: two waves per
//     SIMD.  TW = 1 is gemm_w8_kernel's split; q4_plan (bd_api.hip) says which plan takes which, from the measured A/B
//     (profiles/q4_prefill.txt).
// A workgroup is NW waves over [16 RB rows] x [16 NW TW columns]; wave w owns column tiles (group NW + w) TW + j and ALL RB row blocks.
#pragma once
#include "bd_gemm_w8.h"

namespace bd {

struct Q4Params {
    const unsigned short* X;   // [B, M, K]
    const uint32_t* W4;        // tile-major nibbles
    const uint32_t* qp;        // [N/16][K/G][16] packed (scale, 1024 + z)
    const uint32_t* P;         // [B or 1, K/32, N]
    const float* alpha;        // [B or 1, G]
    void* C;                   // [B, M, N]
    int M, N, K, gsz, tiles_m;
    uint32_t ngrp, magic;      // K / G; floor(2^32 / (G / 128)) + 1, 0 when G == 128
    long long sXb, sXm, sPb, sAlb, sCb, sCm;
    int out_f32, accumulate;
    int vec;                   // every output row is aligned for one 4-column store (8 bytes, fp32: 16)
};

// out = accW + alpha[g(n)] * accS (+ Y_in), one rounding: lane (c, g) holds columns n .. n + 3 of row m
template <int DT> __device__ __forceinline__ void q4_store4(const Q4Params& p, long long off, f32x4_t v) {
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

template <int DT, int RB, int NW, int TW>
__global__ void __launch_bounds__(64 * NW) gemm_q4_kernel(const Q4Params p) {
    static_assert((NW == 4 || NW == 8) && (RB * 4) % NW == 0 && (TW == 1 || TW == 2), "4 waves stage every row block, 8 waves half of them each");
    constexpr int SB = RB * 4 / NW;               // row blocks a wave stages
    constexpr int XSTAGE = RB * 4 * 1024;         // [RB row blocks][4 steps][64 lanes] 16-byte fragments
    __shared__ __attribute__((aligned(16))) char xs[2 * XSTAGE];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int c = lane & 15, g = lane >> 4;
    const int b = blockIdx.y;
    const int tile_m = blockIdx.x % p.tiles_m, grp = blockIdx.x / p.tiles_m;      // row tiles fastest: neighbours share the nibble stream
    const int m0 = tile_m * 16 * RB;
    const int nit = p.K >> 7, ntile = p.N >> 4;
    const int tile0 = (grp * NW + wave) * TW;     // this wave's first column tile
    const int xstep = wave & 3, xrb0 = (wave >> 2) * SB;      // what this wave stages: MFMA step xstep of row blocks xrb0 .. xrb0 + SB - 1

    const char* xsrc[SB];
#pragma unroll
    for (int i = 0; i < SB; ++i) {
        const int r = min(m0 + 16 * (xrb0 + i) + c, p.M - 1);
        xsrc[i] = (const char*)p.X + ((long long)b * p.sXb + (long long)r * p.sXm) * 2 + (32 * xstep + 8 * g) * 2;
    }
    const char* wsrc[TW];
    const uint32_t* qsrc[TW];
    const uint32_t* psrc[TW];
#pragma unroll
    for (int j = 0; j < TW; ++j) {
        const int tl = min(tile0 + j, ntile - 1);
        wsrc[j] = (const char*)p.W4 + (size_t)tl * nit * 1024 + c * 64 + g * 16;
        qsrc[j] = p.qp + (size_t)tl * p.ngrp * 16 + c;
        psrc[j] = p.P + (long long)b * p.sPb + (size_t)g * p.N + tl * 16 + c;
    }

    f32x4_t accW[TW][RB], accS[TW][RB];
#pragma unroll
    for (int j = 0; j < TW; ++j)
#pragma unroll
        for (int rb = 0; rb < RB; ++rb) { accW[j][rb] = f32x4_t{0.f, 0.f, 0.f, 0.f}; accS[j][rb] = f32x4_t{0.f, 0.f, 0.f, 0.f}; }

    struct Stage { u32x4_t w[TW]; uint32_t s[TW], q[TW]; };
    auto issue = [&](Stage& st, u32x4_t (&xr)[SB], int it) {
        const uint32_t gk = p.magic ? __umulhi((uint32_t)it, p.magic) : (uint32_t)it;      // (workgroup-uniform: scalar) the k-group of this stage
#pragma unroll
        for (int j = 0; j < TW; ++j) {
            st.w[j] = *(const u32x4_t*)(wsrc[j] + (size_t)it * 1024);
            st.s[j] = psrc[j][(size_t)it * 4 * p.N];
            st.q[j] = qsrc[j][gk * 16u];
        }
#pragma unroll
        for (int i = 0; i < SB; ++i) xr[i] = *(const u32x4_t*)(xsrc[i] + (size_t)it * 256);
    };
    auto stage_x = [&](const u32x4_t (&xr)[SB], int buf) {
#pragma unroll
        for (int i = 0; i < SB; ++i) *(u32x4_t*)(xs + buf * XSTAGE + (((xrb0 + i) * 4 + xstep) * 64 + lane) * 16) = xr[i];
    };
    auto compute = [&](const Stage& st, int buf) {
        uint32_t rep[TW][2], zz[TW], ss[TW];
#pragma unroll
        for (int j = 0; j < TW; ++j) {
            // the lane's transposed sign word (byte s = signs of step s), inverted, each 16-bit half replicated for expand_signs8
            uint32_t tw = 0;
#pragma unroll
            for (int s = 0; s < 4; ++s) tw |= ((__shfl(st.s[j], c + 16 * s, 64) >> (8 * g)) & 0xffu) << (8 * s);
            tw = ~tw;
            rep[j][0] = (tw & 0xffffu) * 0x10001u;
            rep[j][1] = (tw >> 16) * 0x10001u;
            zz[j] = __builtin_amdgcn_perm(st.q[j], st.q[j], 0x03020302u);
            ss[j] = __builtin_amdgcn_perm(st.q[j], st.q[j], 0x01000100u);
        }
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            // 128 accumulator registers leave the scheduler no room to pull the next steps' fragments forward: left alone it does and spills
            if constexpr (TW * RB == 16) __builtin_amdgcn_sched_barrier(0);
            u32x4_t wf[TW], sf[TW];
#pragma unroll
            for (int j = 0; j < TW; ++j) {
                wf[j] = dequant_q4x8<DT>(st.w[j][s], zz[j], ss[j]);
                sf[j] = expand_signs8(rep[j][s >> 1], 4 * (s & 1), One2<DT>::v);
            }
#pragma unroll
            for (int rb = 0; rb < RB; ++rb) {
                const u32x4_t xf = *(const u32x4_t*)(xs + buf * XSTAGE + ((rb * 4 + s) * 64 + lane) * 16);
#pragma unroll
                for (int j = 0; j < TW; ++j) {
                    accW[j][rb] = mfma16<DT>(wf[j], xf, accW[j][rb]);
                    accS[j][rb] = mfma16<DT>(sf[j], xf, accS[j][rb]);
                }
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

    // ---- out = accW + alpha[g(n)] * accS (+ Y_in), one rounding.  Lane (c, g): row 16 rb + c, columns 4 g .. 4 g + 3 of each of its tiles
    const float* al = p.alpha + (long long)b * p.sAlb;
#pragma unroll
    for (int j = 0; j < TW; ++j) {
        if (tile0 + j >= ntile) break;            // (wave-uniform)
        const int n = (tile0 + j) * 16 + 4 * g;
        float a[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) a[e] = al[(n + e) / p.gsz];
#pragma unroll
        for (int rb = 0; rb < RB; ++rb) {
            const int m = m0 + 16 * rb + c;
            if (m >= p.M) continue;
            f32x4_t v;
#pragma unroll
            for (int e = 0; e < 4; ++e) v[e] = scale_then_add(accS[j][rb][e], a[e], accW[j][rb][e]);
            q4_store4<DT>(p, (long long)b * p.sCb + (long long)m * p.sCm + n, v);
        }
    }
}

}  // namespace bd
