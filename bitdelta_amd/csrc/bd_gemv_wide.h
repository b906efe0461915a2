// Decode path, WIDE form: ONE launch per Linear for 17..64 tenants (one activation row each), the base weight streamed ONCE.
//
//   y[t,:] = x[t,:] . W^T + alpha[t, group(n)] * (x[t,:] . S_t)        T <= 64 rows, M == 1, W tile-major (tile_weight, WT = 1)
//
// Reference call site: DiffCompressModule.forward at decode (demo/demo_backend.py:93-98, M = 1, B = tenants) with more tenants than the
// packed streaming kernel's 16 rows; until this kernel such a call ran as ceil(T / 16) consecutive launches, each streaming W again.
//
// Why its own kernel and not another axis of gemv_stream_kernel: that kernel keeps ONE 16 x 16 fp32 accumulator per tenant (its B operand
// holds all <= 16 rows, and tenant t's product is row t of its own accumulator).  64 tenants would need 64 accumulators -- 256 registers.
// Here the tenants are cut in NG = ceil(T / 16) ROW GROUPS of 16 and a group owns exactly two accumulators, whatever its tenant count:
//   * accB[r] += W fragment (A) x activation fragment of rows 16 r .. 16 r + 15 (B): the stream kernel's base MFMA, once per group; the W
//     fragment is loaded from memory once per launch and feeds the NG base MFMAs from registers;
//   * accD[r] += sign fragment of tenant 16 r + j (A) x the SAME activation fragment with every row but j ZEROED (B), j = 0 .. 15: of
//     tenant j's product only row j is ever used, and with the other 15 rows of B zero the product contributes to column j of D alone --
//     so the 16 tenants of a group accumulate into ONE shared accumulator whose column j is tenant j's delta.  2 NG accumulators in all.
//   The zeroing is a SELECT on the four fragment registers (v_cndmask_b32 against the constant lane mask "row == j", kept in an SGPR
//   pair): 4 VALU per sign MFMA.  The alternative -- per-lane load offsets pushed out of the buffer descriptor so that the loads return
//   zero, as the stream kernel's run-ahead loads do -- needs one activation load per (tenant, step): 64 load instructions per group and
//   stage through the texture path instead of 4, which costs more than the matrix pipe saves.
// Work split: grid = N / 16 blocks of 4 waves, block = one 16-column MFMA tile, its waves own contiguous quarters of k (the stream
//   kernel's split); <= 256 registers and 4 + 8 NG KiB of LDS, so two blocks share a CU and one block's ramp hides behind the other's stream.
// Data movement, per (128-k iteration `it`, row group r) SLOT and lane (li = lane & 15, g = lane >> 4; MFMA step s covers
//   k = 128 it + 32 s + 8 g .. + 7 for every operand -- the natural order of the packed layout):
//   * 4 x 16 B of activation row 16 r + li straight from L2 into the B-operand layout (64 rows x K do not fit LDS at K = 4096);
//   * 4 x 16 B = the 16 sign dwords of the group's tenants for (it, g, column li): pack_decode_masks_wide keeps group r byte for byte in
//     pack_decode_masks' t_pad = 16 order, so a lane's 16 tenants are 64 contiguous bytes and every sign dword is loaded once;
//   * with slot (it, 0): the 4 x 16 B of W (one contiguous 4-KiB block per iteration and tile, non-temporal).
//   Slots form a register ring that is refilled right after a slot is consumed: NG U slots (U = 4 / 2 / 1 / 1 iterations for NG = 1 .. 4)
//   and max(U, 2) W fragment sets are in flight per wave.  Every load is a raw buffer load; rows past T, and iterations past the wave's
//   quarter, get an offset with bit 31 set, which is out of range for every descriptor (extents < 2 GiB, host-checked) and returns zero
//   without touching memory -- no branch around a load, hipcc's own vmcnt counting keeps the ring in flight.
//   * sign fragment = the stream kernel's NIBBLE table (16 entries x 8 B x 32 lane copies = 4 KiB, conflict-free), two ds_read_b64 per
//     fragment, read two tenants ahead of their MFMAs.
// End: the 4 waves' 2 NG partial accumulators meet in LDS, wave r sums group r in wave order (deterministic; no atomics, no workspace,
//   no second launch) and stores scale_then_add(delta, alpha, base) [+ residual], rounded once.
// Algorithmic bytes per launch: 2 N K (W) + T N K / 8 (signs) + 2 T K (x, per block: L2) + out.
#pragma once
#include "bd_gemv_stream.h"

namespace bd {

struct WideParams {
    const unsigned short* X;   // [T, K], row stride sXt elements
    const unsigned short* W;   // tile-major [N/16][K/128][4][16][4][8]
    const uint32_t* P;         // [NG][N/16][K/128][4][16][16] dwords
    const float* alpha;        // fp32 [T, G], row stride sAlt
    void* C;                   // [T, N], row stride sCt elements
    int T, N, K, gsz;
    long long sXt, sCt, sAlt;
    int accumulate, out_f32;
    uint32_t x_bytes, w_bytes, p_bytes, pg_bytes;      // descriptor extents; pg_bytes = one row group of P
};

constexpr int WIDE_NW = 4;
constexpr int WIDE_LUT_BYTES = 4096;
constexpr int wide_lds_bytes(int ng) { return WIDE_LUT_BYTES + WIDE_NW * 2 * ng * 64 * 16; }

template <int DT, int NG>
__global__ void __launch_bounds__(64 * WIDE_NW, 2) gemv_wide_kernel(const WideParams p) {
    static_assert(NG >= 1 && NG <= 4, "row groups of 16 tenants, at most 64");
    constexpr int U = NG == 1 ? 4 : NG == 2 ? 2 : 1;      // iterations whose slots are in flight
    constexpr int WU = U < 2 ? 2 : U;                     // W fragment sets in flight = unroll of the main loop
    __shared__ __attribute__((aligned(256))) char lds[wide_lds_bytes(NG)];
    f32x4_t* const red = (f32x4_t*)(lds + WIDE_LUT_BYTES);          // [wave][2 NG accumulators][lane]
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int li = lane & 15, g = lane >> 4;
    const uint32_t tile = (uint32_t)xcd_remap(blockIdx.x, gridDim.x);
    const int nit = p.K >> 7;
    const int per = (nit + WIDE_NW - 1) / WIDE_NW;
    const int it_lo = min(wave * per, nit), it_hi = min(it_lo + per, nit);

    const __amdgpu_buffer_rsrc_t rx = make_rsrc(p.X, p.x_bytes);
    const __amdgpu_buffer_rsrc_t rw = make_rsrc(p.W, p.w_bytes);
    const __amdgpu_buffer_rsrc_t rp = make_rsrc(p.P, p.p_bytes);

    // The epilogue's operands -- scales and residual values of the 4 outputs this lane stores (wave r reduces row group r) -- are the
    // OLDEST loads of the wave: consuming them at the end never waits for a weight load, and there they would be an exposed round trip.
    const int row_out = 16 * wave + li;
    const bool out_ok = wave < NG && row_out < p.T;
    float a_pre[4] = {0.f, 0.f, 0.f, 0.f};
    uint32_t c_pre[4] = {0u, 0u, 0u, 0u};
    if (out_ok) {
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int n = (int)tile * 16 + 4 * g + e;
            a_pre[e] = p.alpha[(long long)row_out * p.sAlt + n / p.gsz];
            if (p.accumulate) {
                const long long off = (long long)row_out * p.sCt + n;
                c_pre[e] = p.out_f32 ? ((const uint32_t*)p.C)[off] : (uint32_t)((const unsigned short*)p.C)[off];
            }
        }
    }

    // per-lane byte offsets that do not depend on the iteration; bit 31 = out of range
    uint32_t x_row[NG];
#pragma unroll
    for (int r = 0; r < NG; ++r)
        x_row[r] = 16 * r + li < p.T ? (uint32_t)((long long)(16 * r + li) * p.sXt * 2) + (uint32_t)g * 16u : STREAM_OOB;
    const uint32_t w_lane = tile * (uint32_t)nit * 4096u + (uint32_t)li * 64u + (uint32_t)g * 16u;
    const uint32_t p_lane = (tile * (uint32_t)nit * 64u + (uint32_t)g * 16u + (uint32_t)li) * 64u;

    struct Slot { u32x4_t xf[4], sg[4]; };
    auto issue = [&](Slot& s, int it, int r) {
        const uint32_t oob = it < it_hi ? 0u : STREAM_OOB;
        const uint32_t xo = (x_row[r] + (uint32_t)it * 256u) | oob;
        const uint32_t po = ((uint32_t)r * p.pg_bytes + p_lane + (uint32_t)it * 4096u) | oob;
#pragma unroll
        for (int q = 0; q < 4; ++q) s.xf[q] = buf_load16<0>(rx, xo + 64u * q);
#pragma unroll
        for (int q = 0; q < 4; ++q) s.sg[q] = buf_load16<0>(rp, po + 16u * q);
        __builtin_amdgcn_sched_barrier(0);       // slots enter the load queue in the order they are consumed
    };
    auto issue_w = [&](u32x4_t (&w)[4], int it) {
        const uint32_t wo = (w_lane + (uint32_t)it * 4096u) | (it < it_hi ? 0u : STREAM_OOB);
#pragma unroll
        for (int q = 0; q < 4; ++q) w[q] = buf_load16<2>(rw, wo + 1024u * q);
        __builtin_amdgcn_sched_barrier(0);
    };

    Slot sl[U * NG];
    u32x4_t wf[WU][4];
#pragma unroll
    for (int u = 0; u < WU; ++u) {
        issue_w(wf[u], it_lo + u);
        if (u < U) {
#pragma unroll
            for (int r = 0; r < NG; ++r) issue(sl[u * NG + r], it_lo + u, r);
        }
    }

    {   // nibble sign table: thread t writes entry t >> 4 for the lane copies 2 (t & 15), 2 (t & 15) + 1 (one ds_write_b128)
        constexpr uint32_t POS = One2<DT>::v & 0xffffu, NEG = POS | 0x8000u;
        const int ee = (int)threadIdx.x >> 4;
        u32x4_t w;
#pragma unroll
        for (int d = 0; d < 2; ++d) w[d] = w[d + 2] = (((ee >> (2 * d)) & 1) ? POS : NEG) | ((((ee >> (2 * d + 1)) & 1) ? POS : NEG) << 16);
        *(u32x4_t*)(lds + threadIdx.x * 16) = w;
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");

    const uint32_t copy8 = (uint32_t)(lane & 31) * 8u;
    auto lut = [&](uint32_t w, int s) -> u32x4_t {      // low nibble of byte s -> sign values 0..3 (dwords 0, 1), high nibble -> 4..7
        const uint32_t lo = (__builtin_amdgcn_ubfe(w, 8u * s, 4u) << 8) | copy8, hi = (__builtin_amdgcn_ubfe(w, 8u * s + 4u, 4u) << 8) | copy8;
        const u32x2_t a = *(const u32x2_t*)(lds + lo), b = *(const u32x2_t*)(lds + hi);
        return u32x4_t{a[0], a[1], b[0], b[1]};
    };

    f32x4_t accB[NG], accD[NG];
#pragma unroll
    for (int r = 0; r < NG; ++r) accB[r] = accD[r] = f32x4_t{0.f, 0.f, 0.f, 0.f};

    // one slot: 4 steps x (1 base MFMA + 16 sign MFMAs).  The sign fragments are read one PAIR of tenants ahead and the pairs are fenced:
    // left alone, hipcc hoists the 128 ds_read_b64 of a slot to its top and the fragments spill.
    auto compute = [&](const Slot& c, const u32x4_t (&w)[4], f32x4_t& aB, f32x4_t& aD) {
        u32x4_t sf[2][2];
        sf[0][0] = lut(c.sg[0][0], 0);
        sf[0][1] = lut(c.sg[0][1], 0);
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            aB = mfma16<DT>(w[s], c.xf[s], aB);
#pragma unroll
            for (int h = 0; h < 8; ++h) {
                const int nx = 8 * s + h + 1;                       // the next pair: (step, tenants 2 h', 2 h' + 1)
                if (nx < 32) {
                    const int s2 = nx >> 3, j2 = 2 * (nx & 7);
                    sf[nx & 1][0] = lut(c.sg[j2 >> 2][j2 & 3], s2);
                    sf[nx & 1][1] = lut(c.sg[(j2 + 1) >> 2][(j2 + 1) & 3], s2);
                }
#pragma unroll
                for (int d = 0; d < 2; ++d) {
                    const bool mine = li == 2 * h + d;              // B operand of tenant 2 h + d: its own row, zeros elsewhere
                    const u32x4_t b = {mine ? c.xf[s][0] : 0u, mine ? c.xf[s][1] : 0u, mine ? c.xf[s][2] : 0u, mine ? c.xf[s][3] : 0u};
                    aD = mfma16<DT>(sf[h & 1][d], b, aD);
                }
                __builtin_amdgcn_sched_barrier(0);
            }
        }
    };

    // Main loop: whole rounds of WU iterations, at least one; a wave with an empty k range (K < 512) walks one all-zero round.  No branch
    // around a load and no exit inside a round (see gemv_stream_kernel's main loop for what either costs).
    int base = it_lo;
    do {
#pragma unroll
        for (int u = 0; u < WU; ++u) {
#pragma unroll
            for (int r = 0; r < NG; ++r) {
                Slot& s = sl[(u % U) * NG + r];
                compute(s, wf[u], accB[r], accD[r]);
                issue(s, base + u + U, r);
            }
            issue_w(wf[u], base + u + WU);
        }
        base += WU;
    } while (base < it_hi);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");     // the run-ahead (out-of-range) loads of the last round

#pragma unroll
    for (int r = 0; r < NG; ++r) {
        red[(wave * 2 * NG + 2 * r) * 64 + lane] = accB[r];
        red[(wave * 2 * NG + 2 * r + 1) * 64 + lane] = accD[r];
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
    if (out_ok) {        // D[col][row]: this lane holds columns 4 g + e of activation row li of group `wave`
        f32x4_t sb = {0.f, 0.f, 0.f, 0.f}, sd = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int w = 0; w < WIDE_NW; ++w) {                  // fixed wave order: deterministic
            sb += red[(w * 2 * NG + 2 * wave) * 64 + lane];
            sd += red[(w * 2 * NG + 2 * wave + 1) * 64 + lane];
        }
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const long long off = (long long)row_out * p.sCt + (int)tile * 16 + 4 * g + e;
            float v = scale_then_add(sd[e], a_pre[e], sb[e]);
            if (p.accumulate) v += p.out_f32 ? __builtin_bit_cast(float, c_pre[e]) : half_bits_to_f32<DT>(c_pre[e]);
            if (p.out_f32) ((float*)p.C)[off] = v;
            else ((unsigned short*)p.C)[off] = (unsigned short)f32_to_half_bits<DT>(v);
        }
    }
}

}  // namespace bd
