/*
 * bitdelta_hip.h -- C ABI of libbitdelta_hip.so: the MI355X (gfx950) implementation of BitDelta's
 * 1-bit-delta Linear hot path.  Plain pointers and sizes only; every pointer is a DEVICE pointer unless
 * noted; `stream` is a hipStream_t passed as void* (NULL = default stream).  All entry points are
 * re-entrant (the reference's serving threads call without locks, demo/demo_backend.py:261): the only state is
 * (a) the bd_set_* test / tuning overrides, which are THREAD-LOCAL (a thread that forces a kernel family does not
 * change what other threads launch), and (b) per-DEVICE caches (CU count, max-dynamic-LDS attribute already
 * raised) keyed by the current HIP device, so one process may drive several GPUs.
 * Return value: 0 on success, a negative BD_E_* code otherwise (bd_error_string() names it); nothing throws.
 *
 * The reference has no FFI of its own: the interface this library replaces is the Python function surface
 * of /root/reference/bitdelta/binary_gemm_kernel.py and bitdelta/diff.py (cited per function below).
 * bitdelta_amd/_lib.py is the ctypes binding; INTEGRATION.md shows the stub a maintainer of the
 * reference would add.
 *
 * dtype codes: 0 = fp16, 1 = bf16, 2 = fp32 (outputs only).  All strides are in ELEMENTS.
 */
#ifndef BITDELTA_HIP_H
#define BITDELTA_HIP_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

#define BD_F16 0
#define BD_BF16 1
#define BD_F32 2

#define BD_OK 0
#define BD_E_K_NOT_MULTIPLE (-1)   /* K % n_bits != 0  (reference assert, binary_gemm_kernel.py:13) */
#define BD_E_BAD_NBITS (-2)        /* n_bits not in {8,16,32,64} (reference: UnboundLocalError, :23-30) */
#define BD_E_BAD_GROUPS (-3)       /* G < 1 or N % G != 0 */
#define BD_E_BAD_DTYPE (-4)
#define BD_E_BAD_SHAPE (-5)        /* negative / overflowing dimension */
#define BD_E_WORKSPACE (-6)        /* workspace missing or too small */
#define BD_WS_TICKET_BYTES 65536    /* leading bytes of a GEMM workspace that must be zero on entry (see bd_delta_bmm) */
#define BD_E_LAUNCH (-7)           /* hipLaunchKernel failed (hipGetLastError has the detail) */
#define BD_E_NULL (-8)

int bd_version(void);
const char* bd_error_string(int code);

/* pack: replaces pack(x, n_bits)  -- bitdelta/binary_gemm_kernel.py:6-32.
 * bits: torch.bool bytes, logical shape [batch, K, N] with element strides (s_b, s_k, s_n) -- the reference packs a
 * transposed view (bitdelta/diff.py:16).  out: contiguous [batch, K/n_bits, N] of uint8/int16/int32/int64. */
int bd_pack(const void* bits, int64_t batch, int64_t K, int64_t N, int64_t s_b, int64_t s_k, int64_t s_n,
            void* out, int n_bits, void* stream);

/* unpack: replaces unpack(x, n_bits) -- bitdelta/binary_gemm_kernel.py:34-46.
 * words: contiguous [batch, KW, N]; out_bits: contiguous torch.bool bytes [batch, KW*n_bits, N]. */
int bd_unpack(const void* words, int64_t batch, int64_t KW, int64_t N, void* out_bits, int n_bits, void* stream);

/* delta GEMM: replaces binary_matmul / binary_bmm -- bitdelta/binary_gemm_kernel.py:153-184, :297-335 (kernels :48-151,
 * :186-295).   C[b] = A[b] . (2*unpack(P[b]) - 1)
 *   A [B,M,K] dtype (k contiguous), P int32 [B or 1, K/32, N] contiguous (sPb = 0 broadcasts one mask: what
 *   bitdelta/diff.py:38 materialises with mask.repeat), C [B,M,N] out_dtype (n contiguous).
 *   round_mode 1 = the reference epilogue fp32 -> fp16 -> out (:143/:287 then :167/:314); 0 = one rounding fp32 -> out.
 *   alpha != NULL: C = alpha[b, g(n)] * acc (accumulate = 0) or C = C_in + alpha[b, g(n)] * acc (accumulate = 1), fp32
 *   math, one rounding -- folds `coeff *` and `+` of bitdelta/diff.py:39 / demo_backend.py:97-98 into the epilogue.
 *   alpha: fp32 [B or 1, G], sAlb = its batch stride (0 = broadcast); G scale groups split N evenly.
 *   ws / ws_bytes: scratch of at least bd_gemm_workspace_bytes(B, M, N, K) bytes (may be NULL when that is 0).
 *     The first BD_WS_TICKET_BYTES bytes are reserved for the arrival counters of the decode path's optional in-launch split-k
 *     reduction (bd_set_decode_two_launch(0)).  ONLY in that mode they must be ZERO when the call is enqueued (hipMemsetAsync the
 *     buffer once after allocating it); the library leaves them zero when the call completes, and a kernel that finds a counter out of
 *     range traps (hipErrorLaunchFailure at the next synchronisation) rather than return wrong sums.  In the default mode (a second,
 *     tiny reduce launch) the workspace needs no initialisation.  Do not share a workspace between concurrently running launches. */
int bd_delta_bmm(const void* A, const int32_t* P, void* C, int B, int M, int N, int K,
                 int64_t sAb, int64_t sAm, int64_t sPb, int64_t sCb, int64_t sCm,
                 int dtype, int out_dtype, int round_mode,
                 const float* alpha, int64_t sAlb, int G, int accumulate,
                 void* ws, int64_t ws_bytes, void* stream);

/* fused 16-bit-base + 1-bit-delta Linear: replaces BinaryDiff.forward (bitdelta/diff.py:33-39) and
 * DiffCompressModule.forward (demo/demo_backend.py:93-98) in ONE launch:
 *   Y[b] = X[b] . W^T + alpha[b, g(n)] * (X[b] . S[b]),  fp32 accumulate, one rounding to out_dtype.
 *   W [N,K] row-major, leading dimension ldw (BinaryDiff.base is its .T view, diff.py:18; nn.Linear.weight as is). */
int bd_binary_linear(const void* X, const void* W, const int32_t* P, const float* alpha, void* Y,
                     int B, int M, int N, int K,
                     int64_t sXb, int64_t sXm, int64_t ldw, int64_t sPb, int64_t sAlb, int G,
                     int64_t sYb, int64_t sYm, int dtype, int out_dtype,
                     void* ws, int64_t ws_bytes, void* stream);

/* decode form of the fused Linear with the sign words repacked for the streaming decode kernel.  The serving side repacks a
 * tenant set's masks once when it registers them (diff.pt and the nn.Module buffers keep the reference layout):
 *   mask_layout 1, TILE-MAJOR:  P int32 [B or 1, ceil(N/16), K/32, 16]: word (i, n) of the reference layout at [n / 16][i][n % 16]
 *     (a 16-column MFMA tile reads its words as one contiguous run over k); sPb = tenant stride in words (0 broadcasts); t_pad unused.
 *   mask_layout 2, PACKED:  P int32 [ceil(N/16), ceil(K/128), 4, 16, t_pad]: element [tile][it][g][c][t] is tenant t's dword whose
 *     byte s holds the 8 signs of k = 128 it + 32 s + 8 g .. + 7 of column 16 tile + c (a 4 x 4 byte transpose of the iteration's 4
 *     word rows), tenants interleaved and zero-padded to t_pad in {1, 2, 4, 6, 8}; B <= t_pad tenants, all in one call (B*M <= 16).
 *     Natural k order for every operand: one activation fragment set, sector-contiguous weight loads, 1-2 wide sign loads per stage.
 *     With this layout the BASE WEIGHT may be the serving side's tile-major decode copy as well: pass ldw = 0 and
 *     W' [N/16][K/128][4 steps s][16 rows c][4 groups g][8] with W'[tile][it][s][c][g][e] = W[16 tile + c][128 it + 32 s + 8 g + e]
 *     (M == 1, N % 16 == 0, K % 128 == 0): one stage of the kernel is then ONE contiguous 4-KiB block (gate+up 28672x4096 for 6
 *     tenants: 68.8 vs 73.0 us).  Same values, same arithmetic: bit-identical to the row-major operand.
 * Columns past N / k past K are zero padding.  Streaming decode kernel only: M <= 16, N >= 512, <= 8 masks, else BD_E_BAD_SHAPE.
 * accumulate = 1 adds onto Y (residual epilogue).  Needs no workspace. */
int bd_binary_linear_decode(const void* X, const void* W, const int32_t* P, int mask_layout, int t_pad, const float* alpha, void* Y,
                            int B, int M, int N, int K,
                            int64_t sXb, int64_t sXm, int64_t ldw, int64_t sPb, int64_t sAlb, int G,
                            int64_t sYb, int64_t sYm, int dtype, int out_dtype, int accumulate, void* stream);

/* PREFILL-size fused gate|up projection with the MLP's activation in its epilogue (M > 16; the decode-size form is
 * bd_binary_linear_decode_fused with epilogue = 1).  W [N, K] / P [B or 1, K/32, N] (reference sign layout) / alpha [B or 1, 2] describe
 * the gate_proj and up_proj BinaryDiff modules of one MLP (the two Linears bitdelta/diff.py:60-64 selects by name `mlp.*proj`) stored
 * as ONE projection whose output rows are interleaved in blocks of 8 ([g0..7 | u0..7 | g8..15 | ...]); Y [B, M, N/2] receives
 *     round(silu(round(gate))) * round(up),   gate / up = X . W^T + alpha * (X . S)  (fp32, one rounding each)
 * i.e. exactly bd_binary_linear followed by bd_srv_swiglu (bit-identical), without the [M, N] round trip through HBM and the second
 * launch.  N % 16 == 0, K % 64 == 0, 16-byte aligned rows; anything else returns BD_E_BAD_SHAPE and the caller runs the two launches. */
int bd_binary_linear_swiglu(const void* X, const void* W, const int32_t* P, const float* alpha, void* Y,
                            int B, int M, int N, int K,
                            int64_t sXb, int64_t sXm, int64_t ldw, int64_t sPb, int64_t sAlb,
                            int64_t sYb, int64_t sYm, int dtype, void* stream);

/* packed-layout decode Linear with the neighbouring glue of a decoder layer FUSED into the launch (bit-identical to the separate
 * launches; what disappears is a ~4 us kernel + a launch gap per fused op, on a step of a few hundred 15-65 us Linears):
 *   norm_w != NULL (optional when epilogue = 1): X is the UN-NORMALISED residual stream; every block computes HF RMSNorm
 *     norm_w[b] * round(X[b,m] * rsqrt(mean(X[b,m]^2) + eps))  for the B*M rows itself while its first weight stages are in flight and
 *     reads its activations from LDS (bd_srv_rmsnorm's arithmetic, same order).  norm_w [B or 1, K], stride s_norm elements.
 *     Needs M == 1 (one new token per tenant), K a power of two >= 2048, B*K <= 32768 and B*(2K+16) bytes of LDS next to the
 *     kernel's 82 KB (8 tenants x 4096, 4 x 8192).
 *   epilogue = 1: SwiGLU.  W / P / alpha describe a fused gate|up projection whose OUTPUT ROWS are interleaved in blocks of 8
 *     ([g0..7 | u0..7 | g8..15 | u8..15 | ...]; G = 2 scale groups: alpha[b][0] gate, alpha[b][1] up); Y [B, M, N/2] receives
 *     round(silu(round(gate))) * round(up)  -- the HF MLP's act_fn(gate_proj(x)) * up_proj(x) (bd_srv_swiglu's arithmetic).
 *     N % 16 == 0, out_dtype == dtype, accumulate = 0.
 * Shapes outside the envelope return BD_E_BAD_SHAPE and the caller runs the separate launches. */
int bd_binary_linear_decode_fused(const void* X, const void* W, const int32_t* P, int t_pad, const float* alpha, void* Y,
                                  int B, int M, int N, int K,
                                  int64_t sXb, int64_t sXm, int64_t ldw, int64_t sPb, int64_t sAlb, int G,
                                  int64_t sYb, int64_t sYm, int dtype, int out_dtype, int accumulate,
                                  const void* norm_w, int64_t s_norm, float eps, int epilogue, void* stream);

/* RMSNorm HAND-OFF between two decode launches of a decoder layer (packed layout, M == 1, B <= 8; new in round 5 -- the reference runs
 * the HF RMSNorm module between its Linears, demo/demo_backend.py:62-79 wraps it per tenant).  bd_binary_linear_decode_fused with three
 * more pointers:
 *   PRODUCER, ssq_out != NULL (the o_proj / down_proj launch: accumulate = 1 or 0, 16-bit output, N % 16 == 0, epilogue = 0): besides Y the
 *     launch writes ssq_out[n / 16][row] = sum over the 16 columns of tile n / 16 of Y[row][n]^2 (fp32 [N/16][16], fixed order).  With
 *     xw_out != NULL, norm_w [B or 1, N] (stride s_norm) is the weight of the RMSNorm that FOLLOWS and xw_out [B, M, N] (Y's strides)
 *     receives round(Y (.) norm_w): the pre-multiplied copy the consumer reads instead of Y.
 *   CONSUMER, ssq_in != NULL (the q|k|v / gate|up launch that follows; K % 16 == 0, K <= 8192, norm_w = NULL): X is the producer's xw_out
 *     -- the consumer reads exactly what the resident-row form reads, nothing to multiply -- and rsqrt(sum(ssq_in[:, row]) / K + eps) scales
 *     the row's accumulators in the epilogue:  Y = rs * (W + alpha S) . (norm_w (.) x)  -- HF RMSNorm followed by the Linear with the row
 *     scale moved across the contraction (one rounding of x * norm_w instead of two; not bit-identical to the separate bd_srv_rmsnorm launch,
 *     same accuracy).
 *   Needs the tile-major base weight (ldw = 0) on the consumer, K >= 1024, B * K <= 32768.  Both stand-alone rmsnorm launches of a layer
 *   disappear without any block re-reducing or re-normalising the rows.  BD_E_BAD_SHAPE outside the envelope (no fallback).
 *
 *   PRODUCER launches (ssq_out != NULL) do not normalise anything: there the `eps` argument is the FACTOR the written sums of squares are
 *   multiplied by (<= 0: 1).  Intended use (round 6): pass norm_w = nw / s with s a power of two >= max |nw| and eps = 1 / s^2, and give the consumer
 *   eps / s^2 -- xw_out = round16(x . nw / s) then never exceeds |x| (no fp16 overflow whatever the norm weight), and the consumer's row scalar
 *   becomes s . rsqrt(mean(x^2) + eps): the same product exactly (bitdelta_amd.serving_loop.handoff_norm). */
int bd_binary_linear_decode_handoff(const void* X, const void* W, const int32_t* P, int t_pad, const float* alpha, void* Y,
                                    int B, int M, int N, int K,
                                    int64_t sXb, int64_t sXm, int64_t ldw, int64_t sPb, int64_t sAlb, int G,
                                    int64_t sYb, int64_t sYm, int dtype, int out_dtype, int accumulate,
                                    const void* norm_w, int64_t s_norm, float eps, int epilogue,
                                    const float* ssq_in, float* ssq_out, void* xw_out, void* stream);

/* The decode Linear with an INT8 base weight (LLM.int8 vector-wise format: CB int8 [N, K] + SCB = per-output-row absmax; the reference
 * dequantises it to fp16 with (CB * SCB[:, None]) / 127 and runs the 16-bit path, bitdelta/misc.py:72-73 -- here the bytes stay in HBM and are
 * widened in registers inside the one launch):
 *     Y[t, n] = round( wscale[n] * sum_k X[t,k] CB[n,k]  +  alpha[t, g(n)] * sum_k X[t,k] S_t[k,n]  [+ Y_in[t, n]] ),   wscale[n] = SCB[n] / 127
 * fp32 accumulation, one rounding; the int8 -> 16-bit widening is exact and the row scale multiplies the finished base sum once, in fp32.
 *   W8: the TILE-MAJOR int8 decode copy (bitdelta_amd.quant.tile_weight_int8), bytes [N/16][K/128][h][16 rows c][4 groups g][j][8] with
 *       W8'[tile][it][h][c][g][j][e] = CB[16 tile + c][128 it + 32 (2 h + j) + 8 g + e]: one (tile, 128-k) stage = one contiguous 2-KiB block;
 *   wscale: fp32 [N], 16-byte aligned.
 * A superset of bd_binary_linear_decode_handoff for that weight form: packed sign layout (t_pad), every argument with the meaning it has there --
 * norm_w / s_norm / eps (RMSNorm prologue, or the producer's next-norm weight and sum factor), epilogue = 1 (SwiGLU), ssq_in / ssq_out / xw_out
 * (hand-off), accumulate, fp32 output; all NULL / 0 for the plain launch.  Envelope: M == 1, N % 16 == 0, K % 128 == 0, N >= 512, and what the
 * tile-major 16-bit weight needs for the same launch kind; anything else -- a row-major int8 weight does not exist -- returns BD_E_BAD_SHAPE.
 * Arguments are validated before any device work. */
int bd_binary_linear_decode_w8(const void* X, const int8_t* W8, const float* wscale, const int32_t* P, int t_pad, const float* alpha, void* Y,
                               int B, int M, int N, int K,
                               int64_t sXb, int64_t sXm, int64_t sPb, int64_t sAlb, int G,
                               int64_t sYb, int64_t sYm, int dtype, int out_dtype, int accumulate,
                               const void* norm_w, int64_t s_norm, float eps, int epilogue,
                               const float* ssq_in, float* ssq_out, void* xw_out, void* stream);

/* The decode Linear with a 4-BIT GPTQ base weight (qweight int32 [K/8, N], qzeros int32 [K/G, N/8], scales fp16 [K/G, N]; no g_idx): the
 * reference dequantises it to fp16 with (q - z) * scale, z = stored nibble + 1, and runs the 16-bit path (bitdelta/misc.py:76-105) -- here the
 * nibbles stay in HBM and are dequantised in registers inside the one launch, bit for bit to the weight Wdq the reference leaves in the model
 * (fp16((q - z) * scale); for bf16 rounded once more):
 *     Y[t, n] = round( sum_k X[t,k] Wdq[n,k]  +  alpha[t, g(n)] * sum_k X[t,k] S_t[k,n]  [+ Y_in[t, n]] )
 * fp32 accumulation, one rounding: the value a tile-major 16-bit launch on Wdq gives.
 *   W4: the TILE-MAJOR nibble decode copy (bitdelta_amd.quant.tile_weight_gptq4), dwords [N/16][K/128][16 rows c][4 groups g][4 steps s] with
 *       W4'[tile][it][c][g][s] = qweight[16 it + 4 s + g][16 tile + c], the 8 nibbles of k = 128 it + 32 s + 8 g + e, stored interleaved:
 *       nibble p of the dword = element e = 2 (p % 4) + p / 4.  One (tile, 128-k) stage = one contiguous 1-KiB block; 16-byte aligned;
 *   qparams: the packed group parameters (bitdelta_amd.quant.pack_gptq4_params), dwords [N/16][K/G][16 rows c]: bits 0..15 the fp16 scale,
 *       bits 16..31 the fp16 number 1024 + z (0x6400 + z, z = 1 .. 16), of column 16 tile + c in that group; 16-byte aligned;
 *   group_size: G, a multiple of 128 that divides K.
 * Otherwise bd_binary_linear_decode_w8's argument list, every argument with the meaning it has there.  Envelope: M == 1, N % 16 == 0,
 * K % 128 == 0, G % 128 == 0, N >= 512, at most 16 tenants, and what the tile-major 16-bit weight needs for the same launch kind; anything
 * else returns BD_E_BAD_SHAPE.  Arguments are validated before any device work. */
int bd_binary_linear_decode_q4(const void* X, const int32_t* W4, const uint32_t* qparams, int group_size, const int32_t* P, int t_pad,
                               const float* alpha, void* Y, int B, int M, int N, int K,
                               int64_t sXb, int64_t sXm, int64_t sPb, int64_t sAlb, int G,
                               int64_t sYb, int64_t sYm, int dtype, int out_dtype, int accumulate,
                               const void* norm_w, int64_t s_norm, float eps, int epilogue,
                               const float* ssq_in, float* ssq_out, void* xw_out, void* stream);

/* the same Linear with the residual connection folded into its epilogue:  Y[b] = Y_in[b] + X[b] . W^T + alpha * (X[b] . S[b])
 * -- the `hidden = residual + o_proj(...)` / `+ down_proj(...)` of the decoder layers that call the reference's modules.
 * Decode shapes (M <= 16, B*M <= 64): fp32 sum, one rounding.  M > 16 on the fused GEMM's fast path (K % 64 == 0, 16-byte aligned
 * rows): the Linear's output is rounded to the output type and the sum is rounded again, i.e. exactly the two roundings of the
 * separate `y = proj(x); hidden = residual + y` (bit-identical to it), one pass over [M, N] less.  Anything else returns
 * BD_E_BAD_SHAPE and the caller adds the residual itself. */
int bd_binary_linear_residual(const void* X, const void* W, const int32_t* P, const float* alpha, void* Y,
                              int B, int M, int N, int K,
                              int64_t sXb, int64_t sXm, int64_t ldw, int64_t sPb, int64_t sAlb, int G,
                              int64_t sYb, int64_t sYm, int dtype, int out_dtype,
                              void* ws, int64_t ws_bytes, void* stream);

/* bd_binary_linear_residual at prefill sizes (M > 16) TOGETHER WITH the RMSNorm that follows it in the decoder layer (round 6):
 *   Y[b] = Y_in[b] + Linear(X[b]);   H[b] = norm_w[b] * round(Y[b] * rsqrt(mean(Y[b]^2) + eps))     (bd_srv_rmsnorm's arithmetic, tenant b's weight)
 * -- `hidden = residual + o_proj(attn); h = post_attention_layernorm(hidden)` (and down_proj + the next layer's input_layernorm) of the HF decoder
 * layers whose Linears are the reference's BinaryDiff modules (bitdelta/diff.py:38-39) and whose norms are DataParallelModule-wrapped
 * (demo/demo_backend.py:62-79).  When the dispatcher splits the Linear over k (several tenants of <= 64 rows: the o / down projections of a
 * short-prompt request) the norm rides on the reduce launch; otherwise it is one norm launch behind the Linear.  Bit-identical to
 * bd_binary_linear_residual followed by bd_srv_rmsnorm either way.  Y, H [B, M, N] dense in M (sYb = M sYm, sHb = M sHm), N % 8 == 0,
 * N <= 8192, 16-byte aligned rows; norm_w [B, N] (stride s_nw; 0 = one weight for all).  Anything else: BD_E_BAD_SHAPE. */
int bd_binary_linear_residual_norm(const void* X, const void* W, const int32_t* P, const float* alpha, void* Y,
                                   int B, int M, int N, int K,
                                   int64_t sXb, int64_t sXm, int64_t ldw, int64_t sPb, int64_t sAlb, int G,
                                   int64_t sYb, int64_t sYm, int dtype,
                                   const void* norm_w, int64_t s_nw, float eps, void* H, int64_t sHb, int64_t sHm,
                                   void* ws, int64_t ws_bytes, void* stream);

/* per-tenant dense Linear at decode: replaces the weight-swapping loop of DataParallelModule.forward
 * (demo/demo_backend.py:62-79) for nn.Linear leaves (lm_head): row block t runs through tenant t's OWN weight matrix,
 *   Y[t] = X[t] . W[t]^T,   X [T, M, K] (strides sXt, sXm), W [T, N, K] (strides sWt, ldw), Y [T, M, N] (strides sYt, sYm),
 * one launch for all tenants (every weight byte streamed once, fp32 accumulate, one rounding).  M <= 16 only (decode);
 * larger M returns BD_E_BAD_SHAPE: that is an ordinary batched GEMM, not this library's business. */
int bd_tenant_linear(const void* X, const void* W, void* Y, int T, int M, int N, int K,
                     int64_t sXt, int64_t sXm, int64_t sWt, int64_t ldw, int64_t sYt, int64_t sYm,
                     int dtype, int out_dtype, void* stream);

/* ---- decode-step glue of the multi-tenant serving loop (callers of the path, demo/demo_backend.py:190-258 + the HF decoder layer
 * between two of the reference's Linears).  Not the hot path: they exist because at decode every stock op is a launch.
 * bd_srv_rmsnorm: Y[r] = Wt[r / rows_per_tenant] * round(X[r] * rsqrt(mean(X[r]^2) + eps))   (HF RMSNorm with per-tenant weights,
 *   the DataParallelModule-wrapped norms of demo_backend.py:62-79); X, Y [rows, H] (strides sx, sy), Wt [tenants, H] (stride sw).
 * bd_srv_swiglu:  Y = round(silu(G)) * U, G / U [rows, I] (row strides sg / su; the fused gate|up output passes U = G + I) -> Y [rows, I];
 *   interleaved8 = 1: G is a [rows, 2I] projection output interleaved in blocks of 8 (see bd_binary_linear_decode_fused), U ignored.
 * bd_srv_decode_attention: one new token per tenant: RoPE of q and the new k (tables cos/sin [Lmax, 128], rotate-half sign folded
 *   into sin), append k/v at *pos to the caches [T, KVH, Lc, 128], mark valid[t, *pos], then softmax(q.K^T/sqrt(128)).V over the
 *   valid keys 0..*pos (left padding = 0 in valid [T, Lc] bytes), grouped-query (H/KVH in {1, 4}); QKV [T, (H+2*KVH)*128] is the
 *   fused q+k+v Linear's output; out [T, H*128].  `pos` is a DEVICE scalar so the step replays inside a hipGraph. */
int bd_srv_rmsnorm(const void* X, const void* Wt, void* Y, int rows, int H, int64_t sx, int64_t sy, int64_t sw,
                   int rows_per_tenant, float eps, int dtype, void* stream);
/* bd_srv_add_rmsnorm (round 6): x_out = round16(resid + round16(y32)); h_out = HF RMSNorm(x_out) with tenant t's weight -- the cast, the residual add
 * and the norm that follow a row-parallel Linear's all-reduce (bitdelta_amd/tp.py) in ONE launch, same roundings as the three ops.  resid / x_out /
 * h_out [rows, H] 16-bit, y32 [rows, H] fp32, row strides in elements; H % 8 == 0, H <= 8192.  No reference counterpart (the reference has no TP). */
int bd_srv_add_rmsnorm(const void* resid, const float* y32, const void* Wt, void* x_out, void* h_out, int rows, int H, int64_t s_r, int64_t s_y,
                       int64_t s_x, int64_t s_h, int64_t sw, int rows_per_tenant, float eps, int dtype, void* stream);
int bd_srv_swiglu(const void* G, const void* U, void* Y, int rows, int I, int64_t sg, int64_t su, int64_t sy, int interleaved8,
                  int dtype, void* stream);
/* bd_srv_rope: in-place rotary embedding of X [rows, heads*128] (row stride sx), position of row r = pos0 + r % seq, tables as for
 * bd_srv_decode_attention; rounds where `torch.addcmul(x * cos, rotate_half(x), sin)` rounds. */
int bd_srv_rope(void* X, const void* cos_t, const void* sin_t, int rows, int heads, int head_dim, int64_t sx, int seq, int pos0,
                int dtype, void* stream);
/* bd_srv_rope_kv_append (round 6): the prefill of a request from position pos0 -- bd_srv_rope on the q and k heads of the fused q|k|v projection
 * output QKV [T * S, (H + 2 KVH) * 128] (row stride sx; in place: bd_srv_prefill_attention reads q / k / v from it), and in the same launch the
 * rotated k rows and the v rows are written to the caches [T, KVH, Lc, 128] at positions pos0 .. pos0 + S - 1 (the `past_key_values` update of
 * the HF attention module the reference's Linears sit in; demo/demo_backend.py:297-315 prefills through it).  pos0 + S <= Lc. */
int bd_srv_rope_kv_append(void* QKV, const void* cos_t, const void* sin_t, void* kcache, void* vcache, int T, int S, int H, int KVH,
                          int head_dim, int64_t sx, int Lc, int pos0, int dtype, void* stream);
/* bd_srv_rope_tab / bd_srv_rope_kv_append_tab: the two entries above with PER-TENANT rotary tables (a fine-tune with its own rope_theta or RoPE
 * scaling; serving_loop.rope_spec).  s_tab is the tenant stride of cos_t / sin_t in elements: 0 = one shared [Lmax, 128] table (then the same
 * launch and the same bits as the entry without the argument, which is this one at s_tab = 0); otherwise the tables are [T, Lmax, 128] and
 * tenant t's rows start at cos_t + t * s_tab.  bd_srv_rope_tab: the tenant of row r is r / seq (X is [T * seq, heads*128]).  Everything else,
 * NULL handling included, as in the originals.  BD_E_BAD_SHAPE, before any device call, when s_tab < 0 or s_tab % 8 != 0 (every tenant's rows stay
 * 16-byte aligned: the kernels read the tables in 16-byte chunks) or a table pointer is not 16-byte aligned. */
int bd_srv_rope_tab(void* X, const void* cos_t, const void* sin_t, int64_t s_tab, int rows, int heads, int head_dim, int64_t sx, int seq, int pos0,
                    int dtype, void* stream);
int bd_srv_rope_kv_append_tab(void* QKV, const void* cos_t, const void* sin_t, int64_t s_tab, void* kcache, void* vcache, int T, int S, int H,
                              int KVH, int head_dim, int64_t sx, int Lc, int pos0, int dtype, void* stream);
/* bd_srv_step_begin / bd_srv_step_end (round 6): the two ends of ONE greedy decode step of the serving loop (demo/demo_backend.py:190-258: HF's
 * generate loop over the tenant batch -- embedding lookup of the last tokens, attention-mask extension, argmax of the last logits, stop-token check).
 * step_begin: X[t] = embed[t][tok[t]] (embed [T, V, H] 16-bit, tenant stride sEt -- 0 = one shared table -- row stride sEv; X [T, H], row stride sx)
 *   and valid[t, *pos] = 1 (valid [T, Lc] bytes: the key mask bd_srv_decode_attention reads).
 * step_end: nxt[t] = argmax(logits[t, :V]) with torch.argmax's order (a NaN is the maximum, ties go to the lower index); tok[t] = nxt[t];
 *   out[t, *step] = nxt[t] when *step < out_cap (out [T, >= out_cap] int64, row stride s_out); stopped[t] |= nxt[t] in stop_ids[t, :ns]; then
 *   *pos += 1 and *step += 1, once (the last block to finish; `ticket` = a zero-initialised 4-byte device word the call leaves at zero).
 * tok / pos / step / out / stop_ids are int64 (torch.long), valid / stopped bytes (torch.bool): the state the loop keeps on the device so that the
 * step replays inside a hipGraph.  V % 8 == 0, H % 8 == 0.  Integer work: exact. */
int bd_srv_step_begin(const void* embed, int64_t sEt, int64_t sEv, const int64_t* tok, void* X, int64_t sx, void* valid, int Lc,
                      const int64_t* pos, int T, int V, int H, void* stream);
int bd_srv_step_end(const void* logits, int64_t sl, int V, int64_t* tok, int64_t* out, int64_t s_out, int out_cap,
                    const int64_t* stop_ids, int ns, void* stopped, int64_t* pos, int64_t* step, void* ticket, int T, int dtype, void* stream);
/* bd_srv_step_begin_ragged / bd_srv_step_end_ragged: the same two ends with PER-TENANT state, so that a tenant is admitted while the others are
 * mid-generation and retires at its own stop token (serving_loop.TenantSession).  pos / n / limit are int64 [T], active / done bytes [T].
 * step_begin_ragged: tenant t is LIVE when active[t] != 0 and 0 <= pos[t] < Lc.  Live: X[t] = embed[t][clamp(tok[t], 0, V - 1)] and
 *   valid[t, pos[t]] = 1.  Not live: X[t] = 0 (a zero row stays finite through RMSNorm and every Linear) and valid is not touched.  The range
 *   guard is part of the contract: pos advances on the device without the host seeing it.
 * step_end_ragged: one block per tenant, no ticket, no shared counter.  active[t] == 0: nothing of tenant t is read or written.  Otherwise, in
 *   this order: nxt = argmax(logits[t, :V]) (torch.argmax's order, as step_end); tok[t] = nxt; out[t, n[t]] = nxt when 0 <= n[t] < out_cap (out
 *   [T, >= out_cap] int64, row stride s_out); n[t] += 1; pos[t] += 1; reason = (nxt in stop_ids[t, :ns] ? 1 : 0) | (n[t] >= limit[t] ? 2 : 0) |
 *   (pos[t] >= Lc ? 4 : 0); when reason != 0: active[t] = 0 and done[t] = reason.  done is written only then.  V % 8 == 0, sl % 8 == 0.  Exact. */
int bd_srv_step_begin_ragged(const void* embed, int64_t sEt, int64_t sEv, const int64_t* tok, void* X, int64_t sx, void* valid, int Lc,
                             const int64_t* pos, const void* active, int T, int V, int H, void* stream);
int bd_srv_step_end_ragged(const void* logits, int64_t sl, int V, int64_t* tok, int64_t* out, int64_t s_out, int out_cap,
                           const int64_t* stop_ids, int ns, int64_t* pos, int64_t* n, const int64_t* limit, void* active, void* done, int Lc, int T,
                           int dtype, void* stream);
/* bd_srv_sample_rows / bd_srv_step_end_sample: a token chosen by temperature, top-k, top-p and a seed instead of argmax.  The token of a logits
 * row is a PURE FUNCTION of the row and (tau, top_k, top_p, seed, d): it does not depend on the other rows of the launch, on graph or eager
 * execution, or on thread order (every sum that decides a threshold is an integer sum; no floating-point atomics).  The definition:
 *   Greedy: tau == 0 gives the token of bd_srv_step_end_ragged (torch.argmax's order).  A row that holds a NaN or +inf, or nothing finite, gives
 *     that token whatever tau is.  -inf logits have weight 0 and are never sampled.  The token is always in [0, V).
 *   Filters, in the order of HF's warpers (temperature, top-k, top-p), both on logit VALUES so that ties stay together (-0 == +0):
 *     top-k (1 <= top_k < V): keep every token whose logit is >= the k-th largest logit (TopKLogitsWarper's `scores < topk(scores, k)[..., -1]`).
 *     top-p (0 < top_p < 1): with w_i = exp((l_i - m) / tau) over the top-k survivors (m = the row's maximum) and Z = sum w_i, keep token i iff
 *       sum_{l_j > l_i} w_j / Z < top_p -- the smallest set of highest values whose mass reaches top_p, all ties of the boundary value kept, at
 *       least one token kept.  (TopPLogitsWarper keeps a sort-order-dependent subset of EQUAL boundary logits; this keeps all of them.)  The
 *       masses are fp32 (hardware exp2) summed in 2^-40 fixed point: a row whose cumulative ratio lies within ~1e-5 of top_p may land on either
 *       adjacent value.
 *   Draw: Gumbel-max.  Philox4x32-10 with key = (seed & 0xffffffff, seed >> 32) and counter = (i >> 2, 0, d & 0xffffffff, d >> 32); token i takes
 *     output word r = word[i & 3]; u = ((r >> 8) + 0.5) * 2^-24; score_i = l_i / tau - log(-log u) in fp32 (-log u keeps its RELATIVE accuracy up to
 *     u -> 1, where it is ~2^-25: from u = 1/2 on it is a series in the exact 1 - u); the token is the argmax of score_i over the kept set, ties to the lower index.
 *   d is the draw index: the cache row the new token will occupy (bd_srv_step_end_sample: d = pos[t] + 1), so no two tokens of a conversation
 *     share their draws; a caller who wants fresh randomness passes a new seed.
 * Parameter VALUES are device data the host never sees.  The kernel neutralises what is out of range: tau < 0, NaN or +inf -> greedy;
 *   top_k < 1 or >= V -> top-k off; top_p <= 0, >= 1 or NaN -> top-p off.
 * bd_srv_sample_rows: R independent rows (logits [R, V] 16-bit, row stride sl), temperature / top_p float32 [R], top_k int32 [R], seed / draw
 *   int64 [R] (the 64 bits of the seed; d), tok int64 [R] <- the tokens.  Nothing else is written.
 * bd_srv_step_end_sample: bd_srv_step_end_ragged -- same state, same order of updates, same reasons, inactive tenants touch nothing -- with the
 *   token chosen as above from temperature / top_k / top_p / seed [T] and d = pos[t] + 1.
 * dbg (NULL in production): int32 [R or T, 4] <- the number of kept tokens, the 16-bit pattern of the smallest kept logit value (+0 for a zero),
 *   the chosen token's Philox word r, flags (1 = the greedy rule decided -- the first three are then 0 --, 2 = top-k active, 4 = top-p active,
 *   8 = the row held a NaN or +inf or nothing finite).  Rows of inactive tenants are not written.
 * V % 8 == 0, sl % 8 == 0, sl >= V, logits 16-byte aligned, the parameter arrays naturally aligned; R == 0 / T == 0 is BD_OK and launches nothing.
 * One 256-thread block per row; the row is read from global memory once per pass (argmax; two per active filter; the draw), any V. */
int bd_srv_sample_rows(const void* logits, int64_t sl, int V, const float* temperature, const int32_t* top_k, const float* top_p,
                       const int64_t* seed, const int64_t* draw, int64_t* tok, int32_t* dbg, int R, int dtype, void* stream);
int bd_srv_step_end_sample(const void* logits, int64_t sl, int V, int64_t* tok, int64_t* out, int64_t s_out, int out_cap,
                           const int64_t* stop_ids, int ns, int64_t* pos, int64_t* n, const int64_t* limit, void* active, void* done, int Lc,
                           const float* temperature, const int32_t* top_k, const float* top_p, const int64_t* seed, int32_t* dbg, int T,
                           int dtype, void* stream);
/* bd_srv_token_nll: the tail of scoring (the reference's eval_ppl.py): each row of 16-bit logits and its label become the token's negative
 * log-likelihood, nll[r] = -log softmax(logits[r, :V])[labels[r]], and optionally the row's log-sum-exp.  The definition, with l the row's V
 * values, m = max_i l_i and S = sum_i exp(l_i - m):
 *     lse[r] = m + ln S            nll[r] = ln S - (l_label - m)
 *   Labels: a label outside [0, V) is IGNORED (-100 is the reference's ignore value): nll[r] is then exactly 0.0f; lse[r] is written all the same.
 *   Non-finite rows: a row that holds a NaN or a +inf, or nothing finite, gives lse = NaN and nll = NaN (torch.log_softmax's answer) unless the
 *     label is ignored.  -inf logits next to finite ones have weight 0; a label that sits on one gives nll = +inf, and lse stays finite.
 *   A value is a PURE FUNCTION of its row and label: it does not depend on R, on the row's index, on sl, on the other rows, or on graph or eager
 *     execution.  The masses exp(l_i - m) are fp32 (hardware exp2), added eight at a time (one aligned 16-byte vector, pairwise, inside one
 *     thread) and from there on in 2^-40 fixed point: every cross-thread sum is an integer sum.  No floating-point atomics.  ln S and the two
 *     final sums are fp64, rounded once to fp32.
 *   Accuracy: |nll - exact| <= 2^-19 (1 + |exact|), and the same for lse.  The two terms of nll are both >= 0, so nothing cancels; l - m is exact
 *     in fp32 for fp16 and correct to an fp32 ulp for bf16; a mass carries <= 2^-24 (|l_i - m| + 3) relative error and, weighted by the softmax,
 *     sum_i p_i (m - l_i) <= ln V, so ln S is off by at most 2^-24 (ln V + 6) + V 2^-43 (1.0e-6 at V = 32000); the result's rounding adds 2^-24
 *     relative.  tests/nll_ref.py restates the definition in fp64.
 * logits [R, V] fp16 / bf16 with row stride sl (elements); labels int64 [R]; nll fp32 [R]; lse fp32 [R] or NULL.  Any 1 <= V <= 2^22 (a resized
 * vocabulary such as 32001 included: the tail that is not a multiple of 8 is masked inside the kernel); elements V .. sl - 1 of a row may hold
 * anything and never reach a result.  Checked before any device call: R == 0 -> BD_OK, nothing launched; R < 0, V < 1, V > 2^22 (the integer
 * sum's headroom), sl < V, sl % 8 != 0, logits not 16-byte aligned, nll / lse not 4-byte or labels not 8-byte aligned -> BD_E_BAD_SHAPE; logits,
 * labels or nll NULL -> BD_E_NULL; dtype not fp16 / bf16 -> BD_E_BAD_DTYPE.  One 256-thread block per row; up to V = 32768 the row is read from
 * global memory exactly once and held in registers, a longer row twice. */
int bd_srv_token_nll(const void* logits, int64_t sl, int V, const int64_t* labels, float* nll, float* lse, int R, int dtype, void* stream);
/* bd_srv_token_logprobs: what a serving API reports next to a generated token (OpenAI's logprobs / top_logprobs, vLLM's logprobs=): each row of
 * 16-bit logits, a token y and a count top_n become the token's log-probability and the top_n most probable tokens with theirs.  The
 * distribution is softmax(row) at temperature 1, before any top-k / top-p filter: the model's own, whatever the request sampled with.
 *   m, S    exactly bd_srv_token_nll's: m = max_i l_i; per ALIGNED 8-vector the masses exp(l_i - m) summed pairwise in fp32 in a fixed order, the
 *           vector's sum truncated to 2^-40 fixed point; S the INTEGER sum of those words; ln S = log(double(S) * 2^-40) in fp64 on one thread.
 *   lp(i)   = float((double(l_i) - double(m)) - ln S): the float negation of bd_srv_token_nll's value on the same row and label (both sums are
 *           the same fp64 operations with the signs turned), -0 and +0 being one float.
 *   lp[r]   = lp(tok[r]); a token outside [0, V) gives NaN (a chosen token is never out of range: a NaN there shows the caller's error).
 *   top_id[r, 0 .. top_n)   the indices of the top_n largest logit VALUES in descending order; equal values -- -0 and +0 are one value -- in
 *           ascending index order.  The order is that of (key descending, index ascending) with the monotone 16-bit key of the sampling rule.
 *   top_lp[r, j] = lp(top_id[r, j]).
 *   -inf    has lp = -inf and enters the list only when fewer than top_n values are finite, and then in index order (the same tie rule).
 *   A row that holds a NaN or a +inf, or nothing finite: lp = NaN, every top_lp = NaN, every top_id = -1.
 *   Every output is a pure function of (row, y, top_n): not of R, the row's index, sl, graph or eager execution, or thread order.  No
 *   floating-point atomics; every cross-thread count or sum that decides a result is an integer.
 *   Accuracy: bd_srv_token_nll's clause -- every finite lp / top_lp is within 2^-19 (1 + |exact|) of the exact log softmax; the ids are exact.
 *   tests/logprobs_ref.py restates the definition in fp64.
 * logits [R, V] fp16 / bf16 with row stride sl (elements); tok int64 [R]; lp fp32 [R]; top_id int32 and top_lp fp32 [R, top_n], contiguous, or
 * NULL when top_n == 0 (then only lp is computed).  V % 8 == 0, 8 <= V <= 2^22; elements V .. sl - 1 of a row may hold anything and never reach
 * a result.  Checked before any device call: R == 0 -> BD_OK, nothing launched; top_n outside 0 .. 20, top_n > V, V % 8 != 0, sl % 8 != 0,
 * sl < V, V > 2^22, R < 0, logits not 16-byte, tok not 8-byte or an output not 4-byte aligned -> BD_E_BAD_SHAPE; a needed pointer NULL ->
 * BD_E_NULL; dtype not fp16 / bf16 -> BD_E_BAD_DTYPE.  One 256-thread block per row; up to V = 32768 the row is read once and held in registers. */
int bd_srv_token_logprobs(const void* logits, int64_t sl, int V, const int64_t* tok, float* lp, int32_t* top_id, float* top_lp, int top_n,
                          int R, int dtype, void* stream);
/* bd_srv_step_logprobs: bd_srv_token_logprobs at the end of a ragged decode step, launched AFTER bd_srv_step_end_ragged / bd_srv_step_end_sample
 * on the same logits [T, V].  tok int64 [T] is the token the step end has just stored; n int64 [T] its per-tenant token count; lp_n int64 [T]
 * this launch's own counter; lp fp32 [T, cap]; top_id int32 / top_lp fp32 [T, cap, top_n] (NULL when top_n == 0).  Tenant t with
 * n[t] == lp_n[t] emitted nothing in this step: nothing of it is read or written.  Otherwise, with j = n[t] - 1: when 0 <= j < cap entry [t, j]
 * is written from row t and tok[t] by the rule above; in either case lp_n[t] = n[t].  The launch reads no activity flag: a tenant that retired
 * in this step still gets its last token's entry, an inactive one is not touched.  Checks as above with T for R; n or lp_n NULL -> BD_E_NULL,
 * not 8-byte aligned or cap < 0 -> BD_E_BAD_SHAPE. */
int bd_srv_step_logprobs(const void* logits, int64_t sl, int V, const int64_t* tok, const int64_t* n, int64_t* lp_n, float* lp, int32_t* top_id,
                         float* top_lp, int cap, int top_n, int T, int dtype, void* stream);
/* bd_srv_penalize_rows: the controls a serving API carries next to temperature / top-k / top-p (HF's repetition_penalty, OpenAI's
 * presence_penalty / frequency_penalty / logit_bias, vLLM's SamplingParams): each row of 16-bit logits, the row's token history, four floats
 * and a short bias list become the penalised row in the logits' dtype, which the token choice (argmax, bd_srv_sample_rows, the step-end
 * launches) then reads in place of the raw one.
 *   hist[v] (int16, read as raw bits): bit 15 = token v occurs in the context of this turn (the real prompt tokens, never the left pads; after
 *           an extension everything the conversation held before the turn plus the new chunk); bits 0 .. 14 = c, the number of times v has been
 *           generated and fed back in THIS turn, saturating at 32767.  seen = hist[v] != 0.
 *   pen     = (r, r_inv, presence, frequency), r_inv = float(1.0 / r) computed by the host in fp64: the kernel never divides.
 *   bias    nb pairs (bias_id[j], bias_val[j]); an empty slot holds id -1.
 * For every v in [0, V), in fp32, every operation rounded on its own (no fma contraction):
 *   x = float(l[v])
 *   if seen and 0 < r < inf:   x = (x > 0) ? x * r_inv : x * r             (HF's RepetitionPenaltyLogitsProcessor, with the host's reciprocal)
 *   x = x - frequency * float(c)                                            (one product, one subtraction)
 *   if c > 0:                  x = x - presence
 *   for j = 0 .. nb - 1, in list order:   if bias_id[j] == v:  x = x + bias_val[j]      (a repeated id is added twice; -inf bans the token)
 *   out[v] = x rounded to nearest even to the logits' dtype
 * The 16-bit rounding is the loss HF takes when its processors penalise logits held in the model's dtype; the token choice reads 16-bit rows.
 * Device values the host could not have written are neutralised (bd_srv_sample_rows' rule): r that is not in (0, inf), a NaN included, turns
 * the repetition step off; a NaN presence / frequency counts as 0; a bias_id outside [0, V) matches nothing.
 * Neutral parameters (r = 1, presence = frequency = 0, nb = 0) reproduce the input bits: x * 1, x - 0 * c and x - 0 are exact and keep -0,
 * +-inf and subnormals (a NaN stays a NaN).  An out element is a pure function of (l[v], hist[v], pen, bias list): no atomics, nothing depends
 * on thread or block order, on R, on the strides, or on graph or eager execution.  tests/penalty_ref.py restates the definition.
 * logits / out [R, V] fp16 / bf16 with row strides sl / so, hist int16 [R, V] with row stride sh (elements); pen fp32 [R, 4]; bias_id int32 and
 * bias_val fp32 [R, nb], contiguous, NULL allowed only when nb == 0.  Elements V .. stride - 1 of a row are neither read nor written.  Every
 * row is live and hist is only read.  Checked before any device call, in this order: R < 0, V < 1, V > 2^22 -> BD_E_BAD_SHAPE; dtype not fp16 /
 * bf16 -> BD_E_BAD_DTYPE; R == 0 -> BD_OK, nothing launched; nb outside 0 .. BD_LOGIT_BIAS_MAX or R > 65535 -> BD_E_BAD_SHAPE; a needed pointer
 * NULL -> BD_E_NULL; V % 8, a stride % 8 or < V, logits / out / hist / pen not 16-byte or a bias array not 4-byte aligned -> BD_E_BAD_SHAPE.
 * Several blocks per row: grid (ceil(V / 2048), R), one 16-byte vector of logits and of hist per thread, no LDS, no barrier. */
#define BD_LOGIT_BIAS_MAX 64
int bd_srv_penalize_rows(const void* logits, int64_t sl, int V, void* out, int64_t so, const int16_t* hist, int64_t sh, const float* pen,
                         const int32_t* bias_id, const float* bias_val, int nb, int R, int dtype, void* stream);
/* bd_srv_step_penalize: bd_srv_penalize_rows inside a ragged decode step, between the lm_head and bd_srv_step_end_ragged /
 * bd_srv_step_end_sample (which then read `out`), and it COUNTS: tok int64 [T] is the token generated last and fed in this step, active bytes
 * [T].  For an active tenant t the element v == tok[t] is first counted -- c = min(count(hist[t, v]) + 1, 32767), and it is seen -- and the
 * rule above runs with that c; the thread that owns the element stores the new hist[t, v] (bit 15 kept) with one 2-byte store.  No other
 * element of hist is written; a tok[t] outside [0, V) counts nothing.  So a turn's first token is counted by the turn's first step and the last
 * token a tenant emits is never counted.  An inactive tenant's hist row and out row are not touched, nothing of it is read.  out[t, v] is a pure
 * function of (l[v], hist[v], tok[t] == v, pen, bias list).  Checks as above with T for R; tok or active NULL -> BD_E_NULL, tok not 8-byte
 * aligned -> BD_E_BAD_SHAPE. */
int bd_srv_step_penalize(const void* logits, int64_t sl, int V, void* out, int64_t so, int16_t* hist, int64_t sh, const int64_t* tok,
                         const uint8_t* active, const float* pen, const int32_t* bias_id, const float* bias_val, int nb, int T, int dtype,
                         void* stream);
/* bd_srv_constrain_rows: a request's output restricted to a deterministic automaton over token ids (vLLM's guided_choice / guided_regex /
 * allowed_token_ids, OpenAI's structured outputs; a regex or schema compiler outside this library produces the automaton): each row of 16-bit
 * logits becomes the row with every token its state does not allow set to -inf, which the token choice (argmax, bd_srv_sample_rows, the
 * step-end launches) then reads in place of the raw or penalised one.  The automaton is per row, in CSR form:
 *   state[r]     int32: the row's current state, 0 <= state < S; a negative value = no constraint.
 *   off          int32 [R, S + 1]: the edges of state s of row r are off[r, s] .. off[r, s + 1] - 1.
 *   edge_tok     int32 [R, E]: the edges' tokens; within a state sorted ascending, no token twice.
 *   accepting    bytes [R, S]: in an accepting state the request's own stop ids are allowed next to the state's edges.
 *   stop_ids     int64 [R, ns]: the request's stop ids, -1 = an empty slot.
 * For every v in [0, V):
 *   out[v] = l[v], the same 16 bits, when state[r] < 0, or v is an edge token of state[r], or state[r] is accepting and v == stop_ids[r, j] for
 *            some j (a stop id >= 0);
 *   out[v] = -inf otherwise.
 * A kept element keeps its bits: -0, subnormals, NaN and +-inf pass through (no float is made of a logit).  Device values the host could not
 * have written are neutralised: a state >= S masks nothing (as a negative one), slice bounds are clamped into [0, E] (off[s + 1] < off[s]: an
 * empty slice), an edge token outside [0, V) matches nothing.  An out element is a pure function of (l[v], v, the state's edge list, the
 * accepting byte, the stop list): no atomics, nothing depends on R, on the strides, on thread or block order, or on graph or eager execution.
 * tests/constraint_ref.py restates the definition.
 * logits / out [R, V] fp16 / bf16 with row strides sl / so (elements); elements V .. stride - 1 of a row are neither read nor written.  The
 * automaton arrays are contiguous.  edge_tok may be NULL when E == 0, stop_ids when ns == 0.  Checked before any device call, in this order:
 * R < 0, V < 1, V > 2^22 -> BD_E_BAD_SHAPE; dtype not fp16 / bf16 -> BD_E_BAD_DTYPE; R == 0 -> BD_OK, nothing launched; S outside
 * 1 .. BD_CONSTRAINT_STATES_MAX, E outside 0 .. BD_CONSTRAINT_EDGES_MAX, ns outside 0 .. BD_CONSTRAINT_STOP_MAX or R > 65535 ->
 * BD_E_BAD_SHAPE; a needed pointer NULL -> BD_E_NULL; V % 8, a stride % 8 or < V, logits / out not 16-byte, state / off / edge_tok not 4-byte
 * or stop_ids not 8-byte aligned -> BD_E_BAD_SHAPE.
 * Several blocks per row: grid (ceil(V / 2048), R), one 16-byte vector of logits per thread; membership is a lower-bound search of the
 * vector's first index in the state's sorted slice and at most 8 comparisons from there, never a pass over the whole edge list.  No LDS. */
#define BD_CONSTRAINT_STATES_MAX 65536
#define BD_CONSTRAINT_EDGES_MAX 1048576
#define BD_CONSTRAINT_STOP_MAX 64
int bd_srv_constrain_rows(const void* logits, int64_t sl, int V, void* out, int64_t so, const int32_t* state, const int32_t* off,
                          const int32_t* edge_tok, const uint8_t* accepting, int S, int E, const int64_t* stop_ids, int ns, int R, int dtype,
                          void* stream);
/* bd_srv_step_constrain: bd_srv_constrain_rows inside a ragged decode step, between the lm_head (or bd_srv_step_penalize) and
 * bd_srv_step_end_ragged / bd_srv_step_end_sample (which then read `out`); active bytes [T].  An inactive tenant's out row is not touched and
 * nothing of it is read.  The launch only READS state: several blocks share a row, and the state moves in bd_srv_step_constrain_advance, behind
 * the step end.  Checks as above with T for R; active NULL -> BD_E_NULL. */
int bd_srv_step_constrain(const void* logits, int64_t sl, int V, void* out, int64_t so, const int32_t* state, const int32_t* off,
                          const int32_t* edge_tok, const uint8_t* accepting, int S, int E, const int64_t* stop_ids, int ns,
                          const uint8_t* active, int T, int dtype, void* stream);
/* bd_srv_step_constrain_advance: the automaton's transition, launched BEHIND the step end (and bd_srv_step_logprobs) with the token the step
 * chose: one block, one thread per tenant, bd_srv_step_logprobs' counter discipline.  tok / n int64 [T] (the step end's), c_n int64 [T] the
 * launch's own counter, state int32 [T], off / edge_tok / accepting as above, edge_next int32 [T, E] the edges' target states, active / done
 * bytes [T] (the step end's).  For every tenant t:
 *   n[t] == c_n[t]: the tenant emitted nothing in this step; nothing of it is read further or written.
 *   otherwise c_n[t] = n[t]; with s = state[t] in [0, S) (any other value: nothing more happens) and y = tok[t]:
 *     y is an edge token of s and that edge's edge_next lies in [0, S): state[t] = edge_next.  Otherwise the state stays -- a stop id in an
 *     accepting state (the step end has retired the tenant already), or device values the host could not have written: the rule is total.
 *     The state after that is FINAL when it is accepting and has no edges; then, when active[t] != 0: active[t] = 0 and done[t] |= 8 (the
 *     constraint is complete; the reasons 1 / 2 / 4 of bd_srv_step_end_ragged keep their meaning).  A tenant the step end has retired in this
 *     step has its state advanced and its done byte left alone.
 * Integer work: exact.  Checked before any device call, in this order: T < 0 -> BD_E_BAD_SHAPE; T == 0 -> BD_OK, nothing launched; S or E out of
 * range (as above) or T > 1024 -> BD_E_BAD_SHAPE; a needed pointer NULL (edge_tok / edge_next only when E > 0) -> BD_E_NULL; tok / n / c_n not
 * 8-byte, state / off / edge_tok / edge_next not 4-byte aligned -> BD_E_BAD_SHAPE. */
int bd_srv_step_constrain_advance(const int64_t* tok, const int64_t* n, int64_t* c_n, int32_t* state, const int32_t* off,
                                  const int32_t* edge_tok, const int32_t* edge_next, const uint8_t* accepting, int S, int E, uint8_t* active,
                                  uint8_t* done, int T, void* stream);
/* bd_srv_step_stop_sequences: a request stopped at a token SEQUENCE (OpenAI's `stop`, vLLM's `stop` / `include_stop_str_in_output`), and the
 * number of trailing tokens a streaming caller must hold back because they may still become one.  Matching is on token ids: the caller turns a
 * stop string into the one or several token sequences that spell it and passes them all.  Launched LAST in a ragged decode step, behind the step
 * end, bd_srv_step_logprobs and bd_srv_step_constrain_advance (which sets its reason only on a still-active tenant), one block per tenant,
 * bd_srv_step_logprobs' counter discipline with the launch's own counter ss_n.
 *   out      int64 [T, out_cap] with row stride s_out (elements): the step end's output rows; out[t, 0:n] are this turn's tokens.
 *   n        int64 [T]: the step end's per-tenant token count.          ss_n  int64 [T]: this launch's own counter.
 *   seq_tok  int32 [T, Q, W]: tenant t's stop sequences, sequence q in seq_tok[t, q, 0:seq_len[t, q]]; the rest of a row is not compared.
 *   seq_len  int32 [T, Q]: 1 .. W; 0 = an unused slot.
 *   hit / hold int32 [T]; active / done bytes [T] (the step end's).
 * A request carries up to Q <= BD_STOP_SEQ_MAX sequences of 1 .. W <= BD_STOP_SEQ_LEN_MAX ids each.  For every tenant t:
 *   n[t] == ss_n[t]: the tenant emitted nothing in this step; nothing of it is read further or written (a stale hit stays).
 *   otherwise ss_n[t] = n[t], and with n = n[t], y = out[t, 0:n] and len_q = seq_len[t, q], seq_q = seq_tok[t, q, 0:len_q]:
 *     The prompt and earlier turns never take part: only y is compared, so a sequence half in the prompt and half generated does not match.
 *     hit[t]  = the lowest q with 1 <= len_q <= n and y[n - len_q : n] == seq_q; -1 when there is none.
 *     hold[t] = the largest k such that some q has k < len_q, k <= n and y[n - k : n] == seq_q[0:k]; 0 when there is none, and 0 when
 *               hit[t] >= 0.  It is the number of trailing tokens that are a proper prefix of a stop sequence: not to be shown yet.
 *     On a hit: active[t] = 0 and done[t] |= 16.  Unlike reason 8, the bit is also OR-ed into the byte of a tenant the step end has retired
 *     in this same step (reasons 1 / 2 / 4): a caller who trims the matched tokens needs to know of the match even when max_new_tokens ran
 *     out on the same token.
 *     n > out_cap (or n < 0): nothing can be compared -- hit[t] = -1, hold[t] = 0, no element of `out` is addressed.
 *   The rule is total on any device values: a seq_len outside 0 .. W counts as 0 (unused); a negative table entry matches nothing, and so
 *   does an element of `out` that is not a non-negative int32.
 * Integer work: exact, a pure function of (out[t, 0:n], n, the tenant's table), whatever T, the strides, thread order, graph or eager execution.
 * tests/stop_seq_ref.py restates the definition.
 * Checked before any device call, in this order: T < 0, T > 65535, Q outside 1 .. BD_STOP_SEQ_MAX, W outside 1 .. BD_STOP_SEQ_LEN_MAX,
 * out_cap < 0 or s_out < out_cap -> BD_E_BAD_SHAPE; T == 0 -> BD_OK, nothing launched; a pointer NULL -> BD_E_NULL; out / n / ss_n not 8-byte,
 * seq_tok / seq_len / hit / hold not 4-byte aligned -> BD_E_BAD_SHAPE.
 * One thread per (sequence, length) pair; the window of the last W tokens, the table row and the lengths are read once and staged in LDS.  No
 * atomics, no floating point. */
#define BD_STOP_SEQ_MAX 16
#define BD_STOP_SEQ_LEN_MAX 32
int bd_srv_step_stop_sequences(const int64_t* out, int64_t s_out, int out_cap, const int64_t* n, int64_t* ss_n, const int32_t* seq_tok,
                               const int32_t* seq_len, int Q, int W, int32_t* hit, int32_t* hold, uint8_t* active, uint8_t* done, int T,
                               void* stream);
/* bd_srv_ban_rows: the hard bans that depend on what a request has already written -- Hugging Face's NoRepeatNGramLogitsProcessor
 * (no_repeat_ngram_size), NoBadWordsLogitsProcessor (bad_words_ids; vLLM's bad_words) and MinNewTokensLengthLogitsProcessor (min_new_tokens)
 * -- as one masked copy of the row.  Per row r:
 *   ctx        int32 [R, Lc], ctx_len int32 [R]: the conversation's real tokens before this turn (a prompt without its left pads; on a later
 *              turn everything before it, the earlier turns' emitted tokens included).
 *   toks       int64 [R, tok_cap] with row stride s_tok (elements), n int64 [R]: this turn's emitted tokens toks[r, 0:n[r]] (the step end's `out`
 *              and `n`).  n == NULL means no token yet, n = 0 for every row (admission); toks is then not read and may be NULL.
 *   ban_ngram  int32 [R]: the no-repeat n-gram size g, 1 .. BD_BAN_NGRAM_MAX; 0 = off.
 *   ban_tok    int32 [R, Q, W], ban_len int32 [R, Q]: the bad words, sequence q in ban_tok[r, q, 0:ban_len[r, q]]; a length 0 = an unused slot.
 *   ban_min    int32 [R]: the turn's minimum length (min_new_tokens).
 *   stop_ids   int64 [R, ns]: the request's stop ids, -1 = an empty slot.
 * The history is h[0:m) = ctx[r, 0:ctx_len[r]] followed by toks[r, 0:n[r]], m = ctx_len[r] + n[r].  Token v in [0, V) is BANNED when
 *   n-gram:     g >= 1, m >= g - 1, and some i with 0 <= i <= m - g has h[i : i + g - 1] == h[m - g + 1 : m] and h[i + g - 1] == v (the last
 *               g - 1 tokens occurred before, followed by v; with g == 1 every token of the history is banned); or
 *   bad word:   some q with L = ban_len[r, q] has ban_tok[r, q, L - 1] == v and either L == 1, or L > 1, m >= L - 1 and
 *               h[m - L + 1 : m] == ban_tok[r, q, 0 : L - 1]; or
 *   early stop: n[r] < ban_min[r] and v == stop_ids[r, j] for some j.
 * out[v] = -inf (the dtype's bit pattern) for a banned v, and l[v], the same 16 bits, otherwise: -0, subnormals, NaN payloads and +-inf pass
 * through (no float is made of a logit).  An id outside [0, V) bans nothing.  With m >= the longest bad word this is Hugging Face's rule
 * (transformers 5) for all three processors.  Below that length it deviates ON PURPOSE: HF skips a bad word with L > m, here its prefix is
 * matched from m >= L - 1 on, so a two-token bad word right behind a one-token prompt is still banned.  min_new_tokens holds back stop IDS only
 * -- neither a stop sequence (bd_srv_step_stop_sequences) nor a constraint's final state.  A row whose bans, alone or with a constraint, leave no
 * finite element is the caller's error, as a -inf bias on every token is: nothing is defined for it.
 * Device values the host could not have written are neutralised: ctx_len is clamped into [0, Lc], n into [0, tok_cap], a g outside
 * 0 .. BD_BAN_NGRAM_MAX is off, a ban_len outside 0 .. W is an unused slot.  History elements are compared as 64-bit integers.  An out element is
 * a pure function of (l[v], v, h, the row's parameters and tables): no global atomics, no two blocks write one address, nothing depends on R, on
 * the strides, on thread or block order, or on graph or eager execution, and the launch keeps no counter.  tests/ban_ref.py restates the
 * definition.
 * logits / out [R, V] fp16 / bf16 with row strides sl / so (elements); elements V .. stride - 1 of a row are neither read nor written.  The
 * other arrays are contiguous but for toks' row stride.  Checked before any device call, in this order: R < 0, V < 1, V > 2^22 ->
 * BD_E_BAD_SHAPE; dtype not fp16 / bf16 -> BD_E_BAD_DTYPE; R == 0 -> BD_OK, nothing launched; Q outside 1 .. BD_BAN_WORDS_MAX, W outside
 * 1 .. BD_BAN_WORD_LEN_MAX, ns outside 0 .. BD_BAN_STOP_MAX, Lc < 0, tok_cap < 0, s_tok < tok_cap, Lc + tok_cap > 2^31 - 1 or R > 65535 ->
 * BD_E_BAD_SHAPE; a needed pointer NULL (ctx only when Lc > 0, stop_ids when ns > 0, toks when n is given and tok_cap > 0) -> BD_E_NULL; V % 8,
 * a stride % 8 or < V, logits / out not 16-byte, toks / n / stop_ids not 8-byte, the int32 arrays not 4-byte aligned -> BD_E_BAD_SHAPE.
 * Several blocks per row: grid (ceil(V / 2048), R), 256 threads.  Every block walks the row's history (the n-gram tail staged once in LDS,
 * candidates rejected on their last token first), the bad-word table and the stop ids, and sets the bans of its own 2048 elements in a
 * 256-byte LDS bitmap; then one 16-byte load, the mask and one 16-byte store per thread. */
#define BD_BAN_NGRAM_MAX 8
#define BD_BAN_WORDS_MAX 64
#define BD_BAN_WORD_LEN_MAX 32
#define BD_BAN_STOP_MAX 64
int bd_srv_ban_rows(const void* logits, int64_t sl, int V, void* out, int64_t so, const int32_t* ctx, int Lc, const int32_t* ctx_len,
                    const int64_t* toks, int64_t s_tok, int tok_cap, const int64_t* n, const int32_t* ban_ngram, const int32_t* ban_tok,
                    const int32_t* ban_len, int Q, int W, const int32_t* ban_min, const int64_t* stop_ids, int ns, int R, int dtype,
                    void* stream);
/* bd_srv_step_ban: bd_srv_ban_rows inside a ragged decode step, behind the lm_head, bd_srv_step_penalize and bd_srv_step_constrain (whose row it
 * then reads, so a ban wins over a positive logit bias) and in front of bd_srv_step_end_ragged / bd_srv_step_end_sample (which then read
 * `out`); toks / n are the step end's output rows and counts BEFORE it runs, active bytes [T].  An inactive tenant's out row is not touched and
 * nothing of it is read.  Checks as above with T for R; n or active NULL -> BD_E_NULL. */
int bd_srv_step_ban(const void* logits, int64_t sl, int V, void* out, int64_t so, const int32_t* ctx, int Lc, const int32_t* ctx_len,
                    const int64_t* toks, int64_t s_tok, int tok_cap, const int64_t* n, const int32_t* ban_ngram, const int32_t* ban_tok,
                    const int32_t* ban_len, int Q, int W, const int32_t* ban_min, const int64_t* stop_ids, int ns, const uint8_t* active, int T,
                    int dtype, void* stream);
/* bd_srv_truncate_rows: the sampling filters that cut a row's tail by the row's OWN statistics -- Hugging Face's MinPLogitsWarper (min_p),
 * TypicalLogitsWarper (typical_p), EpsilonLogitsWarper (epsilon_cutoff) and EtaLogitsWarper (eta_cutoff) -- as one masked copy of the row.
 * Per row r: the logits l[0 .. V) (fp16 / bf16, V % 8 == 0), its temperature tau[r] (float32) and params[r, 0:4] (float32, contiguous [R, 4]):
 *   min_p          in [0, 1]   neutral 0
 *   typical_p      in (0, 1]   neutral 1
 *   epsilon_cutoff in [0, 1)   neutral 0
 *   eta_cutoff     in [0, 1)   neutral 0
 * out[v] is l[v], the same 16 bits, for a kept element and -inf (the dtype's bit pattern) for a dropped one; an element that was -inf stays
 * -inf.  The row is COPIED bit for bit (all V elements) when all four parameters are neutral, when tau is not in (0, inf) (a greedy request),
 * or when the row is special -- it holds a NaN or +inf, or nothing finite -- where the step end's greedy rule decides.
 * Statistics, over the finite elements F with maximum m: x_i = (l_i - m) / tau, w_i = exp(x_i), Z = sum w_i, p_i = w_i / Z, mu = sum p_i x_i,
 * H = ln Z - mu (the entropy of the row's distribution at tau).
 * Thresholds.  theta = max( ln min_p [min_p > 0], ln eps + ln Z [eps > 0], ln min(eta, sqrt(eta) exp(-H)) + ln Z [eta > 0] ), clamped to
 * <= 0; element i passes when x_i >= theta.  Every element equal to the maximum therefore passes (HF's min_tokens_to_keep = 1).
 * typical_p < 1.  The key is a_i = |x_i - mu| (= |-ln p_i - H|); element i passes when the mass of the elements with a strictly smaller key
 * is below typical_p.  Ties are all kept, as with the top-k threshold.  The most typical element always passes; the maximum need not.
 * All filters are judged on the row the launch receives (after penalties, constraints and bans, before top-k / top-p), and the kept set is the
 * INTERSECTION of their sets; if typical_p's set does not meet the thresholds' set, typical_p is ignored for that row.  With one filter set and
 * top-k / top-p off this is the Hugging Face warper of that name; with several, or with top-k / top-p behind it, the order is the project's
 * own (HF applies them one after another on renormalised survivors).
 * Arithmetic: the masses are bd_srv_sample_rows' 2^-40 fixed-point words, Z and sum w_i (-x_i) INTEGER sums of such words, ln Z, mu and theta
 * formed once in fp64 from the integers, x in fp32, the key |x - mu| in 2^-27 fixed point (finer than x's own fp32 rounding wherever
 * |x| > 0.06; an element that weighs anything lies below 32); the typical_p select is an exact radix select over the four bytes of that key
 * with integer mass histograms.  A finite element whose l - m or x overflows fp32 (a bf16 row wider than FLT_MAX, a tiny tau) has x = -inf:
 * mass 0 and the lowest key.  No floating-point atomics: out is a pure function of the row and the five numbers -- nothing depends on R, the
 * row's index, the strides, the form (rows / step), thread order, or graph or eager execution -- and the launch keeps no counter.
 * Device values the host could not have written are neutralised: a NaN parameter, min_p <= 0, typical_p outside (0, 1), eps <= 0 and eta <= 0
 * are off; min_p >= 1 keeps the maximum only.  tests/truncation_ref.py restates the definition in fp64 with the tolerance the tests allow.
 * logits / out [R, V] with row strides sl / so (elements); elements V .. stride - 1 of a row are neither read nor written; out must not overlap
 * logits.  Checked before any device call, in this order: R < 0, V < 1, V > 2^22 -> BD_E_BAD_SHAPE; dtype not fp16 / bf16 -> BD_E_BAD_DTYPE;
 * R == 0 -> BD_OK, nothing launched; a pointer NULL -> BD_E_NULL; V % 8, a stride % 8 or < V, logits / out not 16-byte, tau / params not
 * 4-byte aligned -> BD_E_BAD_SHAPE.
 * One 256-thread block per row; up to V = 32768 the row is read once and lives in registers.  A row pays for what it asks: min_p alone the
 * maximum and the mask pass; epsilon adds Z; eta or typical_p add mu; only typical_p runs the select. */
int bd_srv_truncate_rows(const void* logits, int64_t sl, int V, void* out, int64_t so, const float* tau, const float* params, int R, int dtype,
                         void* stream);
/* bd_srv_step_truncate: bd_srv_truncate_rows inside a ragged decode step, the last of the masks: behind the lm_head, bd_srv_step_penalize,
 * bd_srv_step_constrain and bd_srv_step_ban (whose row it then reads) and in front of bd_srv_step_end_sample (which then reads `out`, applies
 * top-k / top-p to it and draws); tau is the step end's temperature array, active bytes [T].  An inactive tenant's out row is not touched and
 * nothing of it is read.  Checks as above with T for R; active NULL -> BD_E_NULL. */
int bd_srv_step_truncate(const void* logits, int64_t sl, int V, void* out, int64_t so, const float* tau, const float* params,
                         const uint8_t* active, int T, int dtype, void* stream);
/* bd_srv_cache_warm (round 6): reads [p0, p0 + bytes0) and [p1, p1 + bytes1) (16-byte aligned; whole 16-byte chunks) and discards the values:
 * a weight-prefetch launch for a hipGraph side branch (the serving loop forks it next to the decode attention launch so that the o projection's
 * weight and sign words sit in the Infinity Cache when it starts).  blocks = 0: one 256-thread block per CU.  No reference counterpart (the
 * reference's decode step is demo/demo_backend.py:93-98 under HF's eager loop); changes no arithmetic. */
int bd_srv_cache_warm(const void* p0, int64_t bytes0, const void* p1, int64_t bytes1, int blocks, void* stream);
int bd_srv_decode_attention(const void* QKV, const void* cos_t, const void* sin_t, void* kcache, void* vcache, void* valid,
                            const int64_t* pos, void* out, int T, int H, int KVH, int head_dim, int Lc,
                            int64_t s_qkv, int64_t s_out, int dtype, void* ws, int64_t ws_bytes, void* stream);
/* bd_srv_decode_attention_ragged: bd_srv_decode_attention with one position per tenant.  pos int64 [T], active bytes [T] (both on the device);
 *   everything else as there, including the validation, the workspace (bd_srv_decode_attention_workspace_bytes, same ticket contract), the
 *   split rule and the ring depth: at equal positions it is the same launch geometry and the same bits.  Tenant t's key range 0..pos[t], its
 *   split bounds, its RoPE table row, its cache append at pos[t] and its valid[t, pos[t]] mark all follow its own position.  A tenant with
 *   active[t] == 0, pos[t] < 0 or pos[t] >= Lc stays out of the launch: nothing is appended or marked, its H*128 outputs are written as zeros,
 *   and its blocks leave before any partial store or ticket increment (every split of a (tenant, kv head) pair takes the same decision, so
 *   the tickets are zero at exit).  The range guard is part of the contract: pos is device data that advances without the host seeing it. */
int bd_srv_decode_attention_ragged(const void* QKV, const void* cos_t, const void* sin_t, void* kcache, void* vcache, void* valid,
                                   const int64_t* pos, const void* active, void* out, int T, int H, int KVH, int head_dim, int Lc,
                                   int64_t s_qkv, int64_t s_out, int dtype, void* ws, int64_t ws_bytes, void* stream);
/* bd_srv_decode_attention_tab / bd_srv_decode_attention_ragged_tab: the two entries above with PER-TENANT rotary tables.  s_tab is the tenant
 *   stride of cos_t / sin_t in elements: 0 = one shared [Lmax, 128] table (the same launch and the same bits as the entry without the argument);
 *   otherwise [T, Lmax, 128] with tenant t's rows at cos_t + t * s_tab, so tenant t's q and new k are rotated with row pos (ragged: pos[t]) of ITS
 *   table.  The same kernels: the stride is a launch argument, the tenant's offset is scalar arithmetic in front of the RoPE inputs' loads.
 *   Validation, workspace, split rule, ring depth, NULL handling and the ragged form's stay-out rule as in the originals.  BD_E_BAD_SHAPE, before any
 *   device call, when s_tab < 0, s_tab % 8 != 0 or a table pointer is not 16-byte aligned (the entries without the argument do not ask for
 *   aligned tables and keep not asking). */
int bd_srv_decode_attention_tab(const void* QKV, const void* cos_t, const void* sin_t, int64_t s_tab, void* kcache, void* vcache, void* valid,
                                const int64_t* pos, void* out, int T, int H, int KVH, int head_dim, int Lc,
                                int64_t s_qkv, int64_t s_out, int dtype, void* ws, int64_t ws_bytes, void* stream);
int bd_srv_decode_attention_ragged_tab(const void* QKV, const void* cos_t, const void* sin_t, int64_t s_tab, void* kcache, void* vcache, void* valid,
                                       const int64_t* pos, const void* active, void* out, int T, int H, int KVH, int head_dim, int Lc,
                                       int64_t s_qkv, int64_t s_out, int dtype, void* ws, int64_t ws_bytes, void* stream);
/* bd_srv_prefill_attention: attention of a whole prompt (the prefill call of the serving loop, demo/demo_backend.py:262-275 -> the HF
 *   decoder layer's attention with the left-padded attention_mask; what F.scaled_dot_product_attention computes there), flash-style:
 *   O[b, s, h] = softmax_k(Q[b, s, h] . K[b, k, h / (H/KVH)] * scale) . V[b, k, h / (H/KVH)] over the keys kv_start[b] <= k (<= s when
 *   causal), fp32 online softmax, 16-bit in / out.  Q / K / V / O are [B, S, heads, 128] through their batch and sequence strides in
 *   elements (head h at + 128 h): the three slices of a fused q|k|v projection output are passed as they lie.  kv_start [B] int32 on
 *   the device (left padding) or NULL; query rows with no valid key return 0.  head_dim == 128, S % 64 == 0, strides % 8 == 0,
 *   16-byte aligned pointers; anything else returns BD_E_BAD_SHAPE and the caller keeps its own attention. */
int bd_srv_prefill_attention(const void* Q, const void* K, const void* V, void* O, int B, int S, int H, int KVH, int head_dim,
                             int64_t sqb, int64_t sqs, int64_t skb, int64_t sks, int64_t svb, int64_t svs, int64_t sob, int64_t sos,
                             const int32_t* kv_start, float scale, int causal, int dtype, void* stream);
/* bd_srv_prefill_attention_cached: bd_srv_prefill_attention for a CHUNK of Sq queries at positions q0 .. q0 + Sq - 1 over the keys already in the
 *   KV caches -- the next turn of a conversation whose earlier turns are cached (the reference re-sends and re-prefills the whole history with
 *   every request, demo/demo_backend.py:261-315), or one chunk of a long prompt.  Always causal:
 *   O[b, i, h] = softmax_k(Q[b, i, h] . Kc[b, h / (H/KVH), k] * scale) . Vc[b, h / (H/KVH), k] over kv_start[b] <= k <= q0 + i, i = 0 .. Sq - 1.
 *   Q / O as there ([B, Sq, H, 128] through batch and sequence strides: the q slice of the fused projection output as it lies); Kc / Vc are the
 *   caches [B, KVH, Lc, 128] through batch, head and key strides (skb, skh, sks / svb, svh, svs, elements), read AFTER bd_srv_rope_kv_append
 *   (pos0 = q0) has written the chunk's own rows.  Same tile walk and per-row arithmetic as bd_srv_prefill_attention: row i is bit for bit row
 *   q0 + i of that call over the whole sequence.  Cache rows at or past q0 + Sq are never trusted: addresses are clamped into [0, Lc), such a
 *   key's score is masked and its V row is zeroed before the matrix product, so a non-finite bit pattern there reaches no output.  kv_start [B]
 *   int32 on the device or NULL, clamped into [0, q0 + Sq] in the kernel; query rows with no valid key return 0.
 *   BD_E_BAD_SHAPE, from host checks that run before any device call: head_dim != 128, H % KVH != 0, Sq < 1, q0 < 0, q0 + Sq > Lc, a stride that
 *   is not a multiple of 8, a pointer that is not 16-byte aligned.  B == 0 is an empty call (BD_OK). */
int bd_srv_prefill_attention_cached(const void* Q, const void* Kc, const void* Vc, void* O, int B, int Sq, int H, int KVH, int head_dim, int q0,
                                    int Lc, int64_t sqb, int64_t sqs, int64_t skb, int64_t skh, int64_t sks, int64_t svb, int64_t svh,
                                    int64_t svs, int64_t sob, int64_t sos, const int32_t* kv_start, float scale, int dtype, void* stream);
/* scratch for bd_srv_decode_attention's split of the key range over 4 blocks per (tenant, kv head) (up to 16 for one or two sequences of a
 * grouped-query model; the size returned covers the largest split count and depends on the geometry only), merged inside the launch by the
 * block that finishes last (0 = the cache is short enough to run unsplit; ws may then be NULL).  Without a workspace the kernel
 * runs unsplit.  CONTRACT: the first 16 KiB of ws (arrival counters) are ZERO when the launch is enqueued; the kernel puts them
 * back to zero, so a buffer that is zero-filled once and used by one stream at a time can be reused by every call. */
int64_t bd_srv_decode_attention_workspace_bytes(int T, int H, int KVH, int head_dim, int Lc);

/* bytes of scratch bd_delta_bmm / bd_binary_linear may need for this problem (split-k partials of the decode path) */
int64_t bd_gemm_workspace_bytes(int B, int M, int N, int K);

/* BinaryDiff.__init__ buffers in one pass -- bitdelta/diff.py:9-31: mask = pack((fine - base >= 0).T) int32 [K/32, N],
 * coeff = mean|fine - base| (fp32, device scalar).  base, fine: [N,K] row-major, leading dimension ld. */
int bd_binarize(const void* base, const void* fine, int64_t N, int64_t K, int64_t ld, int dtype,
                int32_t* mask, float* coeff, void* ws, int64_t ws_bytes, void* stream);
int64_t bd_binarize_workspace_bytes(int64_t N, int64_t K);

/* load_diff's merge line -- bitdelta/diff.py:93-95: W[n,k] = round(W[n,k] + round(+-coeff)); coeff: device fp32 scalar. */
int bd_merge_delta(void* W, int64_t ldw, const int32_t* P, const float* coeff, int64_t N, int64_t K, int dtype,
                   void* stream);

/* Replace ONE tenant's sign words of ONE projection inside the buffers of a fused multi-tenant Linear, in place.
 *   src         [KW][N_src] int32, the reference / diff.pt layout: row stride ld_src elements (>= N_src), columns contiguous.
 *   packed_dst  the packed decode words of the whole tenant set, int32 [ceil(N_fused/16)][ceil(KW/4)][4 g][16 c][t_pad] (what
 *               bd_binary_linear_decode reads with packed = 1): the dword at [tile][it][g][c][slot] gets byte s = byte g of
 *               src[4 it + s][n], rows >= KW reading as zero.  Only the dwords of `slot` and of this projection's columns are
 *               written: the other slots, the padding slots and the columns between N_fused and 16 ceil(N_fused/16) keep their bytes.
 *   mask_dst    the tenant's plane of the fused reference-layout words, [KW][N_fused] with row stride ld_mask_dst (>= N_fused): the
 *               same words, unshuffled (what prefill reads).
 *   Either destination may be NULL (skipped); both NULL is BD_E_NULL.
 * Column map, source column n -> fused column n' (16 tile + c = n'):   n' = col_off + (n / col_blk) * col_stride + n % col_blk
 *   concatenated projections:          col_off = the projection's first column, col_blk = N_src (col_stride unused)
 *   a pair interleaved in blocks of 8: col_off = 8 * (0 | 1), col_blk = 8, col_stride = 16
 * t_pad in {1, 2, 4, 6, 8, 12, 16} and 0 <= slot < t_pad, else BD_E_BAD_SHAPE; col_blk >= 1 dividing N_src, else BD_E_BAD_GROUPS; every
 * mapped column inside N_fused, blocks that do not overlap (col_stride >= col_blk) and ld_src >= N_src, else BD_E_BAD_SHAPE.  All of it
 * is checked before any device work; N_src == 0 or KW == 0 is a no-op.  No workspace, no atomics: one launch on `stream`. */
int bd_tenant_signs_load(const int32_t* src, int64_t ld_src, int64_t KW, int64_t N_src, int32_t* mask_dst, int64_t ld_mask_dst,
                         int32_t* packed_dst, int64_t N_fused, int t_pad, int slot, int64_t col_off, int64_t col_blk,
                         int64_t col_stride, void* stream);

/* The tuning / A-B hooks (bd_set_*, bd_last_*) are declared in bitdelta_hip_test.h: thread-local, not part of the stable interface a
 * reference-side binding needs (INTEGRATION.md binds none of them), free to change between versions. */

#ifdef __cplusplus
}
#endif
#endif
