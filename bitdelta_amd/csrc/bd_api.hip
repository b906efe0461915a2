// C ABI of libbitdelta_hip.so (see include/bitdelta_hip.h): argument checking + kernel dispatch.
// The decode Linear's streaming kernel is dispatched in two steps: stream_plan() decides (plain host code: form, depth, cache policy, grid, LDS)
// and launch_stream() lifts the plan to the one instantiation of the shipped set, stream_shipped(); bd_last_decode_plan reports the plan.
// No torch types.  State: the test / tuning overrides (bd_set_*) are THREAD-LOCAL, so a thread that forces a kernel family does not
// change what other threads launch; the per-DEVICE caches (CU count, "max dynamic LDS already raised for this kernel") are keyed
// by the current device id -- the reference's demo runs one process over several GPUs (demo/demo_backend.py:23-25).
#include "../../include/bitdelta_hip.h"
#include "../../include/bitdelta_hip_test.h"
#include "bd_bits.h"
#include "bd_gemm_generic.h"
#include "bd_gemm_mfma.h"
#ifdef BD_AB_VARIANTS      // rejected schedules kept as A/B references: harness-only build (tests/native/Makefile)
#include "../../tests/native/ab/bd_gemm_pp.h"
#endif
#include "bd_gemm_pf.h"
#include "bd_gemm_fx.h"
#include "bd_gemm_w4.h"
#include "bd_gemv.h"
#include "bd_gemv_stream.h"
#include "bd_gemv_rows.h"
#ifdef BD_AB_VARIANTS
#include "../../tests/native/ab/bd_gemv_ring.h"     // LDS-DMA loader / consumer decode kernel: lost its A/B (profiles/r04_decode_ring_ab.txt)
#endif
#include "bd_serving.h"
#include "bd_attn_prefill.h"
#include "bd_token_nll.h"
#include "bd_logprobs.h"
#include "bd_penalize.h"
#include "bd_constrain.h"
#include "bd_stop_seq.h"
#include "bd_ban.h"
#include "bd_truncate.h"
#include <algorithm>
#include <cstdlib>
#include <atomic>
#include <tuple>

using namespace bd;

// Environment override of the shape -> variant table (build notes): BD_GEMM_VARIANT=<n> is the initial value of every thread's
// forced variant (exactly bd_set_gemm_variant(n), which still overrides it); BD_TAIL_SPLIT=0 switches the tail split off.  Read once per thread.
static int env_int(const char* name, int dflt) {
    const char* v = getenv(name);
    return (v && *v) ? atoi(v) : dflt;
}
static thread_local int g_forced_variant = env_int("BD_GEMM_VARIANT", -1);
static thread_local int g_tail_split = env_int("BD_TAIL_SPLIT", 1) ? 1 : 0;          // A/B hook (bd_set_tail_split)
// delta_rows_kernel A/B hook (environment only): bits 1-2 = masks per block forced to 1 / 2 / 4 (value 1 / 2 / 3), bit 4 = never chosen automatically,
// bit 5 = 64-column super-tiles even when they leave CUs idle, bit 6 = 32-column super-tiles always
static thread_local int g_rows_tune = env_int("BD_ROWS_TUNE", 0);
static thread_local int g_norm_rows_min = env_int("BD_NORM_ROWS_MIN", 64);           // bd_srv_rmsnorm: rows from which the wave-per-row kernel runs (A/B hook)
static thread_local int g_attn_depth = env_int("BD_ATTN_DEPTH", 0);                 // decode attention K / V ring depth: 0 = by cache length, 2, 4 (A/B hook)
static thread_local int g_rows_shared_min = env_int("BD_ROWS_SHARED_MIN", 1);       // shared mask: rows from which the kernel is chosen automatically
static thread_local int g_forced_group_m = 0;        // 0 = automatic tile order
static thread_local int g_col16_small_lut = -1;      // sign LUT of the 16-column decode kernel: -1 auto, 1 = single 4-KiB table, 0 = 16-copy conflict-free
                                        // table whenever it fits.  Auto = 16 copies for delta-only launches (-16..18 % at 6-8 masks;
                                        // fused: -2 %, and -15 % WORSE on 14336x4096 where it drops to one block per CU)
static thread_local int g_col16_no_per4 = 0;         // A/B hook: 1 = the 16-column decode kernel always uses its generic one-ahead loop
static thread_local int g_launch_chunking = 0;       // 1 = multi-round tile problems are issued as single-round launches (measured: no gain; off)
static thread_local int g_gemv_wave_spec = 1;        // 1 = fused launches of the VALU decode kernel use its wave-specialised form
static thread_local int g_gemv_two_launch = 1;       // 1 (default) = split-k partials are summed by gemv_reduce_kernel; 0 = in-launch tickets
                                        // (measured slower: the last-arriver tail is serial inside every tile; bd_gemv.h)
static thread_local int g_gemv_target_blocks = 512;
static thread_local int g_stream_tune = 0;            // A/B hook (harness build): bit 0 = natural-order W, bit 1 = nt cache policy, bit 2 = 8-wave blocks, bit 3 = deeper prefetch
static thread_local int g_decode_engine = -1;         // (harness builds) packed-layout decode launches: -1 / 0 = streaming register-load kernel
                                                      // (variant 600), 1 = LDS-DMA loader / consumer kernel (variant 700, tests/native/ab/)
static thread_local int g_ring_tune = -1;             // variant 700 knobs, -1 = defaults: bit 0 = nt weight / sign streams, bit 1 = activations ride the
                                                      // ring even when a resident copy fits, bit 2 = ONE loader wave (default two), bits 8..13 = cap on
                                                      // the ring slots (0 = none)
static thread_local int t_last_variant = -1;
static thread_local int t_last_attention_form = 0; // decode_attn_kernel instantiation of the last launch: nsplit | DEPTH << 8 | MAXS << 16 | G << 24

extern "C" int bd_version(void) { return 1; }
extern "C" int bd_set_gemm_variant(int v) { g_forced_variant = v; return BD_OK; }
extern "C" int bd_last_gemm_variant(void) { return t_last_variant; }
extern "C" int bd_set_tail_split(int v) { g_tail_split = v ? 1 : 0; return BD_OK; }
extern "C" int bd_set_tile_group_m(int g) { g_forced_group_m = g; return BD_OK; }
extern "C" int bd_set_decode_two_launch(int on) { g_gemv_two_launch = on ? 1 : 0; return BD_OK; }
extern "C" int bd_set_decode_wave_spec(int on) { g_gemv_wave_spec = on ? 1 : 0; return BD_OK; }
extern "C" int bd_set_launch_chunking(int on) { g_launch_chunking = on ? 1 : 0; return BD_OK; }
extern "C" int bd_set_decode_generic_loop(int on) { g_col16_no_per4 = on ? 1 : 0; return BD_OK; }
extern "C" int bd_set_stream_tuning(int flags) { g_stream_tune = flags; return BD_OK; }
extern "C" int bd_last_attention_form(void) { return t_last_attention_form; }
extern "C" int bd_set_decode_engine(int engine) { g_decode_engine = engine < 0 ? -1 : (engine ? 1 : 0); return BD_OK; }
extern "C" int bd_set_ring_tuning(int flags) { g_ring_tune = flags; return BD_OK; }
extern "C" int bd_set_decode_small_lut(int mode) { g_col16_small_lut = mode < 0 ? -1 : (mode ? 1 : 0); return BD_OK; }

extern "C" const char* bd_error_string(int code) {
    switch (code) {
        case BD_OK: return "ok";
        case BD_E_K_NOT_MULTIPLE: return "K must be divisible by n_bits";
        case BD_E_BAD_NBITS: return "n_bits must be 8, 16, 32 or 64";
        case BD_E_BAD_GROUPS: return "scale groups must divide N";
        case BD_E_BAD_DTYPE: return "unsupported dtype";
        case BD_E_BAD_SHAPE: return "bad shape / stride / forced variant not applicable";
        case BD_E_WORKSPACE: return "workspace missing or too small";
        case BD_E_LAUNCH: return "kernel launch failed";
        case BD_E_NULL: return "null pointer";
        default: return "unknown error";
    }
}

static inline int launch_status() { return hipGetLastError() == hipSuccess ? BD_OK : BD_E_LAUNCH; }

// ------------------------------------------------------------------ pack / unpack
extern "C" int bd_pack(const void* bits, int64_t batch, int64_t K, int64_t N, int64_t s_b, int64_t s_k, int64_t s_n,
                       void* out, int n_bits, void* stream) {
    if (n_bits != 8 && n_bits != 16 && n_bits != 32 && n_bits != 64) return BD_E_BAD_NBITS;
    if (batch < 0 || K < 0 || N < 0) return BD_E_BAD_SHAPE;
    if (K % n_bits) return BD_E_K_NOT_MULTIPLE;
    if (batch == 0 || K == 0 || N == 0) return BD_OK;
    if (!bits || !out) return BD_E_NULL;
    const int64_t KW = K / n_bits;
    if (KW > 65535 * 8LL || batch > 65535) return BD_E_BAD_SHAPE;
    hipStream_t st = (hipStream_t)stream;
    const uint8_t* b8 = (const uint8_t*)bits;
    if (n_bits == 32 && s_k == 1 && s_n != 1) {
        dim3 grid((unsigned)((N + 63) / 64), (unsigned)((KW + 7) / 8), (unsigned)batch);
        hipLaunchKernelGGL(pack_kmajor_kernel, grid, dim3(256), 0, st, b8, (uint32_t*)out, (long long)KW, (long long)N,
                           (long long)s_b, (long long)s_n);
        return launch_status();
    }
    if (KW > 65535) return BD_E_BAD_SHAPE;
    dim3 grid((unsigned)((N + 255) / 256), (unsigned)KW, (unsigned)batch);
#define BD_PACK(T) hipLaunchKernelGGL(pack_kernel<T>, grid, dim3(256), 0, st, b8, (T*)out, (long long)KW, (long long)N, \
                                      (long long)s_b, (long long)s_k, (long long)s_n)
    if (n_bits == 8) BD_PACK(uint8_t);
    else if (n_bits == 16) BD_PACK(uint16_t);
    else if (n_bits == 32) BD_PACK(uint32_t);
    else BD_PACK(uint64_t);
#undef BD_PACK
    return launch_status();
}

extern "C" int bd_unpack(const void* words, int64_t batch, int64_t KW, int64_t N, void* out_bits, int n_bits, void* stream) {
    if (n_bits != 8 && n_bits != 16 && n_bits != 32 && n_bits != 64) return BD_E_BAD_NBITS;
    if (batch < 0 || KW < 0 || N < 0 || KW > 65535 || batch > 65535) return BD_E_BAD_SHAPE;
    if (batch == 0 || KW == 0 || N == 0) return BD_OK;
    if (!words || !out_bits) return BD_E_NULL;
    hipStream_t st = (hipStream_t)stream;
    dim3 grid((unsigned)((N + 1023) / 1024), (unsigned)KW, (unsigned)batch);
#define BD_UNPACK(T) hipLaunchKernelGGL(unpack_kernel<T>, grid, dim3(256), 0, st, (const T*)words, (uint8_t*)out_bits, \
                                        (long long)KW, (long long)N)
    if (n_bits == 8) BD_UNPACK(uint8_t);
    else if (n_bits == 16) BD_UNPACK(uint16_t);
    else if (n_bits == 32) BD_UNPACK(uint32_t);
    else BD_UNPACK(uint64_t);
#undef BD_UNPACK
    return launch_status();
}

// ------------------------------------------------------------------ one tenant's sign words into the decode / prefill buffers
extern "C" int bd_tenant_signs_load(const int32_t* src, int64_t ld_src, int64_t KW, int64_t N_src, int32_t* mask_dst, int64_t ld_mask_dst,
                                    int32_t* packed_dst, int64_t N_fused, int t_pad, int slot, int64_t col_off, int64_t col_blk,
                                    int64_t col_stride, void* stream) {
    if (KW < 0 || N_src < 0 || N_fused < 0 || KW > (1LL << 26) || N_src > (1LL << 30) || N_fused > (1LL << 30)) return BD_E_BAD_SHAPE;
    if (t_pad != 1 && t_pad != 2 && t_pad != 4 && t_pad != 6 && t_pad != 8 && t_pad != 12 && t_pad != 16) return BD_E_BAD_SHAPE;
    if (slot < 0 || slot >= t_pad) return BD_E_BAD_SHAPE;
    if (col_blk < 1 || N_src % col_blk) return BD_E_BAD_GROUPS;
    const int64_t nblk = N_src / col_blk;
    if (col_off < 0 || col_off > N_fused || (nblk > 1 && (col_stride < col_blk || col_stride > N_fused))) return BD_E_BAD_SHAPE;
    if (N_src > 0 && col_off + (nblk - 1) * (nblk > 1 ? col_stride : 0) + col_blk > N_fused) return BD_E_BAD_SHAPE;
    if (ld_src < N_src || (mask_dst && ld_mask_dst < N_fused)) return BD_E_BAD_SHAPE;
    if (N_src == 0 || KW == 0) return BD_OK;
    if (!src || (!mask_dst && !packed_dst)) return BD_E_NULL;
    const int64_t NIT = (KW + 3) / 4;
    const unsigned gx = (unsigned)((N_src + 255) / 256);
    const int64_t gy = (NIT + 3) / 4;              // a block = 256 source columns x 4 `it` (one per wave)
    if (gy > 65535) return BD_E_BAD_SHAPE;
    const bool adjacent = col_blk % 4 == 0 && col_off % 4 == 0 && (nblk == 1 || col_stride % 4 == 0);
    int vec = 0;
    if (((uintptr_t)src & 15) == 0 && ld_src % 4 == 0) vec |= 1;
    if (adjacent && mask_dst && ((uintptr_t)mask_dst & 15) == 0 && ld_mask_dst % 4 == 0) vec |= 2;
    if (adjacent && packed_dst && t_pad == 1 && ((uintptr_t)packed_dst & 15) == 0) vec |= 4;
    hipLaunchKernelGGL(tenant_signs_load_kernel, dim3(gx, (unsigned)gy), dim3(256), 0, (hipStream_t)stream, (const uint32_t*)src,
                       (long long)ld_src, (int)KW, (int)N_src, (uint32_t*)mask_dst, (long long)ld_mask_dst, (uint32_t*)packed_dst, t_pad, slot,
                       (int)col_off, (int)col_blk, (int)(nblk > 1 ? col_stride : 0), vec);
    return launch_status();
}

// ------------------------------------------------------------------ GEMM dispatch
namespace {

struct Problem {
    const void *A, *W;
    const int32_t* P;
    const float* alpha;
    void* C;
    int B, M, N, K;
    int64_t sAb, sAm, sPb, sCb, sCm, ldw, sAlb;
    int G, dtype, out_dtype, round_mode, accumulate;
    int mask_tiled;           // 0: P is [B or 1, K/32, N] (reference layout); 1: tile-major [B or 1, ceil(N/16), K/32, 16];
                              // 2: packed decode layout [ceil(N/16), ceil(K/128), 4, 16, t_pad] (decode kernel only, see bd_gemv_stream.h)
    int w_tiled;              // layout 2 only: W is the tile-major decode copy [N/16][K/128][4 steps][16 rows][4 groups][8] (ldw passed as 0);
                              // 2 = the INT8 tile-major copy of bd_binary_linear_decode_w8, [N/16][K/128][2][16 rows][4 groups][2][8] bytes
    const float* wscale;      // w_tiled == 2: fp32 [N], multiplies the base sum of each output column
                              // w_tiled == 3: the 4-bit GPTQ tile-major copy of bd_binary_linear_decode_q4, dwords [N/16][K/128][16 rows][4 groups][4 steps]
    const uint32_t* q4p;      // w_tiled == 3: packed group parameters [N/16][K/q4_group][16] (fp16 scale | fp16 (1024 + z) << 16)
    int q4_group;             // w_tiled == 3: GPTQ group size along K (a multiple of 128 that divides K)
    int t_pad;                // layout 2: dwords per (tile, iteration, lane group, column) = tenants padded to 1 / 2 / 4 / 6 / 8
    const void* norm_w;       // layout 2 only: fused RMSNorm prologue (A is the un-normalised residual stream); [B or 1, K], stride sNw
    int64_t sNw;
    float eps;
    int epilogue;             // layout 2 only: 1 = SwiGLU over an 8-interleaved gate|up projection (C has N/2 columns)
    const float* ssq_in;      // layout 2 only: RMSNorm hand-off, consumer side (with norm_w): per-row partial sums of squares [K/16][16]
    float* ssq_out;           // layout 2 only: RMSNorm hand-off, producer side: this launch writes its output's partial sums [N/16][16]
    const void* nw_next;      // ... producer with xw_out: the NEXT RMSNorm's weight [B or 1, N] (stride sNwNext) and the pre-multiplied copy
    int64_t sNwNext;
    void* xw_out;
    const void* pn_w;         // bd_binary_linear_residual_norm: the RMSNorm that FOLLOWS this Linear -- weight [B or 1, N] (stride s_pnw), output pn_h
    int64_t s_pnw;            // [B, M, N] (strides sHb / sHm).  A split-k reduce launch takes it along (splitk_reduce_norm_kernel; TilePlan::post_norm);
    float pn_eps;             // otherwise the entry point launches the norm after the Linear.
    void* pn_h;
    int64_t sHb, sHm;
    void* ws;
    int64_t ws_bytes;
    hipStream_t st;
};

constexpr int MAX_DEVICES = 64;
inline int current_device() {
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0) dev = 0;
    return dev;
}
inline int num_cus() {
    static std::atomic<int> cus[MAX_DEVICES];     // 0 = not queried yet; benign race: idempotent
    const int dev = current_device();
    if (dev >= MAX_DEVICES) return 256;
    int n = cus[dev].load(std::memory_order_relaxed);
    if (n == 0) {
        if (hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n <= 0) n = 256;
        cus[dev].store(n, std::memory_order_relaxed);
    }
    return n;
}
// hipFuncSetAttribute(MaxDynamicSharedMemorySize) is a per-device property of a kernel: raise it once per (kernel, device).
// `done` is one bit per device id, owned by the call site (one static per kernel instantiation).
inline bool ensure_dyn_lds(const void* kern, int bytes, std::atomic<uint64_t>& done) {
    const int dev = current_device();
    const uint64_t bit = dev < MAX_DEVICES ? (1ull << dev) : 0;
    if (bit && (done.load(std::memory_order_acquire) & bit)) return true;
    if (hipFuncSetAttribute(kern, hipFuncAttributeMaxDynamicSharedMemorySize, bytes) != hipSuccess) return false;
    if (bit) done.fetch_or(bit, std::memory_order_release);
    return true;
}

constexpr int GEMV_MAX_M = 16, GEMV_MAX_R = 16;   // decode kernels: <= 16 activation rows per launch; larger batches are chunked

inline bool aligned16(const void* p) { return (((uintptr_t)p) & 15) == 0; }

inline bool fast_ok(const Problem& q) {
    bool ok = (q.K % 64 == 0) && aligned16(q.A) && (q.sAm % 8 == 0) && (q.sAb % 8 == 0);
    if (q.W) ok = ok && aligned16(q.W) && (q.ldw % 8 == 0);
    // 32-bit DMA offsets inside a block: rows*stride*2 bytes must fit
    ok = ok && ((int64_t)256 * q.sAm * 2 < (1LL << 31)) && ((int64_t)q.N * 8 + 1024 < (1LL << 31));
    if (q.W) ok = ok && ((int64_t)256 * q.ldw * 2 < (1LL << 31));
    return ok;
}
inline bool gemv_ok(const Problem& q) {
    bool ok = (q.M <= GEMV_MAX_M) && ((int64_t)q.B * q.M <= 4 * GEMV_MAX_R) && (q.K % 32 == 0) && aligned16(q.A) &&   // <= 4 chunks
              (q.sAm % 8 == 0) && (q.sAb % 8 == 0);
    if (q.W) ok = ok && aligned16(q.W) && (q.ldw % 8 == 0);
    return ok;
}

// f(std::integral_constant<int, V>) for the first V of the ascending list with n <= V (the last V beyond it): a count to its bucket's template argument
template <int... Vs, class F>
void for_bucket(int n, F&& f) {
    constexpr int last = std::max({Vs...});
    (void)(((n <= Vs || Vs == last) && (f(std::integral_constant<int, Vs>{}), true)) || ...);
}

inline void gemv_split(const Problem& q, int& KS, int& kslice) {
    const int tiles_n = (q.N + 63) / 64;
    int want = (g_gemv_target_blocks + tiles_n - 1) / tiles_n;   // fat blocks keep many loads in flight each
    if (g_forced_variant > 200 && g_forced_variant <= 264) want = g_forced_variant - 200;     // test hook: 200 + KS
    if (g_forced_variant > 300 && g_forced_variant <= 364) want = g_forced_variant - 300;
    if (g_forced_variant > 400 && g_forced_variant <= 464) want = g_forced_variant - 400;
    int maxks = q.K / 512;                                // at least 512 k per slice
    if (maxks < 1) maxks = 1;
    KS = want < 1 ? 1 : (want > maxks ? maxks : want);
    kslice = ((q.K + KS - 1) / KS + 127) / 128 * 128;
    const int smax = gemv_kslice_max(16);
    if (kslice > smax) kslice = smax;                     // the activation slice lives in LDS
    KS = (q.K + kslice - 1) / kslice;
}

template <int DT, int RMAX>
int launch_gemv_valu(const Problem& q, const GemvParams& gp) {       // A/B reference (variant 300): VALU sign-flip form
    dim3 grid((unsigned)((q.N + 63) / 64), (unsigned)gp.KS);
    // fused launches: the wave-specialised instantiation (4 weight-streaming waves + 4 sign waves per block)
    // (-6..13 % up to 8 rows; at 16 tenants the sign work dominates and halving the sign waves per CU costs 22 %)
    if (q.W && g_gemv_wave_spec && gp.R <= 8) hipLaunchKernelGGL((gemv_kernel<DT, RMAX, true>), grid, dim3(512), 0, q.st, gp);
    else hipLaunchKernelGGL((gemv_kernel<DT, RMAX, false>), grid, dim3(256), 0, q.st, gp);
    return BD_OK;
}

template <int DT, int NM>
int launch_gemv_mfma(const Problem& q, const GemvParams& gp) {
    dim3 grid((unsigned)((q.N + 63) / 64), (unsigned)gp.KS);
    // LC = 16 (conflict-free 16-copy sign LUT, 64 KiB) measured SLOWER than the single 4-KiB table (T=6, 4096^2: 24.3 vs 17.9 us):
    // building 64 KiB per block and 2 blocks/CU cost more than the ~3-way conflicts of random bytes on one table.
    constexpr int LC = 1;
    const unsigned lds = 256u * 16u * LC + (unsigned)gp.R * (gemv_kslice_max(16) * 2 + 16);
    auto kw = gemv_mfma_kernel<DT, NM, true, LC>;
    auto kd = gemv_mfma_kernel<DT, NM, false, LC>;
    static std::atomic<uint64_t> done_w{0}, done_d{0};
    if (!ensure_dyn_lds((const void*)(q.W ? kw : kd), 256 * 16 * LC + 16 * 2064, q.W ? done_w : done_d)) return BD_E_LAUNCH;
    if (q.W) hipLaunchKernelGGL(kw, grid, dim3(256), lds, q.st, gp);
    else hipLaunchKernelGGL(kd, grid, dim3(256), lds, q.st, gp);
    return BD_OK;
}

template <int DT>
int launch_gemv_chunk(const Problem& q, bool valu_form);

// ---- no-split-k decode kernel (gemv_col16_kernel): 16 columns x all of k per block, 8 waves split k, LDS reduction
constexpr int COL16_LDS_BUDGET = 160 * 1024 - 16 * 1024 /* red */ - 4096 /* LUT */ - 1024 /* slack */;
inline void col16_split(int R, int K, int forced_ks, int& KS, int& kslice) {
    int kmax = (COL16_LDS_BUDGET / (R * 2) - 8) / 128 * 128;      // k per block whose R activation rows fit in LDS
    if (kmax < 128) kmax = 128;
    KS = (K + kmax - 1) / kmax;
    if (forced_ks > KS) KS = forced_ks;
    kslice = ((K + KS - 1) / KS + 127) / 128 * 128;
    KS = (K + kslice - 1) / kslice;
}

template <int DT, int NM, int LC, int PER>
int launch_gemv_col16_lc(const Problem& q, const GemvParams& gp) {
    dim3 grid((unsigned)((q.N + 15) / 16), (unsigned)gp.KS);
    const unsigned lds = 4096u * LC + (unsigned)gp.R * (unsigned)(gp.kslice * 2 + 16);
    auto kw = gemv_col16_kernel<DT, NM, true, LC, PER>;
    auto kd = gemv_col16_kernel<DT, NM, false, LC, PER>;
    static std::atomic<uint64_t> done_w{0}, done_d{0};
    if (!ensure_dyn_lds((const void*)(q.W ? kw : kd), 160 * 1024 - 16 * 1024 - 256, q.W ? done_w : done_d)) return BD_E_LAUNCH;
    if (q.W) hipLaunchKernelGGL(kw, grid, dim3(512), lds, q.st, gp);
    else hipLaunchKernelGGL(kd, grid, dim3(512), lds, q.st, gp);
    return BD_OK;
}

template <int DT, int NM, int LC>
int launch_gemv_col16_per(const Problem& q, const GemvParams& gp) {
    // every wave owns exactly 4 whole iterations (one slice of K = 4096): the straight-line, everything-in-flight instantiation
    // (measured, `bd_harness dec500`: -3..7 % for delta-only launches, but +7..13 % SLOWER for fused ones -> delta-only only)
    const bool per4 = gp.KS == 1 && q.K == 4096 && !q.W && !g_col16_no_per4;
    return per4 ? launch_gemv_col16_lc<DT, NM, LC, 4>(q, gp) : launch_gemv_col16_lc<DT, NM, LC, 0>(q, gp);
}

template <int DT, int NM>
int launch_gemv_col16(const Problem& q, const GemvParams& gp) {
    // 16-copy conflict-free sign LUT when it fits next to the activation rows and there are masks enough to expand
    const bool want = g_col16_small_lut < 0 ? (q.W == nullptr) : (g_col16_small_lut == 0);
    const bool big = NM >= 2 && want && 65536 + (int64_t)gp.R * (gp.kslice * 2 + 16) <= 160 * 1024 - 16 * 1024 - 256 &&
                     (g_col16_small_lut == 0 || (q.N + 15) / 16 <= num_cus());      // auto: only when one block per CU covers N
    if constexpr (NM >= 2) { if (big) return launch_gemv_col16_per<DT, NM, 16>(q, gp); }
    return launch_gemv_col16_per<DT, NM, 1>(q, gp);
}

// what every decode kernel reads of the problem: one k slice, no split-k scratch (the split-k kernels set KS / kslice / ws / tickets themselves)
inline GemvParams gemv_params(const Problem& q) {
    GemvParams gp;
    gp.X = (const unsigned short*)q.A;
    gp.P = (const uint32_t*)q.P;
    gp.W = (const unsigned short*)q.W;
    gp.alpha = q.alpha;
    gp.C = q.C;
    gp.ws = nullptr; gp.tickets = nullptr;
    gp.B = q.B; gp.M = q.M; gp.N = q.N; gp.K = q.K; gp.R = q.B * q.M;
    gp.sXb = q.sAb; gp.sPb = q.sPb; gp.sCb = q.sCb;
    gp.sXm = (int)q.sAm; gp.sCm = (int)q.sCm; gp.ldw = (int)q.ldw; gp.sAlb = (int)q.sAlb; gp.gsz = q.N / q.G;
    gp.KS = 1; gp.kslice = q.K;
    gp.round_mode = q.round_mode; gp.accumulate = q.accumulate; gp.out_f32 = (q.out_dtype == BD_F32);
    return gp;
}

template <int DT>
int launch_gemv_col16_chunk(const Problem& q) {
    GemvParams gp = gemv_params(q);
    const int forced = (g_forced_variant > 500 && g_forced_variant <= 564) ? g_forced_variant - 500 : 0;
    col16_split(gp.R, q.K, forced, gp.KS, gp.kslice);
    if (gp.KS > 1) {
        const int64_t need = GEMV_TICKET_BYTES + (int64_t)gp.KS * gp.R * q.N * 4;
        if (!q.ws || q.ws_bytes < need) return BD_E_WORKSPACE;
        gp.ws = (float*)((char*)q.ws + GEMV_TICKET_BYTES);
    }
    for_bucket<1, 2, 3, 4, 6, 8, 12, 16>(q.sPb == 0 ? 1 : q.B, [&](auto NM) { launch_gemv_col16<DT, NM>(q, gp); });
    if (gp.KS > 1) {
        dim3 g2((unsigned)((q.N + 255) / 256), (unsigned)gp.R);
        hipLaunchKernelGGL((gemv_reduce_kernel<DT>), g2, dim3(256), 0, q.st, gp);
    }
    return launch_status();
}

// ---- streaming decode kernel (gemv_stream_kernel, variant 600): one 8-wave block per CU, contiguous column range per block
constexpr int STREAM_MIN_N = 512;
constexpr int STREAM_WT_NT_DEFAULT = 1;           // (-3.6 % on the 6-tenant Mistral decode step, same process: profiles/r04_decode_ab.txt)
constexpr int STREAM_FG_DEFAULT = 1;              // fine grid (single-tile blocks, two per CU) where the tile count is between one and two per CU
constexpr int STREAM_XRES_DEFAULT = 1;            // activation rows resident in LDS + deeper prefetch (XL = 2) where the rule below says so
// (STREAM_WT_NT_DEFAULT: non-temporal policy on the tile-major weight loads of the streaming kernel)
inline bool stream_ok(const Problem& q, int rows, int nmask) {
    if (rows > GEMV_MAX_R || nmask > (q.mask_tiled == 2 ? 16 : 8) || q.N < STREAM_MIN_N) return false;
    // 32-bit buffer offsets with an out-of-range sentinel at 2 GiB: every extent must stay below it
    const int64_t lim = (1ll << 31) - 64;
    const int64_t xb = ((int64_t)(q.B - 1) * q.sAb + (int64_t)(q.M - 1) * q.sAm + q.K) * 2;
    const int64_t wb = q.W ? ((int64_t)(q.N - 1) * q.ldw + q.K) * 2 : 0;
    const int64_t pb = q.mask_tiled == 2 ? (int64_t)((q.N + 15) / 16) * ((q.K + 127) / 128) * 4 * 16 * q.t_pad * 4
                                         : ((int64_t)(nmask - 1) * q.sPb + (int64_t)(q.K / 32) * ((q.N + 15) / 16 * 16)) * 4;
    return xb > 0 && xb < lim && wb < lim && pb < lim && q.sAb >= 0 && q.sAm >= 0;
}

constexpr int STREAM_LDS_MAX = 160 * 1024;        // LDS of a gfx950 CU: the fused-norm kernels add R activation rows to STREAM_LDS_BYTES

// ---- which gemv_stream_kernel serves a launch.  The DECISION (stream_plan, below: plain host code, no HIP call) and the LAUNCH
// (launch_stream) are separate: every form of this Linear produces the same bits by design, so a launch that took the wrong prefetch depth,
// cache policy or grid would only be slower and no output test could see it -- the plan is what the host tests pin (bd_last_decode_plan,
// tests/golden/stream_dispatch.txt), and the set of compiled kernels is stream_shipped() and nothing else (tests/golden/stream_kernel_forms.txt).
// The kernel's twelve template parameters as run-time values (-1 = not decided yet), in the order they are lifted to template arguments -- which is
// the kernels' order in the code object: NM early keeps one step's forms neighbours (0.9 % of the step, profiles/decode_dispatch_refactor.txt)
struct StreamForm {
    int DT = -1, PK = -1, WT = -1, NM = -1, XL = -1, FG = -1, HASW = -1, WNAT = -1, AUX = -1, EPI = -1, NS = -1, NW = -1;
};
template <int... Vs> struct Vals {};
// the values each parameter can take, in StreamForm's order (FG 2, AUX 6, NS 12 and NW 8: harness builds, -DBD_AB_VARIANTS)
using StreamAxes = std::tuple<Vals<DT_F16, DT_BF16>, Vals<0, 1>, Vals<0, 1, 2, 3>, Vals<0, 1, 2, 3, 4, 6, 8, 12, 16>, Vals<0, 1, 2, 3>, Vals<0, 1, 2>,
                              Vals<0, 1>, Vals<0, 1>, Vals<0, 2, 6>, Vals<0, 1>, Vals<2, 3, 4, 6, 8, 12>, Vals<4, 8>>;
constexpr int STREAM_FORM_FIELDS = std::tuple_size_v<StreamAxes>;
#ifdef BD_AB_VARIANTS
constexpr bool STREAM_AB = true;
#else
constexpr bool STREAM_AB = false;
#endif

// NS = stages of loads in flight per wave: a function of the sign layout, the activation source, the mask count and the weight format, nothing else.
constexpr int stream_depth(int PK, int XL, int NM, int WT) {
    // reference / tile-major sign layouts (and bd_tenant_linear, NM = 0; NS 6 / 4 measured equal or slower there): bounded by the 256-VGPR
    // budget of a 2-waves-per-SIMD block (hipcc spills beyond)
    if (!PK) return NM <= 1 ? 8 : NM == 2 ? 6 : 4;
    // Prefetch depth of the int8 forms: a stage carries HALF the weight bytes, and what saturates HBM is bytes in flight per wave, not stages.
    // With one or two tenants the int8 launches ran latency-bound at the 16-bit depths and twice the stages put the same bytes in flight
    // (1 tenant, gate|up 31.3 -> 26.8 us, step 2.55 -> 2.31 ms); from 4 tenants on the sign work bounds the stage, the deeper queue only adds
    // latency (6 tenants: q|k|v 17.4 -> 18.8 us, o 13.0 -> 14.1) and the norm-prologue form spills: same depth as 16 bits
    // (rocprofv3 kernel traces, profiles/w8_decode_step.txt).
    // The 4-bit forms follow the same rule with a QUARTER of the weight bytes per stage: one or two tenants run four times the 16-bit depth where
    // the activation rows are resident (a stage is 3 loads: nibbles, group parameters, signs -- 8 stages keep 21 loads in flight, far inside the
    // 6-bit vmcnt) and twice where every stage also loads its four activation fragments (7 loads per stage: 4 x 3 stages would need 77 counts);
    // from 4 tenants on the 16-bit depth, for int8's measured reason.
    const bool few = WT >= 2 && NM <= 2;
    // Resident rows, hand-off consumer, norm prologue: TWO stages.  Same-process A/Bs of the whole step late in round 4
    // (profiles/r04_decode_step_ab.txt): 8 -> 6 -> 4 -> 2 stages each made the step faster (1 tenant: 3.57 -> 3.32 ms over the whole sequence
    // of changes; 6 tenants: -0.3 % for the resident-row form alone; gate|up with its norm at 2 instead of 4 stages: -1 % on the whole step) --
    // the memory system is saturated by far fewer loads in flight than the register file can hold, and beyond that point a deeper queue only
    // adds latency (returns are in issue order).  (The parity of NS selects the activation fragment set, so 2 is the minimum.)
    if (XL) return few ? (WT == 3 ? 8 : 4) : 2;
    // plain / SwiGLU-only forms: 1 tenant 3 stages (8 until late in round 4: -6 % on the single-delta step over 8 -> 6 -> 4 -> 3), 2 tenants 4
    // (6: +3 %), 4 and more 4 (3 measured +0.6 % at 6 tenants; NS 6 with nt weight loads measured 5-14 % slower: tools/ab_decode_depth.py)
    return (NM == 1 ? 3 : 4) * (few ? 2 : 1);
}

// The instantiations the library ships.  Fields are decided in StreamForm's order: a rule on a field reads only the fields before it (a later one
// is still -1), and a form whose decided fields already break a rule is out, whatever follows (the lifter below stops there).
// Per dtype 296: reference layout 12 (6 mask counts, fused / delta only) + 3 bd_tenant_linear; packed with row-major W 29 (5 delta only, 7 plain, 7 SwiGLU,
// 10 norm); per tile-major format 84 = 28 per-stage (7 paddings x SwiGLU x nt) + 20 norm (5 x 2 x 2) + 36 resident / hand-off (2 x 2 x (5 + 4 fine grid)).
constexpr bool stream_shipped(const StreamForm& f) {
    const bool nm8 = f.NM == 1 || f.NM == 2 || f.NM == 4 || f.NM == 6 || f.NM == 8;                  // packed layout: tenants padded to ...
    const bool ref = !f.PK && !f.WT && !f.XL && !f.FG;
    // harness builds add the bd_set_stream_tuning bits 0-3 matrix (fp16, fused, 0 / 1 / 6 masks: W order x nt policy x 8-wave blocks x deeper
    // prefetch) and the two-pass resident rows (FG = 2: 4 / 6 tenants, 2 or 4 stages)
    const bool ab = STREAM_AB && ref && f.DT == DT_F16 && f.HASW != 0 && (f.NM == 0 || f.NM == 1 || f.NM == 6);
    if (f.WT > 0 && !f.PK) return false;                                   // tile-major W: packed signs only
    if (f.NM >= 0 && !(f.PK ? (nm8 || f.NM == 12 || f.NM == 16) : (f.NM <= 4 || f.NM == 6 || f.NM == 8))) return false;   // (0 = bd_tenant_linear)
    // norm prologue: packed; resident rows / hand-off: tile-major W; 9 .. 16 tenants: plain / SwiGLU only; fine grid: resident rows, <= 6 tenants
    if (f.XL > 0 && !(f.PK && (f.WT || f.XL == 1) && nm8)) return false;
    if (f.FG > 0 && !(f.XL >= 2 && ((f.FG == 1 && f.NM <= 6) || (STREAM_AB && f.FG == 2 && f.WT == 1 && f.XL == 2 && (f.NM == 4 || f.NM == 6))))) return false;
    if (f.HASW == 0 && !(f.NM >= 1 && f.NM <= 8 && !f.WT && !f.XL)) return false;           // delta only: no fused form
    if (f.WNAT >= 0 && f.WNAT != f.PK && !(ref && f.NM == 0 && f.HASW) && !ab) return false;           // natural-order W off the packed layout
    if (f.AUX > 0 && !(f.AUX == 2 && (f.PK ? f.WT != 0 : (f.NM == 0 && f.WNAT == 1))) && !(ab && f.AUX == 6)) return false;   // nt loads
    if (f.AUX == 0 && f.XL >= 2) return false;                            // (the resident-row forms have no default-policy twin)
    if (f.EPI > 0 && !(f.PK && f.HASW && f.FG != 2)) return false;        // SwiGLU: packed, fused
    const int depth = stream_depth(f.PK, f.XL, f.NM, f.WT);
    const bool abm = ab && f.AUX != 2;                     // (the matrix: AUX 0 / 6)
    if (f.NS >= 0 && f.NS != depth && !(abm && (2 * f.NS == depth || 4 * f.NS == 3 * depth || 2 * f.NS == 3 * depth)) &&
        !(f.FG == 2 && f.NS == 4)) return false;
    if (f.NW >= 0 && f.NW != (abm && f.NS < depth ? 8 : 4)) return false;            // (8-wave blocks run half the stages per wave)
    return true;
}

// What stream_plan decides about one launch; bd_last_decode_plan reports it field by field.
struct StreamPlan {
    int rc = BD_OK;                    // != BD_OK: the launch is refused
    StreamForm f;
    unsigned grid = 0, grid_y = 1;     // (grid_y: bd_tenant_linear's tenants)
    int block = 0, lds = 0;            // threads per block, dynamic LDS bytes
    int cpb = 0; uint32_t xs_off = 0, xrow = 0;      // StreamParams::cpb / xs_off / xrow
    int form = 0;                      // bd_last_decode_form: 0 = one block per CU, 1 = fine grid, 2 = two-pass resident rows (harness builds)
#ifdef BD_AB_VARIANTS
    bool ring = false;                 // handed over to the loader / consumer kernel (variant 700)
#endif
};
static thread_local StreamPlan t_last_plan;         // of this thread's last streaming decode launch or dry run
static thread_local int g_decode_dry_run = 0;       // bd_set_decode_dry_run: plan and record, never touch the device

// block size and dynamic LDS of the planned form; refuses what does not fit
inline void stream_plan_lds(StreamPlan& pl, int R) {
    const StreamForm& f = pl.f;
    const int base = f.FG ? STREAM_FG_XS_OFF : STREAM_LDS_BYTES;
    pl.block = 64 * f.NW;
    pl.lds = f.XL ? std::max((int)(pl.xs_off + (uint32_t)R * pl.xrow), base) : base;
    if (pl.lds > (f.FG == 1 ? STREAM_FG_LDS_MAX : STREAM_LDS_MAX)) pl.rc = BD_E_BAD_SHAPE;
}

template <int DT, int NM, bool HASW, int NS, int NW, int WNAT, int AUX, int PK, int XL, int EPI, int WT, int FG>
int launch_stream_inst(const StreamPlan& pl, const StreamParams& sp, hipStream_t st) {
    if (g_decode_dry_run) return BD_OK;
    auto kern = gemv_stream_kernel<DT, NM, HASW, NS, NW, WNAT, AUX, PK, XL, EPI, WT, FG>;
    static std::atomic<uint64_t> lds_done{0};
    if (!ensure_dyn_lds((const void*)kern, FG == 1 ? STREAM_FG_LDS_MAX : XL ? STREAM_LDS_MAX : STREAM_LDS_BYTES, lds_done)) return BD_E_LAUNCH;
    hipLaunchKernelGGL(kern, dim3(pl.grid, pl.grid_y), dim3(pl.block), pl.lds, st, sp);
    return BD_OK;
}

// Lifts the run-time values of a form to template arguments, one field per level: a fold over the field's value list compares and recurses.
// A prefix that stream_shipped() rules out ends there, so exactly the shipped forms are instantiated; anything else answers BD_E_BAD_SHAPE.
template <int... Done>
struct StreamLift {
    static int run(const int* want, const StreamPlan& pl, const StreamParams& sp, hipStream_t st) {
        constexpr StreamForm f{Done...};
        if constexpr (!stream_shipped(f)) return BD_E_BAD_SHAPE;
        else if constexpr (sizeof...(Done) == STREAM_FORM_FIELDS)
            return launch_stream_inst<f.DT, f.NM, f.HASW != 0, f.NS, f.NW, f.WNAT, f.AUX, f.PK, f.XL, f.EPI, f.WT, f.FG>(pl, sp, st);
        else return next(std::tuple_element_t<sizeof...(Done), StreamAxes>{}, want, pl, sp, st);
    }
    template <int... Vs>
    static int next(Vals<Vs...>, const int* want, const StreamPlan& pl, const StreamParams& sp, hipStream_t st) {
        int rc = BD_E_BAD_SHAPE;      // (a value outside the list)
        (void)((want[sizeof...(Done)] == Vs && ((rc = StreamLift<Done..., Vs>::run(want, pl, sp, st)), true)) || ...);
        return rc;
    }
};

// The one launcher of gemv_stream_kernel: records the plan, launches it unless this is a dry run, answers the launch status.
inline int launch_stream(StreamPlan pl, const StreamParams& sp, hipStream_t st) {
    const StreamForm& f = pl.f;
    const int want[STREAM_FORM_FIELDS] = {f.DT, f.PK, f.WT, f.NM, f.XL, f.FG, f.HASW, f.WNAT, f.AUX, f.EPI, f.NS, f.NW};
    if (pl.rc == BD_OK) pl.rc = StreamLift<>::run(want, pl, sp, st);
    t_last_plan = pl;
    if (pl.rc != BD_OK || g_decode_dry_run) return pl.rc;
    return launch_status();
}

#ifdef BD_AB_VARIANTS
// ---- loader / consumer decode kernel (gemv_ring_kernel, variant 700): packed sign layout, fused Linear, K % 128 == 0
constexpr int DECODE_ENGINE_DEFAULT = 0;          // what packed-layout decode launches run when nobody called bd_set_decode_engine
constexpr int RING_TUNE_DEFAULT = 1;              // nt streams, resident activations when they fit, as many slots as fit
inline bool ring_wanted() {
    if (g_forced_variant == 700) return true;
    if (g_forced_variant >= 0) return false;
    return (g_decode_engine < 0 ? DECODE_ENGINE_DEFAULT : g_decode_engine) == 1;
}
// fills the LDS geometry of `rp`; false when the launch does not fit the kernel's envelope (the caller falls back to variant 600,
// or answers BD_E_BAD_SHAPE when 700 was forced)
inline bool ring_plan(const Problem& q, RingParams& rp) {
    const int tune = g_ring_tune < 0 ? RING_TUNE_DEFAULT : g_ring_tune;
    if (!q.W || q.mask_tiled != 2) return false;
    rp.epi = q.epilogue == 1;
    rp.nw = (const unsigned short*)q.norm_w; rp.sNw = q.sNw; rp.eps = q.eps;
    return ring_plan_geometry(rp, q.B * q.M, q.K, q.t_pad, q.w_tiled != 0, q.ldw, q.norm_w != nullptr, tune);
}
template <int DT, int NM, int NT>
int launch_ring_inst2(const RingParams& rp, unsigned grid, hipStream_t st) {
    auto kern = gemv_ring_kernel<DT, NM, NT>;
    static std::atomic<uint64_t> lds_done{0};
    if (!ensure_dyn_lds((const void*)kern, RING_LDS_MAX, lds_done)) return BD_E_LAUNCH;
    const unsigned lds = ring_lds_bytes(rp);
    if (lds > (unsigned)RING_LDS_MAX) return BD_E_BAD_SHAPE;
    hipLaunchKernelGGL(kern, dim3(grid), dim3(64 * (4 + rp.nl)), lds, st, rp);
    return BD_OK;
}
template <int NM>
int launch_ring_inst(int dtype, const RingParams& rp, unsigned grid, hipStream_t st) {
    if (dtype == BD_BF16) return rp.nt ? launch_ring_inst2<DT_BF16, NM, 1>(rp, grid, st) : launch_ring_inst2<DT_BF16, NM, 0>(rp, grid, st);
    return rp.nt ? launch_ring_inst2<DT_F16, NM, 1>(rp, grid, st) : launch_ring_inst2<DT_F16, NM, 0>(rp, grid, st);
}

#endif

// Harness builds (STREAM_AB): bd_set_stream_tuning bits 0-3, the A/B matrix of the reference-layout forms (fp16, fused, 0 / 1 / 6 masks): bit 0
// natural-order W, bit 1 nt cache policy, bit 2 8-wave blocks (two waves per SIMD, half the stages each), bit 3 the deeper prefetch (x 1.5)
inline void stream_plan_tuned(StreamForm& f) {
    const int t = g_stream_tune & 15;
    if (f.DT != DT_F16 || !f.HASW || !(f.NM == 0 || f.NM == 1 || f.NM == 6)) return;
    f.WNAT = t & 1; f.AUX = (t & 2) ? 6 : 0; f.NW = (t & 4) ? 8 : 4;
    f.NS = f.NS * ((t & 8) ? 3 : 2) / ((t & 4) ? 4 : 2);
}

// The decision.  Reads the problem, the CU count and this thread's tuning state (forced variant, bd_set_stream_tuning); makes no HIP call.
// q.w_tiled is the weight format: 0 row-major, 1 tile-major, 2 = the int8 tile-major copy of bd_binary_linear_decode_w8, 3 = the 4-bit GPTQ copy
// of bd_binary_linear_decode_q4 -- the same rules for all of them, the kernel's WT.
StreamPlan stream_plan(const Problem& q, int cus) {
    StreamPlan pl;
    StreamForm& f = pl.f;
    f.DT = q.dtype == BD_BF16 ? DT_BF16 : DT_F16;
    f.PK = q.mask_tiled == 2; f.WT = q.w_tiled; f.XL = 0; f.FG = 0;
    f.HASW = q.W != nullptr; f.WNAT = f.PK; f.AUX = 0; f.EPI = f.PK && q.epilogue == 1; f.NW = 4;
    const int nmask = q.sPb == 0 ? 1 : q.B;
    // columns per block: the whole chip streams one launch, so every CU gets ~N / CUs columns (rounded up to whole sign-word
    // quads); a few more blocks than CUs would serialise a second, nearly empty round
    int cpb = (q.N + cus - 1) / cus;
    cpb = (cpb + 3) & ~3;
    if (cpb < 4) cpb = 4;
    if (g_forced_variant > 600 && g_forced_variant <= 664) cpb = 4 * (g_forced_variant - 600);     // test hook: 600 + cpb/4
    if (q.epilogue == 1 || q.ssq_out) cpb = (cpb + 15) & ~15;      // whole [8 gate | 8 up] tiles / whole hand-off tiles per block
    pl.cpb = cpb;
    pl.grid = (unsigned)((q.N + cpb - 1) / cpb);
    pl.xs_off = (uint32_t)STREAM_XS_OFF; pl.xrow = (uint32_t)q.K * 2u + 16u;
    if (!f.PK) {
        // reference / tile-major sign layouts: accumulator sets = distinct masks (extra sets of a bucket repeat the last mask)
        // Shipped configuration (profiles/r02_decode_stream_ab.txt): 4-wave blocks (one wave per SIMD, the whole register file: NS stages
        // of loads in flight per wave), word-row order for W, default cache policy.
        f.NM = nmask <= 4 ? (nmask < 1 ? 1 : nmask) : nmask <= 6 ? 6 : 8;
        f.NS = stream_depth(f.PK, f.XL, f.NM, f.WT);
        if (STREAM_AB) stream_plan_tuned(f);
        stream_plan_lds(pl, q.B * q.M);
        return pl;
    }
    // packed layout: all tenants of the call in one chunk, interleaved
    // kernel kinds: plain | RMSNorm prologue (XL) | XL + SwiGLU epilogue | SwiGLU epilogue only; each with row-major or tile-major W (WT)
    f.NM = q.t_pad;
#ifdef BD_AB_VARIANTS
    if (ring_wanted() && q.w_tiled <= 1) {      // loader / consumer kernel (variant 700); launches outside its envelope stay on the streaming kernel
        RingParams rp{};
        if (ring_plan(q, rp)) { pl.ring = true; return pl; }
        if (g_forced_variant == 700) { pl.rc = BD_E_BAD_SHAPE; return pl; }
    }
#else
    if (g_forced_variant == 700) { pl.rc = BD_E_BAD_SHAPE; return pl; }      // harness-only kernel (round 4 A/B loser): never silently replaced
#endif
    // tile-major W: optional nt policy on the weight loads (STREAM_WT_NT_DEFAULT, or bd_set_stream_tuning bit 4 = on / bit 5 = off)
    const bool wnt = (g_stream_tune & 16) ? true : (g_stream_tune & 32) ? false : (STREAM_WT_NT_DEFAULT != 0);
    // ... and optionally the activation rows resident in LDS with a deeper weight prefetch (XL = 2; bd_set_stream_tuning bit 6 = on,
    // bit 7 = off): plain and SwiGLU launches with M = 1 and R * K <= 32768
    // (any K: tile-major W already needs K % 128 == 0; the norm prologue keeps its power-of-two rule, this form does not need it)
    // Every wave must own at least one 128-k iteration: a wave with an empty k range still walks one padded stage per tile, whose
    // zero sign words expand to -1 fragments -- harmless against the zero activation fragments of the per-stage form, NOT against
    // fragments read from the resident rows (K = 1152: 9 iterations over 4 waves leave the last wave empty).
    const int nit_x = (q.K + 127) / 128;
    const bool xres_ok = q.w_tiled && (!q.norm_w || q.ssq_in) && q.M == 1 && q.t_pad <= 8 && q.K >= 1024 && 3 * ((nit_x + 3) / 4) < nit_x &&
                         (int64_t)q.B * q.K <= 16 * 2048 &&
                         (int64_t)STREAM_XS_OFF + (int64_t)q.B * (2 * (int64_t)q.K + 16) <= STREAM_LDS_MAX;
    // Fine grid (FG, round 6; gemv_stream_kernel): a resident-row launch whose 16-column tiles number between one and two per CU --
    // Mistral's fused q|k|v: 384 tiles -- runs as ONE round of single-tile blocks, two per CU (<= 80 KB of LDS with the nibble sign table,
    // <= 256 VGPRs), instead of 256 blocks that walk 1.5 tiles each.  bd_set_stream_tuning: 256 = never, 512 = every eligible launch
    // with at most two tiles per CU (one tile per CU included: the o projection).
    const int fg_tiles = q.N / 16;
    const bool fg_ok = xres_ok && q.N % 16 == 0 && q.t_pad <= 6 && fg_tiles <= 2 * cus &&
                       (int64_t)STREAM_FG_XS_OFF + (int64_t)q.B * (2 * (int64_t)q.K + 16) <= STREAM_FG_LDS_MAX;
    // Default: resident rows wherever they apply.  (Until the prefetch depths came down to 2 stages this form lost on short launches -- at 6
    // stages the 4096 x 4096 o projection of a 6-tenant step was +25 % -- and was dispatched by size; at 2 stages it wins on every eligible
    // launch: 6 tenants 4.805 -> 4.770 ms per step with o included, profiles/r04_decode_step_ab.txt.)  The hand-off consumer needs them
    // whatever the flags say.
    const bool xres_auto = STREAM_XRES_DEFAULT != 0;
    const bool xres = xres_ok && ((g_stream_tune & 64) ? true : (g_stream_tune & 128) ? false : xres_auto);
    // The fine grid is a resident-row form: decided only for launches that take one (the consumer or `xres`), so a launch that falls
    // through to the per-stage forms below keeps its own column split (cpb) and LDS layout.
    const bool fg = fg_ok && (q.ssq_in || xres) && !(g_stream_tune & 256) &&
                    ((g_stream_tune & 512) ? true : (STREAM_FG_DEFAULT != 0 && fg_tiles > cus));
    // Two-pass resident rows (FG = 2, round 6; gemv_stream_kernel): rows that do not fit LDS at once -- the down projection of a multi-tenant
    // step, 6 x 14336 -- with ONE tile per block, every wave's k quarter cut in two halves.  Bit-identical to the per-stage-load form and
    // SLOWER (down 33.0 -> 37.1 us at 2 stages of prefetch, 40.0 at 4; step +4 ... +6 %: profiles/r06_decode_step.txt), so like every A/B
    // loser it exists in harness builds only (-DBD_AB_VARIANTS; bd_set_stream_tuning 8192 = on, + 16384 = 2 stages instead of 4).
#ifdef BD_AB_VARIANTS
    const bool fg2 = (g_stream_tune & 8192) && q.w_tiled == 1 && !q.norm_w && !q.ssq_in && q.epilogue == 0 && q.M == 1 && q.t_pad <= 8 && q.N % 16 == 0 &&
                     fg_tiles <= cus && q.K % 1024 == 0 && q.K >= 8192 && (int64_t)q.B * q.K > 16 * 2048 && (int64_t)q.B * (q.K / 2) <= 24 * 2048 &&
                     (int64_t)STREAM_FG_XS_OFF + (int64_t)q.B * ((int64_t)q.K + 16) <= STREAM_LDS_MAX;
    if (fg2) {
        f.XL = 2; f.FG = 2; f.AUX = 2; f.NS = (g_stream_tune & 16384) ? 2 : 4;
        pl.cpb = 16; pl.grid = (unsigned)fg_tiles; pl.xs_off = (uint32_t)STREAM_FG_XS_OFF; pl.xrow = (uint32_t)q.K + 16u;
        pl.form = 2;
        stream_plan_lds(pl, q.B * q.M);
        return pl;
    }
#endif
    if (q.ssq_in && !xres_ok) { pl.rc = BD_E_BAD_SHAPE; return pl; }
    if (q.ssq_in || xres) {
        // resident rows (XL = 2), or RMSNorm by hand-off (XL = 3): the resident-row form with the rows pre-multiplied by the norm weight and
        // the row scale in the epilogue; same envelope as the resident rows, nothing else implements it
        // (A/B, not shipped: the short 6-tenant launches -- q|k|v, o -- on 8-wave blocks, half the stages per wave, are 1 % faster on the
        //  step, 4.688 -> 4.639 ms, but 8 partial sums in another order are no longer bit-identical to every other form of the Linear:
        //  profiles/r04_decode_step_ab.txt.  The kernel template still takes NW = 8 with XL = 2.)
        f.XL = q.ssq_in ? 3 : 2; f.AUX = 2;
        if (fg) { f.FG = 1; pl.cpb = 16; pl.grid = (unsigned)fg_tiles; pl.xs_off = (uint32_t)STREAM_FG_XS_OFF; pl.form = 1; }
    } else {
        f.XL = q.norm_w ? 1 : 0;
        f.AUX = (q.w_tiled && wnt) ? 2 : 0;
    }
    f.NS = stream_depth(f.PK, f.XL, f.NM, f.WT);
    stream_plan_lds(pl, q.B * q.M);
    return pl;
}

int launch_gemv_stream_chunk(const Problem& q) {
    StreamParams sp{};
    sp.wscale = q.wscale;
    if (q.w_tiled == 3) {
        const uint32_t m = (uint32_t)(q.q4_group / 128);
        sp.q4p = q.q4p;
        sp.q4_ngrp = (uint32_t)(q.K / q.q4_group);
        sp.q4_bytes = (uint32_t)((int64_t)(q.N / 16) * sp.q4_ngrp * 64);
        sp.q4_magic = m > 1 ? (uint32_t)((1ull << 32) / m) + 1u : 0u;
    }
    sp.g = gemv_params(q);
    const int nmask = q.sPb == 0 ? 1 : q.B;
    const StreamPlan pl = stream_plan(q, num_cus());
    sp.cpb = pl.cpb; sp.xs_off = pl.xs_off; sp.xrow = pl.xrow;
    sp.pts = q.mask_tiled == 1 ? 16u * (uint32_t)(q.K / 32) : 16u;
    sp.prs = q.mask_tiled == 1 ? 16u : (uint32_t)q.N;
    sp.tp = (uint32_t)q.t_pad;
    sp.nw = (const unsigned short*)q.norm_w; sp.sNw = q.sNw; sp.eps = q.eps;
    sp.ssq_in = q.ssq_in; sp.ssq_out = q.ssq_out;
    sp.ssq_scale = (q.ssq_out && q.eps > 0.f) ? q.eps : 1.f;      // producer launches: the `eps` slot of the entry point carries the factor (header)
    sp.nw_next = (const unsigned short*)q.nw_next; sp.sNwNext = q.sNwNext; sp.xw_out = (unsigned short*)q.xw_out;
    sp.no_res_prefetch = (g_stream_tune & 1024) ? 1 : 0;
    sp.n_bytes = q.norm_w ? (uint32_t)(((int64_t)(q.B - 1) * q.sNw + q.K) * 2) : 0u;
    sp.jsh = 0;
    while ((2048 << sp.jsh) < q.K) ++sp.jsh;
    sp.x_bytes = (uint32_t)(((int64_t)(q.B - 1) * q.sAb + (int64_t)(q.M - 1) * q.sAm + q.K) * 2);
    sp.w_bytes = q.W ? (uint32_t)(((int64_t)(q.N - 1) * q.ldw + q.K) * 2) : 0u;
    if (q.w_tiled)       // tile-major W: [N/16][K/128] blocks of 4 KiB (int8: 2 KiB, 4-bit: 1 KiB)
        sp.w_bytes = (uint32_t)((int64_t)((q.N + 15) / 16) * ((q.K + 127) / 128) * (q.w_tiled == 3 ? 1024 : q.w_tiled == 2 ? 2048 : 4096));
    sp.p_bytes = (uint32_t)(((int64_t)(nmask - 1) * q.sPb + (int64_t)(q.K / 32) * (q.mask_tiled ? (q.N + 15) / 16 * 16 : q.N)) * 4);
    if (q.mask_tiled == 2)      // packed layout: extent from the pack's own geometry
        sp.p_bytes = (uint32_t)((int64_t)((q.N + 15) / 16) * ((q.K + 127) / 128) * 4 * 16 * q.t_pad * 4);
#ifdef BD_AB_VARIANTS
    if (pl.ring) {
        t_last_plan = pl;
        if (g_decode_dry_run) return BD_OK;
        RingParams rp{};
        rp.g = sp.g; rp.cpb = pl.cpb;
        ring_plan(q, rp);
        int rrc = BD_OK;
        for_bucket<1, 2, 4, 6, 8>(q.t_pad, [&](auto NM) { rrc = launch_ring_inst<NM>(q.dtype, rp, pl.grid, q.st); });
        if (rrc != BD_OK) return rrc;
        t_last_variant = 700;
        return launch_status();
    }
#endif
    return launch_stream(pl, sp, q.st);
}

// batches of more than 16 activation rows run as consecutive launches over chunks of floor(16 / M) batch entries (each chunk streams
// the base weight again; still far cheaper than M = 1 tiles of the MFMA tile kernels, which re-read it once per batch entry)
// ---- delta only, <= 16 activation rows per block, reference layout (delta_rows_kernel, bd_gemv_rows.h): the reference's published
//      binary_bmm (M = 1, one mask per batch entry) and binary_matmul (one mask, M <= 16) decode shapes
struct RowsPlan { int rpm, mc, cw; unsigned grid; };
inline bool rows_plan(const Problem& q, RowsPlan& pl) {
    if (q.W || q.alpha || q.accumulate || q.mask_tiled != 0 || q.M < 1 || q.M > 16 || q.sPb < 0) return false;
    if (q.N % 32 || q.K % 128 || q.sPb % 2 || q.sAb % 8 || q.sAm % 8 || q.sAb < 0 || q.sAm < 0 || !aligned16(q.A) || !aligned16(q.P)) return false;
    const int64_t lim = (1ll << 31) - 64;                       // 32-bit buffer offsets, out-of-range sentinel at 2 GiB
    const int nmask = q.sPb == 0 ? 1 : q.B;
    const int64_t xb = ((int64_t)(q.B - 1) * q.sAb + (int64_t)(q.M - 1) * q.sAm + q.K) * 2;
    const int64_t pb = ((int64_t)(nmask - 1) * q.sPb + (int64_t)(q.K / 32) * q.N) * 4;
    if (!(xb > 0 && xb < lim && pb > 0 && pb < lim)) return false;
    const int64_t cus = num_cus();
    if (q.sPb == 0) {                                            // one mask shared by every row: one chunk of B * M rows
        if ((int64_t)q.B * q.M > 16) return false;
        pl.rpm = q.B * q.M; pl.mc = 1;
    } else {
        pl.rpm = q.M;
        // two masks per block when that still gives every CU TWO blocks (<= 220 VGPRs, 66 KB of LDS at M = 1: they are co-resident and overlap
        // each other's start and end), one mask per block otherwise.  tools/bench_rows.py, us per launch at 1 / 2 / 4 masks per block:
        // B = 16, 4096^2 14.6 / 13.3 / 13.8; B = 8, 8192^2 23.1 / 18.8 / 21.6; B = 16, 8192^2 43.2 / 35.9 / 40.2; B = 8, 4096^2 8.2 / 8.7 / 12.9;
        // B = 4, 4096^2 6.1 / 7.9 / 12.1  (four masks per block -- 336 VGPRs, one block per CU -- stays behind the 804 test hook)
        pl.mc = (2 * q.M <= 16 && (int64_t)(q.N / 64) * ((q.B + 1) / 2) >= 2 * cus) ? 2 : 1;
    }
    if (g_forced_variant > 800 && g_forced_variant <= 804 && q.sPb != 0) pl.mc = g_forced_variant == 801 ? 1 : g_forced_variant == 802 ? 2 : 4;   // test hook
    { const int forced = (g_rows_tune >> 1) & 3; if (forced && q.sPb != 0) pl.mc = 1 << (forced - 1); }
    if (pl.mc * pl.rpm > 16) return false;
    const int64_t nch = q.sPb == 0 ? 1 : (q.B + pl.mc - 1) / pl.mc;
    // 64-column super-tiles (dwordx4 sign loads) when they give every CU a block, 32-column ones (dwordx2) otherwise
    pl.cw = (q.N % 64 == 0 && ((int64_t)(q.N / 64) * nch >= cus || (g_rows_tune & 32))) ? 4 : 2;
    if (g_rows_tune & 64) pl.cw = 2;
    if (pl.cw == 4 && (q.sPb % 4)) return false;
    if (pl.mc == 4 && pl.cw == 2) pl.cw = 4;                     // (the 804 hook keeps its one instantiation)
    if (pl.cw == 4 && q.N % 64) return false;
    pl.grid = (unsigned)((q.N / (16 * pl.cw)) * nch);
    return true;
}
// automatic choice: launches with enough blocks to occupy at least half of the chip; per-entry masks from 4 rows on, a shared mask always
// (tools/bench_rows.py, 800 against the streaming kernel, us: M = 1, one mask 5.4 vs 7.1 at 4096^2 and 7.5 vs 13.2 at 8192^2; M = 16 7.8 vs 9.4 and
// 12.2 vs 21.3; B = 2, M = 8 at 8192^2 10.1 vs 23.9 -- the streaming kernel re-reads all 16 activation rows for every 16-column tile)
inline bool rows_auto(const Problem& q) {
    RowsPlan pl;
    if ((g_rows_tune & 16) || !rows_plan(q, pl)) return false;
    const bool shared = q.sPb == 0 || q.B == 1;
    if (shared ? ((int64_t)q.B * q.M < g_rows_shared_min) : ((int64_t)q.B * q.M < 4)) return false;
    return (int64_t)pl.grid * 2 >= num_cus();
}
template <int DT, int MC, int CW>
int launch_rows_inst(const RowsParams& rp, int R, unsigned grid, hipStream_t st) {
    // 4 stages of loads per wave, nt policy on the sign loads (default policy and 2 stages measured within +-4 % of it, mixed signs:
    // tests/native/rows_bench.hip keeps those instantiations)
    auto kern = delta_rows_kernel<DT, MC, 4, 2, 0, CW>;
    static std::atomic<uint64_t> lds_done{0};
    const int lds = STREAM_LUT_BYTES + 4 * R * 16 * CW * 4;
    if (!ensure_dyn_lds((const void*)kern, STREAM_LUT_BYTES + 4 * 16 * 16 * CW * 4, lds_done)) return BD_E_LAUNCH;
    hipLaunchKernelGGL(kern, dim3(grid), dim3(256), lds, st, rp);
    return BD_OK;
}
template <int DT>
int launch_rows(const Problem& q) {
    RowsPlan pl;
    if (!rows_plan(q, pl)) return BD_E_BAD_SHAPE;
    RowsParams rp{};
    rp.X = (const unsigned short*)q.A; rp.P = (const uint32_t*)q.P; rp.C = q.C;
    rp.B = q.B; rp.M = q.M; rp.N = q.N; rp.K = q.K; rp.rpm = pl.rpm;
    rp.sXb = q.sAb; rp.sXm = q.sAm; rp.sPb = q.sPb; rp.sCb = q.sCb; rp.sCm = q.sCm;
    const int nmask = q.sPb == 0 ? 1 : q.B;
    rp.x_bytes = (uint32_t)(((int64_t)(q.B - 1) * q.sAb + (int64_t)(q.M - 1) * q.sAm + q.K) * 2);
    rp.p_bytes = (uint32_t)(((int64_t)(nmask - 1) * q.sPb + (int64_t)(q.K / 32) * q.N) * 4);
    rp.round_mode = q.round_mode; rp.out_f32 = (q.out_dtype == BD_F32);
    const int R = pl.mc * pl.rpm;
    int rc;
    if (pl.mc == 4) rc = launch_rows_inst<DT, 4, 4>(rp, R, pl.grid, q.st);
    else if (pl.mc == 2) rc = pl.cw == 4 ? launch_rows_inst<DT, 2, 4>(rp, R, pl.grid, q.st) : launch_rows_inst<DT, 2, 2>(rp, R, pl.grid, q.st);
    else rc = pl.cw == 4 ? launch_rows_inst<DT, 1, 4>(rp, R, pl.grid, q.st) : launch_rows_inst<DT, 1, 2>(rp, R, pl.grid, q.st);
    if (rc != BD_OK) return rc;
    t_last_variant = 800;
    return launch_status();
}

template <int DT>
int launch_gemv(const Problem& q, bool valu_form, bool col16 = false, bool stream = false) {
    const int cb = GEMV_MAX_R / q.M;
    auto one = [&](const Problem& c) {
        return stream ? launch_gemv_stream_chunk(c) : col16 ? launch_gemv_col16_chunk<DT>(c) : launch_gemv_chunk<DT>(c, valu_form);
    };
    if (q.B <= cb) return one(q);
    const int esz = q.out_dtype == BD_F32 ? 4 : 2;
    for (int b0 = 0; b0 < q.B; b0 += cb) {
        Problem c = q;
        c.B = q.B - b0 < cb ? q.B - b0 : cb;
        c.A = (const char*)q.A + (int64_t)b0 * q.sAb * 2;
        c.P = q.P + (int64_t)b0 * q.sPb;
        c.C = (char*)q.C + (int64_t)b0 * q.sCb * esz;
        if (q.alpha) c.alpha = q.alpha + (int64_t)b0 * q.sAlb;
        const int rc = one(c);
        if (rc != BD_OK) return rc;
    }
    return BD_OK;
}

template <int DT>
int launch_gemv_chunk(const Problem& q, bool valu_form) {
    GemvParams gp = gemv_params(q);
    gp.ws = (float*)q.ws;
    gemv_split(q, gp.KS, gp.kslice);
    if (gp.KS > 1) {
        const int64_t need = GEMV_TICKET_BYTES + (int64_t)gp.KS * gp.R * q.N * 4;
        if (!q.ws || q.ws_bytes < need) return BD_E_WORKSPACE;
        gp.ws = (float*)((char*)q.ws + GEMV_TICKET_BYTES);
        // in-launch reduction unless the tile count exceeds the ticket area or the two-launch form is forced (g_gemv_two_launch)
        if ((q.N + 63) / 64 <= GEMV_TICKET_BYTES / 4 && !g_gemv_two_launch) gp.tickets = (uint32_t*)q.ws;
    }
    if (valu_form) {
        // rows >= R are computed and discarded, so the buckets are kept fine-grained
        for_bucket<1, 2, 3, 4, 6, 8, 12, 16>(gp.R, [&](auto RMAX) { launch_gemv_valu<DT, RMAX>(q, gp); });
    } else {
        // accumulator sets = distinct masks (extra sets of a bucket repeat the last mask)
        for_bucket<1, 2, 3, 4, 6, 8, 12, 16>(q.sPb == 0 ? 1 : q.B, [&](auto NM) { launch_gemv_mfma<DT, NM>(q, gp); });
    }
    if (gp.KS > 1 && !gp.tickets) {
        dim3 g2((unsigned)((q.N + 255) / 256), (unsigned)gp.R);
        hipLaunchKernelGGL((gemv_reduce_kernel<DT>), g2, dim3(256), 0, q.st, gp);
    }
    return launch_status();
}


// ------------------------------------------------------------------ tile path: variants 0 - 21 and 100
// Dispatched like the decode Linear: tile_plan() decides (plain host code: variant, k slices, tail split, workspace, every launch's tiles, grid
// and LDS), TILE_ROWS says what each variant is and which calls it takes, and launch_tile_plan() lifts each planned launch to its Cfg type and
// issues it through one body.  bd_last_gemm_plan reports the plan; under bd_set_gemm_dry_run nothing below dispatch() touches the device.

// Schedules: 0 = single barrier per k-tile (bd_gemm_mfma.h; the small-M tiles), 1 = half-tile ping-pong (bd_gemm_pp.h), 2 = full-tile ping-pong
// (bd_gemm_pf.h; the shipped delta-only schedule), 3 = one-pass fused, two accumulator sets (bd_gemm_fx.h), 4 = four-wave persistent
// (bd_gemm_w4.h: grid = min(batch x tiles, CUs) workgroups of 256 threads, each walking its share of the (batch entry, tile) stream),
// 5 = the generic edge kernel (bd_gemm_generic.h: any alignment, any K % 32 == 0).
enum { S_SB = 0, S_PP = 1, S_PF = 2, S_FX = 3, S_W4 = 4, S_GEN = 5 };
enum { FUSED_ONLY = 1, DELTA_ONLY = 2, EITHER = 3 };
// W4Cfg OPT: LUT sign expansion (+1.5 % over VALU expansion, same box) + the k loop unrolled by four -- bit-identical outputs, -3.6 / -5.5 % cycles
// per k-tile, +0.6 % on the timed prefill step in a same-box A/B of two library builds; profiles/r05_w4_cycles.txt
constexpr int W4_OPT = 1 | 8192;

// One row per tile variant (fused 0 / 5 have rows of their own: other schedules than the delta-only ones): id, the calls it serves, what it
// takes (flags), schedule, tile rows x columns, wave rows, ring slots, the Cfg's OPT.
enum {
    T_F32 = 1,        // takes fp32 output
    T_RESIDUAL = 2,   // takes a fused call's residual epilogue (Y += ...; one-pass fused tiles only)
    T_SWIGLU = 4,     // requires Problem::epilogue == 1 (every other row requires 0)
    T_AB = 8,         // a rejected schedule kept as an A/B reference: compiled only with -DBD_AB_VARIANTS (the native harness), the shipped
                      // library answers BD_E_BAD_SHAPE
    T_PAIR = 16,      // pair tiles: two batch entries of <= 64 rows share one 128 x 128 tile and its W stream
    T_SPLIT = 32,     // k slices into fp32 slabs in the workspace + a reduce launch
};
struct TileRow {
    int id, who, flags, sched, bm, bn, wm, ns, opt;
    constexpr bool is(int flag) const { return (flags & flag) != 0; }
};
// The ORDER of the rows is the order in which the kernels are requested and so their order in the code object, which is worth time
// (profiles/prefill_dispatch_refactor.txt): a new row goes where its kernel should lie, not where its number would sort.
constexpr TileRow TILE_ROWS[] = {
    {0, DELTA_ONLY, T_F32, S_PF, 256, 256, 2, 4, 1},                      // full-tile ping-pong, LUT sign expansion
    {0, FUSED_ONLY, T_F32 | T_AB, S_PP, 256, 256, 2, 4, 2},               // two k loops over one accumulator set, 2-slot base ring
    {5, DELTA_ONLY, T_F32, S_PF, 256, 128, 2, 4, 0},
    {5, FUSED_ONLY, T_F32 | T_AB, S_PF, 256, 128, 2, 4, 0},
    {6, EITHER, T_F32 | T_AB, S_PP, 256, 256, 2, 4, 2},                   // half-tile ping-pong (A/B reference)
    {7, EITHER, T_F32 | T_AB, S_PP, 256, 128, 2, 4, 2},
    {4, EITHER, T_F32 | T_AB, S_SB, 256, 256, 2, 4, 0},                   // single-barrier 256x256 (A/B reference)
    {8, FUSED_ONLY, T_F32 | T_RESIDUAL, S_FX, 256, 128, 2, 3, 1},         // one-pass fused (profiles/r01_fx_vs_two_loop.txt)
    // split-k over blockIdx.y + reduce launch (forced: k slices from the rule, at least 2): TWO rows, the 64x128 tile up to 64 rows per mask
    // (half the MFMA / LDS work of a padded 128-row tile), then the 128x128 tile
    {10, FUSED_ONLY, T_F32 | T_SPLIT, S_FX, 64, 128, 2, 4, 1},
    {10, FUSED_ONLY, T_F32 | T_SPLIT, S_FX, 128, 128, 2, 4, 1},
    // 64x128: up to 64 rows per mask (multi-tenant prefill of short prompts, demo_backend.py:297-299: M = 64 x 6 tenants) -- the 128-row
    // tile does twice the MFMA and LDS work for rows that do not exist
    {11, FUSED_ONLY, T_F32 | T_RESIDUAL, S_FX, 64, 128, 2, 4, 1},
    {12, FUSED_ONLY, T_F32 | T_RESIDUAL, S_FX, 64, 256, 2, 3, 1},         // wide outputs / many tenants (see the rule)
    {16, FUSED_ONLY, T_F32 | T_RESIDUAL | T_PAIR, S_FX, 128, 128, 2, 4, 1},              // pair tiles (multi-tenant prefill of short prompts)
    {17, FUSED_ONLY, T_F32 | T_RESIDUAL | T_PAIR | T_SPLIT, S_FX, 128, 128, 2, 4, 1},    // ... + split-k (o / down of a 6-tenant request: 96 tiles on 256 CUs)
    // FOUR-WAVE pair tiles: one wave per SIMD, wave tile 64 x 64, persistent over (pair, column tile); 21 = with the SwiGLU epilogue (gate|up of a
    // multi-tenant request of short prompts, no [M, 2 I] round trip); 19 = + split-k: the stream runs over (pair, k slice, column tile), the
    // slices are whole, equal runs of k-tiles, the residual is added by the reduce launch
    {18, FUSED_ONLY, T_F32 | T_RESIDUAL | T_PAIR, S_W4, 128, 128, 2, 3, W4_OPT},
    {21, FUSED_ONLY, T_SWIGLU | T_PAIR, S_W4, 128, 128, 2, 3, W4_OPT},
    {20, FUSED_ONLY, T_F32 | T_RESIDUAL, S_W4, 128, 128, 2, 3, W4_OPT},   // ONE entry per tile (prompts of 65 .. 128 rows per tenant)
    {19, FUSED_ONLY, T_F32 | T_RESIDUAL | T_PAIR | T_SPLIT, S_W4, 128, 128, 2, 3, W4_OPT},
    {9, FUSED_ONLY, T_F32 | T_RESIDUAL, S_FX, 128, 128, 2, 4, 1},         // twice the tiles when 256x128 cannot fill the CUs (128 < M <~ 768)
    {13, DELTA_ONLY, T_F32, S_W4, 256, 256, 2, 3, W4_OPT},
    {14, FUSED_ONLY, T_F32 | T_RESIDUAL, S_W4, 256, 128, 2, 3, W4_OPT},   // (fp32 output: general-form epilogue only)
    {15, FUSED_ONLY, T_SWIGLU, S_W4, 256, 128, 2, 3, W4_OPT},             // 14 with the SwiGLU epilogue (8-interleaved gate|up pair, C has N/2 columns)
    {1, EITHER, T_F32, S_SB, 128, 256, 1, 4, 0},
    {2, EITHER, T_F32, S_SB, 64, 256, 1, 4, 0},
    {3, EITHER, T_F32, S_SB, 32, 256, 1, 4, 0},
    {100, EITHER, T_F32, S_GEN, 64, 64, 1, 0, 0},
};
constexpr int N_TILE_ROWS = sizeof(TILE_ROWS) / sizeof(TILE_ROWS[0]);
constexpr bool row_serves(const TileRow& r, bool fused) { return (r.who & (fused ? FUSED_ONLY : DELTA_ONLY)) && (STREAM_AB || !r.is(T_AB)); }
// which launches of a row exist: fp32 ones where it takes fp32 output, and a split row's tile launch writes fp32 slabs whatever the output is
constexpr bool row_launches(const TileRow& r, bool fused, bool f32) { return row_serves(r, fused) && (f32 ? r.is(T_F32) : !r.is(T_SPLIT)); }
inline int tile_row(int id, bool fused) {
    for (int i = 0; i < N_TILE_ROWS; ++i)
        if (TILE_ROWS[i].id == id && row_serves(TILE_ROWS[i], fused)) return i;
    return -1;
}

template <int DT_, bool FUSED_, bool OUT_F32_>
struct GenericCfg {
    static constexpr int DT = DT_, BM = 64, BN = 64, NT = 256, LDS_BYTES = 0;
    static constexpr bool FUSED = FUSED_, OUT_F32 = OUT_F32_;
};
template <int I, int DT, bool FUSED, bool F32>
struct RowCfg {
    static constexpr TileRow r = TILE_ROWS[I];
    static constexpr int epi = r.is(T_SWIGLU) ? 1 : 0, pair = r.is(T_PAIR) ? 1 : 0;
    using type = std::conditional_t<r.sched == S_W4, W4Cfg<DT, r.bm, r.bn, FUSED, F32, r.opt, epi, pair>,
                 std::conditional_t<r.sched == S_FX, FxCfg<DT, r.bm, r.bn, r.ns, F32, r.opt, pair>,
                 std::conditional_t<r.sched == S_GEN, GenericCfg<DT, FUSED, F32>, GemmCfg<DT, r.bm, r.bn, r.wm, 4, r.ns, FUSED, F32, r.opt>>>>;
};
template <class Cfg, int SCHED> struct TileKernel { static auto get() { return delta_gemm_kernel<Cfg>; } };
#ifdef BD_AB_VARIANTS
template <class Cfg> struct TileKernel<Cfg, S_PP> { static auto get() { return delta_gemm_pp_kernel<Cfg>; } };
#endif
template <class Cfg> struct TileKernel<Cfg, S_PF> { static auto get() { return delta_gemm_pf_kernel<Cfg>; } };
template <class Cfg> struct TileKernel<Cfg, S_FX> { static auto get() { return delta_gemm_fx_kernel<Cfg>; } };
template <class Cfg> struct TileKernel<Cfg, S_W4> { static auto get() { return delta_gemm_w4_kernel<Cfg>; } };
template <class Cfg> struct TileKernel<Cfg, S_GEN> { static auto get() { return delta_gemm_generic_kernel<Cfg::DT, Cfg::FUSED, Cfg::OUT_F32>; } };

// Lifts a row to its Cfg type and calls f(Tag<Cfg>, row index).  A launch the row does not have answers BD_E_BAD_SHAPE and instantiates nothing,
// so exactly the table's kernels are compiled.  The launch record is read from the fp16 Cfg: block and LDS size do not depend on the dtype.
template <class T> struct Tag { using type = T; };
using TileRowSeq = std::make_integer_sequence<int, N_TILE_ROWS>;
template <int DT, bool FUSED, bool F32, class F, int... Is>
int lift_row(int row, F&& f, std::integer_sequence<int, Is...>) {
    int rc = BD_E_BAD_SHAPE;
    auto one = [&](auto i) {
        constexpr int I = decltype(i)::value;
        if constexpr (row_launches(TILE_ROWS[I], FUSED, F32)) {
            using Cfg = typename RowCfg<I, DT, FUSED, F32>::type;
            using Cfg16 = typename RowCfg<I, DT_F16, FUSED, F32>::type;
            static_assert(Cfg::NT == Cfg16::NT && Cfg::LDS_BYTES == Cfg16::LDS_BYTES, "the plan records block and LDS bytes from the fp16 Cfg");
            rc = f(Tag<Cfg>{}, i);
        }
    };
    // (from the last row down: the compiler instantiates the bodies of `one` in the reverse of the order they are named here, and the order
    //  of instantiation -- the table's -- is the order of the kernels in the code object)
    (void)((row == N_TILE_ROWS - 1 - Is && (one(std::integral_constant<int, N_TILE_ROWS - 1 - Is>{}), true)) || ...);
    return rc;
}

// share of the CU-rounds a tile count keeps busy (1.0 = every round full)
inline double round_fill(long long tiles, long long cus) { return (double)tiles / (double)(((tiles + cus - 1) / cus) * cus); }

// 256x256 vs 256x128 ping-pong tile: rounds of CU-wide tile waves x measured relative cost of one tile
// (256x128 does half the work of a 256x256 tile at ~0.85x its MFMA rate; DESIGN.md "tile choice").
inline int choose_big_tile(const Problem& q, long long cus) {
    const long long tm = (q.M + 255) / 256;
    const long long t0 = tm * ((q.N + 255) / 256) * q.B, t5 = tm * ((q.N + 127) / 128) * q.B;
    const double c0 = (double)((t0 + cus - 1) / cus) * 1.0, c5 = (double)((t5 + cus - 1) / cus) * (0.5 / 0.85);
    return c5 < c0 ? 5 : 0;
}

// one-pass fused kernel: 256x128 tile vs 128x128 tile.  Rounds of CU-wide tile waves x measured relative tile cost: a 128x128 tile
// takes ~0.70 of a 256x128 tile's k loop (profiles/r01_small_m.txt), so it wins exactly when it does not add rounds (M <~ 1024 at
// N = 4096; M <= 256 at N = 11008).
// (round 5: the 128x128 tile on the four-wave schedule, variant 20, takes ~0.64 of a four-wave 256x128 tile's k loop -- tools/ab_w4_128.py:
//  M = 512 gate|up 3 rounds in 145.9 us vs 2 rounds in 149.9; M = 768 q|k|v 133.5 vs 138.7 -- and is 5..17 % faster than the 8-wave 128x128
//  tile on every shape measured: profiles/r05_mt_prefill_tiles.txt)
inline int choose_fused_tile(const Problem& q, double rel128, long long cus) {
    const long long tn = (q.N + 127) / 128;
    const long long t8 = (q.M + 255) / 256 * tn * q.B, t9 = (q.M + 127) / 128 * tn * q.B;
    const double c8 = (double)((t8 + cus - 1) / cus), c9 = (double)((t9 + cus - 1) / cus) * rel128;
    return c9 < c8 ? 9 : 8;
}

// Tail split of a multi-round fused launch (one mask, 16-bit output).  The persistent 256x128 kernel needs ceil(tiles / CUs) rounds; when
// the last round is mostly empty (Llama-2-7B gate|up at 2048 rows: 1376 tiles = 5.4 rounds -> 6), the tile columns of the FULL rounds go
// to it and the remaining columns to 128x128 tiles (twice as many, ~0.70 of a round each), launched behind it on the same stream: 5 + 0.53
// instead of 6 rounds.  The tail is four-wave since round 5 (variant 20's kernel: 5..17 % faster than the 8-wave 128x128 tile on every shape
// measured); same 128-wide tile columns.  Returns the number of 128-wide tile columns for the main launch, or -1 = no split.
inline int fused_tail_split_cols(const Problem& q, long long cus) {
    if (q.B != 1) return -1;
    const long long tm = (q.M + 255) / 256, tn = (q.N + 127) / 128, T = tm * tn;
    if (T <= cus || T % cus == 0) return -1;
    const long long full = T / cus;                       // full rounds
    const long long n_main = full * cus / tm;             // whole tile columns inside them
    const long long rem = tn - n_main;
    if (n_main <= 0 || rem <= 0) return -1;
    const double now = (double)((T + cus - 1) / cus);
    const long long t_rem = ((q.M + 127) / 128) * rem;
    const double split = (double)((n_main * tm + cus - 1) / cus) + (double)((t_rem + cus - 1) / cus) * 0.70;
    return split < now - 0.2 ? (int)n_main : -1;
}

// Split-k for the one-pass fused kernel at mid-size M (16 < M <= 512: decode batches, speculative decoding, short prefills), where
// even 128x128 tiles leave most CUs idle and the launch is bound by how fast FEW CUs can stream W.  KS slices of k per tile (each
// block writes an fp32 partial [M][N] slab to the workspace) + one reduce launch.  Returns KS (1 = do not split).
constexpr int64_t SPLITK_WS_CAP = 64ll << 20;
inline int splitk_factor(int B, int M, int N, int K, long long cus) {
    if (M <= 16 || M > 512 || K % 64 || N % 8) return 1;
    const long long tiles = (long long)((M + 127) / 128) * ((N + 127) / 128) * B;
    if (tiles * 2 > cus) return 1;                       // already at least half a round of tiles
    long long ks = cus / tiles;
    if (ks > 8) ks = 8;
    const long long by_k = (K / 64) / 8;                 // at least 8 k-tiles (512 k) per slice
    if (ks > by_k) ks = by_k;
    while (ks > 1 && (int64_t)B * ks * M * N * 4 > SPLITK_WS_CAP) --ks;
    return ks < 2 ? 1 : (int)ks;
}

// ---- pair tiles (bd_gemm_fx.h / bd_gemm_w4.h, PAIR): two batch entries of <= 64 rows share one 128 x 128 tile (and its W stream); optional split-k
inline bool pair_ok(const Problem& q) {
    return q.W && q.B >= 2 && q.M >= 1 && q.M <= 64 && fast_ok(q) && q.sAb >= 0 && q.sAb < (1ll << 30) && q.sPb >= 0 && q.sPb < (1ll << 29);
}
static const int g_pair_ks_env = env_int("BD_PAIR_SPLITK", 0);       // A/B: force the k-slice count of the split pair tiles (0 = the rule)
inline int pair_splitk_dims(int B, int N, int K, long long cus) {    // k slices so that pairs x column tiles x slices ~ fills the CUs (>= 512 k per slice)
    const long long tiles = (long long)((B + 1) / 2) * ((N + 127) / 128);
    if (K % 64 || N % 8 || tiles * 2 > cus) return 1;
    if (g_pair_ks_env > 1) { int f = g_pair_ks_env; while (f > 1 && (K / f < 512 || (K / 64) % f)) --f; return f; }
    long long ks = cus / tiles;
    if (ks > 8) ks = 8;
    while (ks > 1 && K / ks < 512) --ks;
    return (int)ks;
}

// One launch of a tile plan; bd_last_gemm_plan reports it field by field.
struct TileLaunch {
    bool on = false;                   // issued at all
    int row = -1, f32 = 0;             // the kernel: TILE_ROWS index, and whether THIS launch writes fp32 (the output itself or split-k slabs)
    int bm = 0, bn = 0, sched = 0;     // (reduce launch: sched 1 = it carries the post-norm)
    int tiles_m = 0, tiles_n = 0, tile_n0 = 0, group_m = 0, ksplit = 0, nbatch = 0, nent = 0;      // GemmParams
    unsigned grid_x = 0, grid_y = 0;   // (generic kernel: z = nbatch)
    int block = 0, lds = 0;            // threads per block, dynamic LDS bytes
};
// What tile_plan decides about one call.
struct TilePlan {
    int rc = BD_OK;                    // != BD_OK: the call is refused
    int variant = -1;                  // bd_last_gemm_variant (>= 200: a decode family; nothing below is filled)
    int ks = 1, tail_col = -1;         // k slices (1 = unsplit); first 128-wide tile column of variant 14's tail launch (-1 = none)
    int64_t ws_bytes = 0;              // workspace the plan needs
    int post_norm = 0;                 // the reduce launch carries Problem::pn_w (otherwise the entry point launches the norm after the Linear)
    bool chunked = false;              // bd_set_launch_chunking applies to the main launch (not part of the record)
    TileLaunch main, tail, reduce;
};
static thread_local TilePlan t_tile_plan;           // of this thread's last call that reached dispatch()
static thread_local int g_gemm_dry_run = 0;         // bd_set_gemm_dry_run: plan and record, never touch the device

inline int64_t slab_bytes(const Problem& q, int ks) { return GEMV_TICKET_BYTES + (int64_t)q.B * ks * q.M * q.N * 4; }

// the launch of row `ri` over tile columns [col0, col1) of the problem (col1 < 0: to the last one)
inline TileLaunch plan_launch(const Problem& q, int ri, bool fused, bool f32, int ks, int col0, int col1, long long cus) {
    const TileRow& r = TILE_ROWS[ri];
    TileLaunch l;
    l.on = true; l.row = ri; l.f32 = f32; l.bm = r.bm; l.bn = r.bn; l.sched = r.sched;
    l.tiles_m = (q.M + r.bm - 1) / r.bm;
    l.tile_n0 = col0; l.tiles_n = (col1 < 0 ? (q.N + r.bn - 1) / r.bn : col1) - col0;
    l.ksplit = ks;
    const int entries = r.is(T_PAIR) ? (q.B + 1) / 2 : q.B;          // a pair tile's two halves are two batch entries (tiles_m = 1)
    l.nent = q.B; l.nbatch = r.sched == S_W4 ? entries * ks : q.B;
    // Tile walk order (profiles/r01_tile_order.txt): delta-only = n fastest (the XCD's run shares X row panels; the mask is tiny).
    // Fused = groups of 4 tile rows: each XCD's run covers a ~4 x 8 block of tiles, which minimises X + W bytes per XCD
    // (+3..5 % on the MLP shapes over n-fastest, equal to m-fastest on the single-round ones).
    l.group_m = fused ? (l.tiles_m < 4 ? l.tiles_m : 4) : 1;
    if (g_forced_group_m > 0) l.group_m = g_forced_group_m < l.tiles_m ? g_forced_group_m : l.tiles_m;
    const long long total = (long long)l.tiles_m * l.tiles_n * l.nbatch;
    if (r.sched == S_W4) { l.grid_x = (unsigned)(total < cus ? total : cus); l.grid_y = 1; }
    else if (r.sched == S_GEN) { l.grid_x = (unsigned)l.tiles_n; l.grid_y = (unsigned)l.tiles_m; }
    else { l.grid_x = (unsigned)(l.tiles_m * l.tiles_n); l.grid_y = (unsigned)(entries * ks); }
    const auto geometry = [&](auto tag, auto) { using Cfg = typename decltype(tag)::type; l.block = Cfg::NT; l.lds = Cfg::LDS_BYTES; return BD_OK; };
    if (fused) f32 ? lift_row<DT_F16, true, true>(ri, geometry, TileRowSeq{}) : lift_row<DT_F16, true, false>(ri, geometry, TileRowSeq{});
    else f32 ? lift_row<DT_F16, false, true>(ri, geometry, TileRowSeq{}) : lift_row<DT_F16, false, false>(ri, geometry, TileRowSeq{});
    return l;
}

// fills `pl` (a fresh TilePlan)
void tile_plan(const Problem& q, bool fused, bool out_f32, long long cus, TilePlan& pl) {
    const auto refuse = [&](int rc) { pl.rc = rc; };
    int v = g_forced_variant;
    const bool forced = v >= 0;
    if (v > 200 && v <= 264) v = 200;        // 200 + KS: decode path with a forced k-split (test hook)
    if (v > 300 && v <= 364) v = 300;        // 300 (+ KS): force the VALU sign-flip decode kernel
    if (v > 400 && v <= 464) v = 400;        // 400 (+ KS): force the MFMA + LUT decode kernel
    if (v > 500 && v <= 564) v = 500;        // 500 (+ KS): force the no-split-k 16-column decode kernel
    if (v > 600 && v <= 664) v = 600;        // 600 (+ columns per block / 4): force the streaming decode kernel
    if (v > 800 && v <= 804) v = 800;        // 800 (+ masks per block): force the one-mask-per-row delta kernel (bd_gemv_rows.h)
    if (v == 700) {                           // 700: the loader / consumer decode kernel (packed sign layout, fused Linear only); the
        if (q.mask_tiled != 2 || !q.W) return refuse(BD_E_BAD_SHAPE);     // stream path picks it up (launch_gemv_stream_chunk, ring_wanted)
        v = 600;
    }
    // prefill-size SwiGLU launch (bd_binary_linear_swiglu): the four-wave kernel's 256 x 128 tile, or its pair tile for several entries of <= 64
    // rows (round 6) -- the rows with epi = 1
    const bool swiglu = q.epilogue == 1 && q.M > GEMV_MAX_M;
    const auto slices = [&](bool pair) { return pair ? pair_splitk_dims(q.B, q.N, q.K, cus) : splitk_factor(q.B, q.M, q.N, q.K, cus); };
    const auto ws_holds = [&](int ks) { return q.ws && q.ws_bytes >= slab_bytes(q, ks); };
    const bool slab_rows = q.N % 8 == 0 && q.sCm % 4 == 0 && q.sCb % 4 == 0;          // the reduce launch reads and writes whole 16-byte chunks
    int ks = 1;
    const auto split10 = [&](int& n) { n = slices(false); return n > 1 && ws_holds(n); };      // the unpaired split: its slice count, and whether it is taken
    if (forced) {
        if (swiglu && v >= 200) return refuse(BD_E_BAD_SHAPE);
        if ((v == 200 || v == 300 || v == 400 || v == 500 || v == 600) && !gemv_ok(q)) return refuse(BD_E_BAD_SHAPE);
    } else if (swiglu) v = (fused && q.M <= 64 && q.B >= 2 && pair_ok(q)) ? 21 : 15;
    else if (gemv_ok(q)) v = 200;
    else if (!fast_ok(q)) v = 100;
    else if (fused && q.M > 16 && q.M <= 64 && q.B >= 2 && pair_ok(q)) {
        // several batch entries of <= 64 rows (multi-tenant prefill of short prompts, demo_backend.py:297-299): two entries per 128-row
        // tile share one W stream; narrow outputs add split-k (tools/bench_mt_prefill.py, 6 tenants x 64 rows, Mistral-7B shapes:
        // q|k|v 59 -> 50 us, o 39 -> 33, gate|up 201 -> 177, down 130 -> 91; profiles/r04_mt_prefill_tiles.txt)
        // Round 5: the same tiles on the FOUR-WAVE schedule (bd_gemm_w4.h PAIR; variants 18 / 19) -- q|k|v 51.6 -> 51.4 us, o 35.3 -> 32.2,
        // gate|up 192 -> 162 (1.12 PF useful), down 94.6 -> 83.4: -12 % per layer (profiles/r05_mt_prefill_tiles.txt).  Its split-k
        // slices are whole runs of k-tiles: when the slice count does not divide K / 64 the 8-wave kernel keeps the launch.
        // (A workspace that is missing or too small silently keeps the unsplit launch.)
        ks = slices(true);
        const bool split = ks > 1 && slab_rows && ws_holds(ks);
        if (!split) v = 18;
        else v = (q.K / 64) % ks == 0 ? 19 : 17;
    }
    else if (fused && q.M > 16 && !q.accumulate && slab_rows && split10(ks)) v = 10;
    else if (fused && q.M > 16 && q.M <= 64)                  // (not split: there are enough 64-row tiles)
        // 64x256 tiles (twice the MFMAs per X fragment read) once they fill at least half the CUs, else 64x128 for the parallelism:
        // 6 tenants x 64 rows: q+k+v 56 vs 76 us, gate+up 207 vs 253 us, but o 54 vs 38 us (tools/bench_mt_prefill.py)
        v = ((long long)((q.N + 255) / 256) * q.B * 2 >= cus) ? 12 : 11;
    else if (fused && q.M > 16) {
        // one-pass kernel (profiles/r01_fx_vs_two_loop.txt, r01_small_m.txt, r01_mid_m.txt: also for 16 < M <= 64, rows padded to the 128-row
        // tile); 16-bit outputs: the same tiles on the four-wave persistent schedule: 256x128 +4..7 % on every shape measured
        // (profiles/r03_w4_*.txt), 128x128 +5..17 % (round 5)
        v = choose_fused_tile(q, out_f32 ? 0.70 : 0.64, cus);
        if (!out_f32) v = v == 8 ? 14 : 20;
    } else if (q.M > 128) {
        v = choose_big_tile(q, cus);
        // four-wave persistent 256x256 kernel once its tiles keep >= 80 % of the CU-rounds busy (it has no 256x128 form)
        if (round_fill((long long)((q.M + 255) / 256) * ((q.N + 255) / 256) * q.B, cus) >= 0.8) v = 13;
    }
    else v = q.M > 64 ? 1 : q.M > 32 ? 2 : 3;
    if (v >= 200) { pl.variant = v; return; }              // a decode family: dispatch_decode
    // what the variant takes (a forced variant whose preconditions fail is refused, never replaced)
    const int ri = tile_row(v, fused);
    if (ri < 0) return refuse(BD_E_BAD_SHAPE);
    const TileRow& r = TILE_ROWS[ri];
    const bool split = r.is(T_SPLIT), pair = r.is(T_PAIR);
    if ((r.sched != S_GEN && !fast_ok(q)) || (out_f32 && !r.is(T_F32)) || r.is(T_SWIGLU) != swiglu || (fused && q.accumulate && !r.is(T_RESIDUAL)) ||
        (split && !slab_rows))
        return refuse(BD_E_BAD_SHAPE);
    pl.variant = v;                       // (as before the plan: the refusals below leave the variant they refused in bd_last_gemm_variant)
    if (pair && !pair_ok(q)) return refuse(BD_E_BAD_SHAPE);
    if (split) {
        if (forced) {                     // k slices from the rule, at least 2; 19: whole, equal runs of k-tiles; every slice holds a 64-k tile
            ks = slices(pair);
            if (ks < 2) ks = (v == 19 || q.K / 64 >= 2) ? 2 : 1;
            while (v == 19 && ks > 1 && (q.K / 64) % ks) --ks;
            if (ks < 2 || ks > q.K / 64) return refuse(BD_E_BAD_SHAPE);
        }
        pl.ks = ks; pl.ws_bytes = slab_bytes(q, ks);
        if (!ws_holds(ks)) return refuse(BD_E_WORKSPACE);
    }
    if (v == 14 && !forced && g_tail_split && !out_f32) pl.tail_col = fused_tail_split_cols(q, cus);
    pl.main = plan_launch(q, v == 10 && q.M > 64 ? ri + 1 : ri, fused, split || out_f32, pl.ks, 0, pl.tail_col, cus);      // (10's second row)
    if (pl.tail_col >= 0) pl.tail = plan_launch(q, tile_row(20, true), true, false, 1, pl.tail_col, -1, cus);
    pl.chunked = g_launch_chunking && (r.sched == S_PF || r.sched == S_FX) && !pair && !split;
    if (split) {
        // partial slabs [B][KS][M][N] -> C.  A pending post-norm (Problem::pn_w) rides on the reduce launch when the rows are whole 16-byte
        // chunks of at most 8192 columns: one launch instead of reduce + RMSNorm.
        TileLaunch& d = pl.reduce;
        pl.post_norm = q.pn_w && !out_f32 && q.N % 8 == 0 && q.N <= 8192 && aligned16(q.C) && q.sCm % 8 == 0 && q.sCb % 8 == 0;
        d.on = true; d.sched = pl.post_norm; d.ksplit = ks; d.nbatch = d.nent = q.B; d.block = 256;
        d.grid_x = pl.post_norm ? (unsigned)(q.B * q.M) : (unsigned)(((long long)q.M * q.N / 4 + 255) / 256);
        d.grid_y = pl.post_norm ? 1u : (unsigned)q.B;
    }
}

// The one launch body of the tile kernels.
template <class Cfg, int SCHED>
int launch_cfg(const GemmParams& p, const TileLaunch& l, bool chunked, hipStream_t st) {
    auto kern = TileKernel<Cfg, SCHED>::get();
    if constexpr (Cfg::LDS_BYTES > 0) {
        static std::atomic<uint64_t> lds_done{0};
        if (!ensure_dyn_lds((const void*)kern, Cfg::LDS_BYTES, lds_done)) return BD_E_LAUNCH;
    }
    // Experiment kept behind bd_set_launch_chunking(1): issue a multi-round problem as several launches of at most one tile per CU
    // (an mc x nc block of tiles each, via GemmParams::tile_m0 / tile_n0).  Hypothesis: rounds inside one launch drift apart and that
    // is why 8192x4096x4096 runs 10 % below back-to-back 2048-row launches.  Measured (profiles/r01_launch_chunking.txt): no gain
    // (-0..3 %, -15 % with 6 tenants) -- the back-to-back figure was warm-cache re-reads of the same operands, not synchronisation.
    const long long cus = chunked ? num_cus() : 0, B = l.grid_y;
    if (chunked && (long long)p.tiles_m * p.tiles_n * B > cus && B <= cus) {
        const long long per = cus / B;                                     // tiles per launch and batch entry
        // orientation A: all tile rows x as many tile columns as fit; B: all tile columns x as many rows as fit
        long long mcA = p.tiles_m < per ? p.tiles_m : per, ncA = per / mcA; if (ncA > p.tiles_n) ncA = p.tiles_n;
        long long ncB = p.tiles_n < per ? p.tiles_n : per, mcB = per / ncB; if (mcB > p.tiles_m) mcB = p.tiles_m;
        const long long nA = ((p.tiles_m + mcA - 1) / mcA) * ((p.tiles_n + ncA - 1) / ncA);
        const long long nB = ((p.tiles_m + mcB - 1) / mcB) * ((p.tiles_n + ncB - 1) / ncB);
        const int mc = (int)(nA <= nB ? mcA : mcB), nc = (int)(nA <= nB ? ncA : ncB);
        for (int m0 = 0; m0 < p.tiles_m; m0 += mc)
            for (int n0 = 0; n0 < p.tiles_n; n0 += nc) {
                GemmParams c = p;
                c.tile_m0 = m0; c.tile_n0 = n0;
                c.tiles_m = p.tiles_m - m0 < mc ? p.tiles_m - m0 : mc;
                c.tiles_n = p.tiles_n - n0 < nc ? p.tiles_n - n0 : nc;
                if (c.group_m > c.tiles_m) c.group_m = c.tiles_m;
                hipLaunchKernelGGL(kern, dim3((unsigned)(c.tiles_m * c.tiles_n), l.grid_y), dim3(l.block), l.lds, st, c);
            }
        return BD_OK;
    }
    hipLaunchKernelGGL(kern, dim3(l.grid_x, l.grid_y, SCHED == S_GEN ? (unsigned)l.nbatch : 1u), dim3(l.block), l.lds, st, p);
    return BD_OK;
}

// the reduce launch of a split plan: partial slabs [B][KS][M][N] -> C, with the post-norm where the plan says so
template <int DT>
void launch_splitk_reduce(const Problem& q, const TilePlan& pl, const float* part) {
    const TileLaunch& d = pl.reduce;
    if (pl.post_norm)
        hipLaunchKernelGGL((splitk_reduce_norm_kernel<DT>), dim3(d.grid_x), dim3(d.block), 0, q.st, part, (unsigned short*)q.C,
                           (const unsigned short*)q.pn_w, (unsigned short*)q.pn_h, pl.ks, q.M, q.N, (long long)q.sCb, (long long)q.sCm,
                           (long long)q.sHb, (long long)q.sHm, (long long)q.s_pnw, q.accumulate, q.pn_eps);
    else
        hipLaunchKernelGGL((splitk_reduce_kernel<DT>), dim3(d.grid_x, d.grid_y), dim3(d.block), 0, q.st, part, q.C, q.B, pl.ks, q.M, q.N,
                           (long long)q.sCb, (int)q.sCm, q.out_dtype == BD_F32 ? 1 : 0, q.accumulate);
}

// Issues a plan whose tile launches are (FUSED, F32) ones: main and tail through launch_cfg, and behind a split row's launch its reduce launch.
template <int DT, bool FUSED, bool F32>
int launch_tile_plan(const Problem& q, const TilePlan& pl) {
    for (const TileLaunch* l : {&pl.main, &pl.tail}) {
        if (!l->on) continue;
        GemmParams p;
        p.A = (const char*)q.A; p.P = q.P; p.C = (char*)q.C; p.W = (const char*)q.W; p.alpha = q.alpha;
        p.M = q.M; p.N = q.N; p.K = q.K;
        p.tiles_m = l->tiles_m; p.tiles_n = l->tiles_n; p.tile_m0 = 0; p.tile_n0 = l->tile_n0; p.ksplit = l->ksplit;
        p.sAb = q.sAb; p.sPb = q.sPb; p.sCb = q.sCb;
        p.sAm = (int)q.sAm; p.sCm = (int)q.sCm; p.ldw = (int)q.ldw;
        p.sAlb = (int)q.sAlb; p.gsz = q.N / q.G;
        p.round_mode = q.round_mode; p.accumulate = q.accumulate;
        p.nbatch = l->nbatch; p.nent = l->nent; p.group_m = l->group_m;
        const int rc = lift_row<DT, FUSED, F32>(l->row, [&](auto tag, auto i) {
            using Cfg = typename decltype(tag)::type;
            constexpr TileRow r = TILE_ROWS[decltype(i)::value];
            if constexpr (r.is(T_SPLIT)) {
                // fp32 partial slabs [entry * KS + slice][M][N] in the workspace; the residual is added by the reduce launch
                float* part = (float*)((char*)q.ws + GEMV_TICKET_BYTES);
                p.C = (char*)part; p.sCm = q.N; p.sCb = (long long)q.M * q.N; p.accumulate = 0;
                const int rc = launch_cfg<Cfg, r.sched>(p, *l, false, q.st);
                if (rc == BD_OK) launch_splitk_reduce<DT>(q, pl, part);
                return rc;
            } else return launch_cfg<Cfg, r.sched>(p, *l, pl.chunked, q.st);
        }, TileRowSeq{});
        if (rc != BD_OK) return rc;
    }
    return launch_status();
}

// the decode families (forced, or the automatic 200)
template <int DT, bool FUSED>
int dispatch_decode(const Problem& q, int v) {
    switch (v) {
        // decode: the VALU sign-flip kernel is as fast or faster on the fused Linear shapes (profiles/r01_decode_kernels.txt);
        // the MFMA + LUT kernel wins when the delta dominates (delta-only with >= 8 masks) and on narrow outputs (k/v projections)
        // ... and whenever a mask is shared by >= 2 rows (M > 1 or a broadcast mask): it expands each word once for all rows
        case 200: {
            // one mask per row, delta only, reference layout (binary_bmm at M = 1): 64-column super-tiles, the whole batch in one launch
            if constexpr (!FUSED) { if (g_forced_variant < 0 && rows_auto(q)) return launch_rows<DT>(q); }
            const int cb = GEMV_MAX_R / q.M, bc = q.B < cb ? q.B : cb, nmask = q.sPb == 0 ? 1 : bc;
            // streaming kernel: one launch, one block per CU, everything in flight from the first cycle (profiles/r02_decode_*.txt)
            if (stream_ok(q, bc * q.M, nmask)) { t_last_variant = 600; return launch_gemv<DT>(q, false, false, true); }
            // no-split-k kernel (one launch) when the chunk's activations fit in LDS and there are enough 16-column blocks to fill
            // the chip but not several rounds of them: 4096 < ... <= 8192 columns (+3..10 % over the two-launch kernels there)
            // (all of its N/16 blocks must be resident at once: a second round of 8-wave blocks pays the start-up latency again --
            // 8192x8192, 4 tenants: 50.8 vs 37.5 us)
            // up to 8 rows, fused: the wave-specialised VALU kernel is the fastest on every Llama / Mistral shape
            // (profiles/r01_decode_kernels.txt: 4096^2 T=6 14.4 us vs 15.8 one-launch kernel vs 16.7 single-role)
            if (q.W && bc * q.M <= 8 && bc * q.M < 2 * nmask && g_gemv_wave_spec) return launch_gemv<DT>(q, true);
            int ks16, ksl16;
            col16_split(bc * q.M, q.K, 0, ks16, ksl16);
            const long long lds16 = 4096 + (long long)bc * q.M * (ksl16 * 2 + 16) + 16 * 1024 + 512;
            const long long per_cu = lds16 > 0 ? (160 * 1024) / lds16 : 0;
            if (ks16 == 1 && q.N > 2048 && (q.N + 15) / 16 <= (long long)num_cus() * (per_cu < 2 ? per_cu : 2))
                return launch_gemv<DT>(q, false, true);
            return launch_gemv<DT>(q, !((!q.W && nmask >= 8) || q.N <= 2048 || bc * q.M >= 2 * nmask));
        }
        case 300: return launch_gemv<DT>(q, true);
        case 400: return launch_gemv<DT>(q, false);
        case 500: return launch_gemv<DT>(q, false, true);
        case 600: {
            const int cb = GEMV_MAX_R / q.M, bc = q.B < cb ? q.B : cb, nmask = q.sPb == 0 ? 1 : bc;
            if (!stream_ok(q, bc * q.M, nmask)) return BD_E_BAD_SHAPE;
            return launch_gemv<DT>(q, false, false, true);
        }
        case 800:    // delta_rows_kernel (801 / 802 / 804: masks per block forced)
            if constexpr (!FUSED) return launch_rows<DT>(q);
            else return BD_E_BAD_SHAPE;
        default: return BD_E_BAD_SHAPE;
    }
}

// Issues a plan.  The order in which this function names its callees is the order in which the compiler is asked for their kernels, and so the
// kernels' order in the code object: per dtype the fused fp32 tile launches, the fused decode families, the fused 16-bit tile launches, the
// delta-only fp32 ones, the delta-only decode families, the delta-only 16-bit ones -- where they lay before the dispatch was split into a plan
// and a launcher.  Byte-identical kernels at other addresses measured +0.2 % on the prefill step (profiles/prefill_dispatch_refactor.txt).
template <int DT>
int launch_plan(const Problem& q, const TilePlan& pl, bool fused) {
    const bool tile = pl.variant < 200, f32 = pl.main.f32 != 0;      // (a tail launch writes what the main launch writes)
    if (tile && fused && f32) return launch_tile_plan<DT, true, true>(q, pl);
    if (fused && !tile) return dispatch_decode<DT, true>(q, pl.variant);
    if (fused) return launch_tile_plan<DT, true, false>(q, pl);
    if (tile && f32) return launch_tile_plan<DT, false, true>(q, pl);
    if (!tile) return dispatch_decode<DT, false>(q, pl.variant);
    return launch_tile_plan<DT, false, false>(q, pl);
}

int dispatch(const Problem& q) {
    TilePlan& pl = t_tile_plan;
    pl = TilePlan{};
    if (q.B < 0 || q.M < 0 || q.N < 0 || q.K < 0) return BD_E_BAD_SHAPE;
    if (q.K % 32) return BD_E_K_NOT_MULTIPLE;
    if (q.dtype != BD_F16 && q.dtype != BD_BF16) return BD_E_BAD_DTYPE;
    if (q.out_dtype != q.dtype && q.out_dtype != BD_F32) return BD_E_BAD_DTYPE;
    if (q.G < 1 || (q.N > 0 && q.N % q.G)) return BD_E_BAD_GROUPS;
    if (q.B == 0 || q.M == 0 || q.N == 0) return BD_OK;
    if (q.B > 65535) return BD_E_BAD_SHAPE;
    if (!q.A || !q.P || !q.C) return BD_E_NULL;
    if ((q.W || q.accumulate) && !q.alpha) return BD_E_NULL;
    if (q.K == 0) return BD_E_BAD_SHAPE;
    const bool fused = q.W != nullptr;
    tile_plan(q, fused, q.out_dtype == BD_F32, num_cus(), pl);
    if (pl.variant >= 0) t_last_variant = pl.variant;
    if (pl.rc != BD_OK || g_gemm_dry_run) return pl.rc;
    return q.dtype == BD_BF16 ? launch_plan<DT_BF16>(q, pl, fused) : launch_plan<DT_F16>(q, pl, fused);
}

}  // namespace

extern "C" int bd_set_gemm_dry_run(int on) { g_gemm_dry_run = on ? 1 : 0; return BD_OK; }
extern "C" int bd_last_gemm_plan(int32_t* out, int n) {
    const TilePlan& pl = t_tile_plan;
    int32_t rec[BD_GEMM_PLAN_INTS] = {pl.rc, pl.variant, pl.ks, pl.tail_col, (int32_t)(pl.ws_bytes & 0xffffffffll), (int32_t)(pl.ws_bytes >> 32), pl.post_norm};
    int at = 7;
    for (const TileLaunch* l : {&pl.main, &pl.tail, &pl.reduce})
        for (int v : {l->on ? l->bm : -1, l->bn, l->sched, l->tiles_m, l->tiles_n, l->tile_n0, l->group_m, l->ksplit, l->nbatch, l->nent, (int)l->grid_x,
                      (int)l->grid_y, l->block, l->lds})
            rec[at++] = v;
    for (int i = 0; out && i < n && i < BD_GEMM_PLAN_INTS; ++i) out[i] = rec[i];
    return BD_GEMM_PLAN_INTS;
}
extern "C" int bd_last_decode_form(void) { return t_last_plan.form; }
extern "C" int bd_set_decode_dry_run(int on) { g_decode_dry_run = on ? 1 : 0; return BD_OK; }
extern "C" int bd_last_decode_plan(int32_t* out, int n) {
    const StreamPlan& pl = t_last_plan;
    const StreamForm& f = pl.f;
    const int32_t rec[BD_DECODE_PLAN_INTS] = {pl.rc, f.DT, f.NM, f.HASW, f.NS, f.NW, f.WNAT, f.AUX, f.PK, f.XL, f.EPI, f.WT, f.FG, (int32_t)pl.grid,
                                              (int32_t)pl.grid_y, pl.block, pl.lds, pl.cpb, (int32_t)pl.xs_off, (int32_t)pl.xrow, pl.form};
    for (int i = 0; out && i < n && i < BD_DECODE_PLAN_INTS; ++i) out[i] = rec[i];
    return BD_DECODE_PLAN_INTS;
}

extern "C" int64_t bd_gemm_workspace_bytes(int B, int M, int N, int K) {
    if (B <= 0 || M <= 0 || N <= 0 || K <= 0) return 0;
    if (M > GEMV_MAX_M || (int64_t)B * M > 4 * GEMV_MAX_R) {
        // mid-size M: split-k partial slabs of the fused tile kernel -- only where the automatic rule really splits (or a test
        // forces the split-k variant); every other tile-kernel launch needs no scratch at all
        if (M > 16 && M <= 512 && K % 64 == 0 && N % 8 == 0) {
            int ks = splitk_factor(B, M, N, K, num_cus());
            if (ks < 2 && g_forced_variant == 10) ks = 2;
            if (B >= 2 && M <= 64) {                      // pair tiles (variants 16 / 17) split by their own rule
                int kp = pair_splitk_dims(B, N, K, num_cus());
                if (kp < 2 && (g_forced_variant == 17 || g_forced_variant == 19)) kp = 2;
                if (kp > ks) ks = kp;
            }
            if (ks < 2) return 0;
            const int64_t need = (int64_t)B * ks * M * N * 4;
            return need <= SPLITK_WS_CAP * 2 ? GEMV_TICKET_BYTES + need : 0;
        }
        return 0;
    }
    Problem q{};
    { const int cb = GEMV_MAX_R / M; B = B < cb ? B : cb; }     // the decode path works on chunks of <= 16 rows
    q.B = B; q.M = M; q.N = N; q.K = K;
    int KS, kslice;
    gemv_split(q, KS, kslice);
    int KSmax = K / 512 < 1 ? 1 : K / 512;               // upper bound over the auto rule and the forced-KS test hook
    if (KS > KSmax) KSmax = KS;
    return GEMV_TICKET_BYTES + (int64_t)KSmax * B * M * N * 4;
}

extern "C" int bd_delta_bmm(const void* A, const int32_t* P, void* C, int B, int M, int N, int K, int64_t sAb, int64_t sAm,
                            int64_t sPb, int64_t sCb, int64_t sCm, int dtype, int out_dtype, int round_mode,
                            const float* alpha, int64_t sAlb, int G, int accumulate, void* ws, int64_t ws_bytes,
                            void* stream) {
    Problem q{};
    q.A = A; q.P = P; q.C = C; q.W = nullptr; q.alpha = alpha;
    q.B = B; q.M = M; q.N = N; q.K = K;
    q.sAb = sAb; q.sAm = sAm; q.sPb = sPb; q.sCb = sCb; q.sCm = sCm; q.ldw = 0; q.sAlb = sAlb;
    q.G = alpha ? G : 1; q.dtype = dtype; q.out_dtype = out_dtype; q.round_mode = round_mode;
    q.accumulate = accumulate ? 1 : 0;
    q.ws = ws; q.ws_bytes = ws_bytes; q.st = (hipStream_t)stream;
    if (alpha && !accumulate) {
        // C = alpha * acc without a C_in: express as the fused epilogue of an all-zero base is not worth a kernel;
        // zero C then accumulate (two tiny ops on the output only).
        if (B > 0 && M > 0 && N > 0 && C && !g_gemm_dry_run) {
            const size_t esz = out_dtype == BD_F32 ? 4 : 2;
            if (sCm == N && (sCb == (int64_t)M * N || B == 1)) {
                if (hipMemsetAsync(C, 0, (size_t)B * M * N * esz, q.st) != hipSuccess) return BD_E_LAUNCH;
            } else {
                for (int b = 0; b < B; ++b)
                    if (hipMemset2DAsync((char*)C + (size_t)b * sCb * esz, (size_t)sCm * esz, 0, (size_t)N * esz, M, q.st) !=
                        hipSuccess)
                        return BD_E_LAUNCH;
            }
        }
        q.accumulate = 1;
    }
    return dispatch(q);
}

// int8 / 4-bit base weight (bd_binary_linear_decode_w8 / _q4: q.w_tiled 2 / 3, the kernel's WT): the streaming decode kernel and nothing else --
// a forced variant other than the streaming kernel's own test hooks is refused, like every launch no kernel implements
static int dispatch_quant(const Problem& q) {
    if (q.dtype != BD_F16 && q.dtype != BD_BF16) return BD_E_BAD_DTYPE;
    if (q.out_dtype != q.dtype && q.out_dtype != BD_F32) return BD_E_BAD_DTYPE;
    if (q.G < 1 || q.N % q.G) return BD_E_BAD_GROUPS;
    if (!q.A || !q.P || !q.C || !q.alpha) return BD_E_NULL;
    if (g_forced_variant >= 0 && !(g_forced_variant >= 600 && g_forced_variant <= 664)) return BD_E_BAD_SHAPE;
    t_last_variant = 600;
    return launch_gemv_stream_chunk(q);
}

// `q` arrives with what the entry point fuses around the Linear or says about its base weight, filled by name: norm_w / sNw / eps / epilogue,
// ssq_in / ssq_out / xw_out, pn_*, and wscale (int8: its presence is the signal) or q4p / q4_group (4-bit); everything else is set here.
static int binary_linear_impl(const void* X, const void* W, const int32_t* P, const float* alpha, void* Y, int B, int M,
                              int N, int K, int64_t sXb, int64_t sXm, int64_t ldw, int64_t sPb, int64_t sAlb, int G,
                              int64_t sYb, int64_t sYm, int dtype, int out_dtype, int accumulate, int mask_tiled, int t_pad,
                              void* ws, int64_t ws_bytes, void* stream, Problem q = {}) {
    if (B > 0 && M > 0 && N > 0 && !W) return BD_E_NULL;
    q.A = X; q.P = P; q.C = Y; q.W = W; q.alpha = alpha;
    q.B = B; q.M = M; q.N = N; q.K = K;
    q.sAb = sXb; q.sAm = sXm; q.sPb = sPb; q.sCb = sYb; q.sCm = sYm; q.ldw = ldw; q.sAlb = sAlb;
    q.G = G; q.dtype = dtype; q.out_dtype = out_dtype; q.round_mode = 0; q.accumulate = accumulate ? 1 : 0;
    q.mask_tiled = mask_tiled; q.t_pad = t_pad;
    q.w_tiled = 0;
    if (ldw == 0 && W) {      // tile-major base weight (the decode copy made by the serving side): packed sign layout only, whole blocks
        if (mask_tiled != 2 || N % 16 || K % 128 || M != 1) return BD_E_BAD_SHAPE;
        q.w_tiled = 1;
        q.ldw = K;            // (extent checks below; the kernel does not use it)
    }
    if (q.wscale) {           // int8 tile-major base weight + row scales: the tile-major envelope, nothing else (no row-major int8 form)
        if (!q.w_tiled || B < 1 || B > GEMV_MAX_R || !aligned16(q.wscale)) return BD_E_BAD_SHAPE;
        q.w_tiled = 2;
    }
    if (q.q4_group) {           // 4-bit GPTQ tile-major base weight + packed group parameters: the tile-major envelope, nothing else
        if (q.wscale || !q.w_tiled || !q.q4p || B < 1 || B > GEMV_MAX_R || !aligned16(q.q4p) || !aligned16(W)) return BD_E_BAD_SHAPE;
        if (q.q4_group < 128 || q.q4_group % 128 || K % q.q4_group || K / 128 >= 65536) return BD_E_BAD_SHAPE;
        q.w_tiled = 3;
    }
    if (q.ssq_in || q.ssq_out || q.xw_out) {
        // RMSNorm hand-off (gemv_stream_kernel, StreamParams::ssq_in / ssq_out / xw_out): packed layout, one row per tenant, <= 8 tenants
        if (mask_tiled != 2 || M != 1 || B > 8 || (q.ssq_in && q.ssq_out)) return BD_E_BAD_SHAPE;
        if (q.ssq_in && (q.norm_w || !aligned16(q.ssq_in) || K % 16 || K > 16 * 256 * 2)) return BD_E_BAD_SHAPE;   // (X = the producer's pre-multiplied copy)
        if (q.ssq_out && (N % 16 || out_dtype == BD_F32 || q.epilogue || !aligned16(q.ssq_out))) return BD_E_BAD_SHAPE;
        if (q.xw_out && (!q.ssq_out || !q.norm_w || q.sNw < 0)) return BD_E_BAD_SHAPE;
        if (q.ssq_out && q.norm_w && !q.xw_out) return BD_E_BAD_SHAPE;
        if (q.ssq_out) {            // the producer's norm_w is the NEXT norm's weight (epilogue multiply), not a prologue on its own input
            q.nw_next = q.norm_w; q.sNwNext = q.sNw;
            q.norm_w = nullptr;
        }
    }
    if (q.norm_w || q.epilogue) {
        // fused prologue / epilogue of the packed streaming kernel: see gemv_stream_kernel (XL, EPI)
        if (mask_tiled != 2 || (q.epilogue != 0 && q.epilogue != 1)) return BD_E_BAD_SHAPE;
        if (q.norm_w) {
            if (!aligned16(q.norm_w) || q.sNw % 8 || q.sNw < 0) return BD_E_BAD_SHAPE;
            // one row per tenant (M == 1: the decode step), K = 2048 * 2^s, all rows in 16 x 16-byte chunks per thread
            // (the hand-off form needs no power of two: its copy is flat)
            if (M != 1 || K < 2048 || (!q.ssq_in && (K & (K - 1))) || (int64_t)B * K > 16 * 2048) return BD_E_BAD_SHAPE;
            if ((int64_t)STREAM_XS_OFF + (int64_t)B * M * (2 * (int64_t)K + 16) > STREAM_LDS_MAX) return BD_E_BAD_SHAPE;
            if ((int64_t)(B - 1) * q.sNw + K >= (1ll << 30)) return BD_E_BAD_SHAPE;
        }
        if (q.epilogue && (N % 16 || G != 2 || out_dtype != dtype || accumulate)) return BD_E_BAD_SHAPE;
    }
    q.ws = ws; q.ws_bytes = ws_bytes; q.st = (hipStream_t)stream;
    // tile-major masks exist for the streaming decode kernel only (serving-side repack; the reference layout works everywhere)
    if (q.mask_tiled) {
        const bool forced_other = g_forced_variant >= 0 && g_forced_variant != 200 && g_forced_variant != 700 &&
                                  !(g_forced_variant >= 600 && g_forced_variant <= 664);
        if (M < 1 || M > GEMV_MAX_M || forced_other || !gemv_ok(q)) return BD_E_BAD_SHAPE;
        const int cb = GEMV_MAX_R / M, bc = B < cb ? B : cb;
        if (!stream_ok(q, bc * M, sPb == 0 ? 1 : bc)) return BD_E_BAD_SHAPE;
        if (q.mask_tiled == 2) {      // interleaved tenants: the whole batch is one chunk, one dword slot per tenant
            const bool tp_ok = t_pad == 1 || t_pad == 2 || t_pad == 4 || t_pad == 6 || t_pad == 8 || t_pad == 12 || t_pad == 16;
            if (!tp_ok || B > t_pad || B > cb || (sPb == 0 && B > 1 && t_pad != 1)) return BD_E_BAD_SHAPE;
            q.sPb = t_pad == 1 ? 0 : 1;             // only "broadcast or not" matters to the kernel in this layout
            if (t_pad == 1 && B > 1) q.sPb = 0;
        } else if (q.mask_tiled != 1) return BD_E_BAD_SHAPE;
    }
    // Y += ... is an epilogue of the decode kernels only (a residual add costs a launch per Linear there; at prefill sizes it is
    // noise next to the GEMM and stays with the caller)
    // Y += ... (residual epilogue): the decode kernels and the one-pass fused tile kernels (M > 16 on their fast path)
    if (q.accumulate && !gemv_ok(q) && !(M > 16 && fast_ok(q))) return BD_E_BAD_SHAPE;
    if (q.w_tiled >= 2) return dispatch_quant(q);
    return dispatch(q);
}

extern "C" int bd_binary_linear(const void* X, const void* W, const int32_t* P, const float* alpha, void* Y, int B, int M,
                                int N, int K, int64_t sXb, int64_t sXm, int64_t ldw, int64_t sPb, int64_t sAlb, int G,
                                int64_t sYb, int64_t sYm, int dtype, int out_dtype, void* ws, int64_t ws_bytes,
                                void* stream) {
    return binary_linear_impl(X, W, P, alpha, Y, B, M, N, K, sXb, sXm, ldw, sPb, sAlb, G, sYb, sYm, dtype, out_dtype, 0, 0, 0, ws,
                              ws_bytes, stream);
}

extern "C" int bd_binary_linear_swiglu(const void* X, const void* W, const int32_t* P, const float* alpha, void* Y, int B, int M, int N,
                                       int K, int64_t sXb, int64_t sXm, int64_t ldw, int64_t sPb, int64_t sAlb, int64_t sYb, int64_t sYm,
                                       int dtype, void* stream) {
    if (B > 0 && M > 0 && N > 0 && !W) return BD_E_NULL;
    if (M <= GEMV_MAX_M) return BD_E_BAD_SHAPE;                    // decode shapes: bd_binary_linear_decode_fused (packed sign layout)
    if (N % 16 || K % 64 || sYm % 8 || sYb % 8 || !aligned16(Y)) return BD_E_BAD_SHAPE;
    Problem q{};
    q.A = X; q.P = P; q.C = Y; q.W = W; q.alpha = alpha;
    q.B = B; q.M = M; q.N = N; q.K = K;
    q.sAb = sXb; q.sAm = sXm; q.sPb = sPb; q.sCb = sYb; q.sCm = sYm; q.ldw = ldw; q.sAlb = sAlb;
    q.G = 2; q.dtype = dtype; q.out_dtype = dtype; q.round_mode = 0; q.accumulate = 0;
    q.epilogue = 1;
    q.st = (hipStream_t)stream;
    if (!fast_ok(q)) return BD_E_BAD_SHAPE;
    return dispatch(q);
}

extern "C" int bd_binary_linear_decode(const void* X, const void* W, const int32_t* P, int mask_layout, int t_pad, const float* alpha,
                                       void* Y, int B, int M, int N, int K, int64_t sXb, int64_t sXm, int64_t ldw, int64_t sPb,
                                       int64_t sAlb, int G, int64_t sYb, int64_t sYm, int dtype, int out_dtype, int accumulate,
                                       void* stream) {
    if (mask_layout != 1 && mask_layout != 2) return BD_E_BAD_SHAPE;
    return binary_linear_impl(X, W, P, alpha, Y, B, M, N, K, sXb, sXm, ldw, sPb, sAlb, G, sYb, sYm, dtype, out_dtype,
                              accumulate, mask_layout, t_pad, nullptr, 0, stream);
}

extern "C" int bd_binary_linear_decode_fused(const void* X, const void* W, const int32_t* P, int t_pad, const float* alpha, void* Y,
                                             int B, int M, int N, int K, int64_t sXb, int64_t sXm, int64_t ldw, int64_t sPb,
                                             int64_t sAlb, int G, int64_t sYb, int64_t sYm, int dtype, int out_dtype,
                                             int accumulate, const void* norm_w, int64_t s_norm, float eps, int epilogue,
                                             void* stream) {
    if (!norm_w && epilogue != 1) return BD_E_NULL;
    if (B < 1 || M < 1 || N < 1 || K < 1) return BD_E_BAD_SHAPE;
    Problem e{};
    e.norm_w = norm_w; e.sNw = s_norm; e.eps = eps; e.epilogue = epilogue;
    return binary_linear_impl(X, W, P, alpha, Y, B, M, N, K, sXb, sXm, ldw, sPb, sAlb, G, sYb, sYm, dtype, out_dtype, accumulate, 2,
                              t_pad, nullptr, 0, stream, e);
}

extern "C" int bd_binary_linear_decode_handoff(const void* X, const void* W, const int32_t* P, int t_pad, const float* alpha, void* Y,
                                               int B, int M, int N, int K, int64_t sXb, int64_t sXm, int64_t ldw, int64_t sPb,
                                               int64_t sAlb, int G, int64_t sYb, int64_t sYm, int dtype, int out_dtype,
                                               int accumulate, const void* norm_w, int64_t s_norm, float eps, int epilogue,
                                               const float* ssq_in, float* ssq_out, void* xw_out, void* stream) {
    if (!ssq_in && !ssq_out) return BD_E_NULL;
    if (B < 1 || M < 1 || N < 1 || K < 1) return BD_E_BAD_SHAPE;
    Problem e{};
    e.norm_w = norm_w; e.sNw = s_norm; e.eps = eps; e.epilogue = epilogue;
    e.ssq_in = ssq_in; e.ssq_out = ssq_out; e.xw_out = xw_out;
    return binary_linear_impl(X, W, P, alpha, Y, B, M, N, K, sXb, sXm, ldw, sPb, sAlb, G, sYb, sYm, dtype, out_dtype, accumulate, 2,
                              t_pad, nullptr, 0, stream, e);
}

extern "C" int bd_binary_linear_decode_w8(const void* X, const int8_t* W8, const float* wscale, const int32_t* P, int t_pad, const float* alpha,
                                          void* Y, int B, int M, int N, int K, int64_t sXb, int64_t sXm, int64_t sPb, int64_t sAlb, int G,
                                          int64_t sYb, int64_t sYm, int dtype, int out_dtype, int accumulate, const void* norm_w,
                                          int64_t s_norm, float eps, int epilogue, const float* ssq_in, float* ssq_out, void* xw_out,
                                          void* stream) {
    if (B < 1 || M != 1 || N < 1 || K < 1 || N % 16 || K % 128) return BD_E_BAD_SHAPE;      // (no row-major int8 form, no M > 1 form)
    if (!W8 || !wscale) return BD_E_NULL;
    Problem e{};
    e.norm_w = norm_w; e.sNw = s_norm; e.eps = eps; e.epilogue = epilogue;
    e.ssq_in = ssq_in; e.ssq_out = ssq_out; e.xw_out = xw_out;
    e.wscale = wscale;
    return binary_linear_impl(X, W8, P, alpha, Y, B, M, N, K, sXb, sXm, /* ldw: tile-major */ 0, sPb, sAlb, G, sYb, sYm, dtype, out_dtype,
                              accumulate, 2, t_pad, nullptr, 0, stream, e);
}

extern "C" int bd_binary_linear_decode_q4(const void* X, const int32_t* W4, const uint32_t* qparams, int group_size, const int32_t* P, int t_pad,
                                          const float* alpha, void* Y, int B, int M, int N, int K, int64_t sXb, int64_t sXm, int64_t sPb, int64_t sAlb,
                                          int G, int64_t sYb, int64_t sYm, int dtype, int out_dtype, int accumulate, const void* norm_w,
                                          int64_t s_norm, float eps, int epilogue, const float* ssq_in, float* ssq_out, void* xw_out,
                                          void* stream) {
    if (B < 1 || M != 1 || N < 1 || K < 1 || N % 16 || K % 128) return BD_E_BAD_SHAPE;      // (no row-major 4-bit form, no M > 1 form)
    if (group_size < 128 || group_size % 128 || K % group_size) return BD_E_BAD_SHAPE;      // (a 128-k stage lies inside one group)
    if (!W4 || !qparams) return BD_E_NULL;
    Problem e{};
    e.norm_w = norm_w; e.sNw = s_norm; e.eps = eps; e.epilogue = epilogue;
    e.ssq_in = ssq_in; e.ssq_out = ssq_out; e.xw_out = xw_out;
    e.q4p = qparams; e.q4_group = group_size;
    return binary_linear_impl(X, W4, P, alpha, Y, B, M, N, K, sXb, sXm, /* ldw: tile-major */ 0, sPb, sAlb, G, sYb, sYm, dtype, out_dtype,
                              accumulate, 2, t_pad, nullptr, 0, stream, e);
}

extern "C" int bd_binary_linear_residual(const void* X, const void* W, const int32_t* P, const float* alpha, void* Y, int B,
                                         int M, int N, int K, int64_t sXb, int64_t sXm, int64_t ldw, int64_t sPb,
                                         int64_t sAlb, int G, int64_t sYb, int64_t sYm, int dtype, int out_dtype, void* ws,
                                         int64_t ws_bytes, void* stream) {
    return binary_linear_impl(X, W, P, alpha, Y, B, M, N, K, sXb, sXm, ldw, sPb, sAlb, G, sYb, sYm, dtype, out_dtype, 1, 0, 0, ws,
                              ws_bytes, stream);
}

// residual Linear + the RMSNorm that follows it (prefill sizes: the o / down projections of a decoder layer and the norm in front of the next
// Linear).  The norm rides on the split-k reduce launch when the dispatcher splits (the multi-tenant request of short prompts); otherwise it is
// the ordinary per-tenant norm launch behind the Linear -- the same arithmetic either way.
extern "C" int bd_binary_linear_residual_norm(const void* X, const void* W, const int32_t* P, const float* alpha, void* Y, int B, int M, int N,
                                              int K, int64_t sXb, int64_t sXm, int64_t ldw, int64_t sPb, int64_t sAlb, int G, int64_t sYb,
                                              int64_t sYm, int dtype, const void* norm_w, int64_t s_nw, float eps, void* H, int64_t sHb,
                                              int64_t sHm, void* ws, int64_t ws_bytes, void* stream) {
    if (B < 0 || M < 0 || N < 0) return BD_E_BAD_SHAPE;
    if (dtype != BD_F16 && dtype != BD_BF16) return BD_E_BAD_DTYPE;
    if (B == 0 || M == 0 || N == 0) return BD_OK;
    if (!norm_w || !H || !Y) return BD_E_NULL;
    // the norm kernels' envelope: whole 16-byte chunks, rows of at most 8192 columns (both norm forms), dense [B, M] row grid for the fallback launch
    if (M <= GEMV_MAX_M || N % 8 || N > 8192 || sYm % 8 || sYb % 8 || sHm % 8 || sHb % 8 || s_nw % 8 || s_nw < 0 || !aligned16(Y) || !aligned16(H) ||
        !aligned16(norm_w) || sYb != (int64_t)M * sYm || sHb != (int64_t)M * sHm)
        return BD_E_BAD_SHAPE;
    Problem e{};
    e.pn_w = norm_w; e.s_pnw = s_nw; e.pn_eps = eps; e.pn_h = H; e.sHb = sHb; e.sHm = sHm;
    const int rc = binary_linear_impl(X, W, P, alpha, Y, B, M, N, K, sXb, sXm, ldw, sPb, sAlb, G, sYb, sYm, dtype, dtype, 1, 0, 0, ws, ws_bytes,
                                      stream, e);
    if (rc != BD_OK || t_tile_plan.post_norm || g_gemm_dry_run) return rc;
    return bd_srv_rmsnorm(Y, norm_w, H, B * M, N, sYm, sHm, s_nw, M, eps, dtype, stream);
}

// ------------------------------------------------------------------ per-tenant dense Linear (serving: lm_head per tenant)
extern "C" int bd_tenant_linear(const void* X, const void* W, void* Y, int T, int M, int N, int K, int64_t sXt, int64_t sXm,
                                int64_t sWt, int64_t ldw, int64_t sYt, int64_t sYm, int dtype, int out_dtype, void* stream) {
    if (T < 0 || M < 0 || N < 0 || K < 0) return BD_E_BAD_SHAPE;
    if (dtype != BD_F16 && dtype != BD_BF16) return BD_E_BAD_DTYPE;
    if (out_dtype != dtype && out_dtype != BD_F32) return BD_E_BAD_DTYPE;
    if (T == 0 || M == 0 || N == 0) return BD_OK;
    if (!X || !W || !Y) return BD_E_NULL;
    if (K % 32) return BD_E_K_NOT_MULTIPLE;
    // decode shapes only (the weight-streaming kernel): larger M is a plain batched GEMM and belongs to the BLAS library
    if (M > GEMV_MAX_M || T > 65535 || K == 0) return BD_E_BAD_SHAPE;
    if (!aligned16(X) || !aligned16(W) || sXm % 8 || sXt % 8 || ldw % 8 || sWt % 8) return BD_E_BAD_SHAPE;
    const int64_t lim = (1ll << 31) - 64;
    const int64_t xb = ((int64_t)(M - 1) * sXm + K) * 2, wb = ((int64_t)(N - 1) * ldw + K) * 2;
    if (xb >= lim || wb >= lim || sXm < 0) return BD_E_BAD_SHAPE;
    StreamParams sp{};
    GemvParams& gp = sp.g;
    gp.X = (const unsigned short*)X; gp.W = (const unsigned short*)W; gp.P = nullptr; gp.alpha = nullptr; gp.C = Y;
    gp.ws = nullptr; gp.tickets = nullptr;
    gp.B = 1; gp.M = M; gp.N = N; gp.K = K; gp.R = M;
    gp.sXb = 0; gp.sPb = 0; gp.sCb = 0;
    gp.sXm = (int)sXm; gp.sCm = (int)sYm; gp.ldw = (int)ldw; gp.sAlb = 0; gp.gsz = N;
    gp.KS = 1; gp.kslice = K; gp.round_mode = 0; gp.accumulate = 0; gp.out_f32 = (out_dtype == BD_F32);
    sp.sXt = sXt; sp.sWt = sWt; sp.sCt = sYt;
    sp.x_bytes = (uint32_t)xb; sp.w_bytes = (uint32_t)wb; sp.p_bytes = 0; sp.pts = 16; sp.prs = (uint32_t)N;
    int bpt = num_cus() / T;                       // blocks per tenant: all tenants stream concurrently, ~one block per CU in total
    if (bpt < 1) bpt = 1;
    int cpb = (N + bpt - 1) / bpt;
    cpb = (cpb + 3) & ~3;
    if (cpb < 4) cpb = 4;
    sp.cpb = cpb;
    StreamPlan pl;
    StreamForm& f = pl.f;
    f.DT = dtype == BD_BF16 ? DT_BF16 : DT_F16;
    f.PK = f.WT = f.XL = f.FG = f.NM = f.EPI = 0; f.HASW = 1; f.NW = 4;
    f.NS = stream_depth(0, 0, 0, 0);
    // A/B (round 6; bd_set_stream_tuning bits 11 / 12): natural-order weight loads (a load instruction = 16 rows x 64 contiguous bytes) with / without the
    // non-temporal policy, against the shipped word-row order.  profiles/r06_decode_step.txt has the outcome.
    f.WNAT = (g_stream_tune & (2048 | 4096)) ? 1 : 0;
    f.AUX = (g_stream_tune & 2048) ? 2 : 0;
    if (STREAM_AB && !f.WNAT) stream_plan_tuned(f);
    pl.cpb = cpb; pl.grid = (unsigned)((N + cpb - 1) / cpb); pl.grid_y = (unsigned)T;
    stream_plan_lds(pl, M);
    return launch_stream(pl, sp, (hipStream_t)stream);
}

// ------------------------------------------------------------------ serving-loop glue (decode step; callers of the path)
extern "C" int bd_srv_rmsnorm(const void* X, const void* Wt, void* Y, int rows, int H, int64_t sx, int64_t sy, int64_t sw,
                              int rows_per_tenant, float eps, int dtype, void* stream) {
    if (rows < 0 || H < 0 || rows_per_tenant < 1) return BD_E_BAD_SHAPE;
    if (dtype != BD_F16 && dtype != BD_BF16) return BD_E_BAD_DTYPE;
    if (rows == 0 || H == 0) return BD_OK;
    if (!X || !Wt || !Y) return BD_E_NULL;
    if (H % 8 || sx % 8 || sy % 8 || sw % 8 || !aligned16(X) || !aligned16(Wt) || !aligned16(Y)) return BD_E_BAD_SHAPE;
    hipStream_t st = (hipStream_t)stream;
    // many rows of 2048 / 4096 / 6144 / 8192 elements: one wave per row, the row in registers (rmsnorm_rows_kernel; bit-identical results)
    if (rows >= g_norm_rows_min && H % 2048 == 0 && H <= 8192) {
        const dim3 grid((unsigned)((rows + 3) / 4));
#define BD_NR(DT, NCH) hipLaunchKernelGGL((rmsnorm_rows_kernel<DT, NCH>), grid, dim3(256), 0, st, (const unsigned short*)X, (const unsigned short*)Wt, \
                                          (unsigned short*)Y, rows, (long long)sx, (long long)sy, (long long)sw, rows_per_tenant, eps)
        const int nch = H / 2048;
        if (dtype == BD_BF16) { if (nch == 1) BD_NR(DT_BF16, 1); else if (nch == 2) BD_NR(DT_BF16, 2); else if (nch == 3) BD_NR(DT_BF16, 3); else BD_NR(DT_BF16, 4); }
        else { if (nch == 1) BD_NR(DT_F16, 1); else if (nch == 2) BD_NR(DT_F16, 2); else if (nch == 3) BD_NR(DT_F16, 3); else BD_NR(DT_F16, 4); }
#undef BD_NR
        return launch_status();
    }
    if (dtype == BD_BF16)
        hipLaunchKernelGGL((rmsnorm_tenant_kernel<DT_BF16>), dim3(rows), dim3(256), 0, st, (const unsigned short*)X, (const unsigned short*)Wt,
                           (unsigned short*)Y, H, (long long)sx, (long long)sy, (long long)sw, rows_per_tenant, eps);
    else
        hipLaunchKernelGGL((rmsnorm_tenant_kernel<DT_F16>), dim3(rows), dim3(256), 0, st, (const unsigned short*)X, (const unsigned short*)Wt,
                           (unsigned short*)Y, H, (long long)sx, (long long)sy, (long long)sw, rows_per_tenant, eps);
    return launch_status();
}

extern "C" int bd_srv_add_rmsnorm(const void* resid, const float* y32, const void* Wt, void* x_out, void* h_out, int rows, int H, int64_t s_r,
                                  int64_t s_y, int64_t s_x, int64_t s_h, int64_t sw, int rows_per_tenant, float eps, int dtype, void* stream) {
    if (rows < 0 || H < 0 || rows_per_tenant < 1) return BD_E_BAD_SHAPE;
    if (dtype != BD_F16 && dtype != BD_BF16) return BD_E_BAD_DTYPE;
    if (rows == 0 || H == 0) return BD_OK;
    if (!resid || !y32 || !Wt || !x_out || !h_out) return BD_E_NULL;
    if (H % 8 || H > 8192 || s_r % 8 || s_y % 4 || s_x % 8 || s_h % 8 || sw % 8 || !aligned16(resid) || !aligned16(y32) || !aligned16(Wt) ||
        !aligned16(x_out) || !aligned16(h_out))
        return BD_E_BAD_SHAPE;
    hipStream_t st = (hipStream_t)stream;
    if (dtype == BD_BF16)
        hipLaunchKernelGGL((add_rmsnorm_kernel<DT_BF16>), dim3(rows), dim3(256), 0, st, (const unsigned short*)resid, y32, (const unsigned short*)Wt,
                           (unsigned short*)x_out, (unsigned short*)h_out, H, (long long)s_r, (long long)s_y, (long long)s_x, (long long)s_h,
                           (long long)sw, rows_per_tenant, eps);
    else
        hipLaunchKernelGGL((add_rmsnorm_kernel<DT_F16>), dim3(rows), dim3(256), 0, st, (const unsigned short*)resid, y32, (const unsigned short*)Wt,
                           (unsigned short*)x_out, (unsigned short*)h_out, H, (long long)s_r, (long long)s_y, (long long)s_x, (long long)s_h,
                           (long long)sw, rows_per_tenant, eps);
    return launch_status();
}

extern "C" int bd_srv_swiglu(const void* G, const void* U, void* Y, int rows, int I, int64_t sg, int64_t su, int64_t sy,
                             int interleaved8, int dtype, void* stream) {
    if (rows < 0 || I < 0 || rows > 65535) return BD_E_BAD_SHAPE;
    if (dtype != BD_F16 && dtype != BD_BF16) return BD_E_BAD_DTYPE;
    if (rows == 0 || I == 0) return BD_OK;
    if (!G || !U || !Y) return BD_E_NULL;
    if (I % 8 || sg % 8 || su % 8 || sy % 8 || !aligned16(G) || !aligned16(U) || !aligned16(Y)) return BD_E_BAD_SHAPE;
    if (interleaved8 && G == Y) return BD_E_BAD_SHAPE;       // (in place is fine for the split form only)
    hipStream_t st = (hipStream_t)stream;
    dim3 grid((unsigned)((I / 8 + 255) / 256), (unsigned)rows);
    if (dtype == BD_BF16)
        hipLaunchKernelGGL((swiglu_kernel<DT_BF16>), grid, dim3(256), 0, st, (const unsigned short*)G, (const unsigned short*)U,
                           (unsigned short*)Y, I, (long long)sg, (long long)su, (long long)sy, interleaved8 ? 1 : 0);
    else
        hipLaunchKernelGGL((swiglu_kernel<DT_F16>), grid, dim3(256), 0, st, (const unsigned short*)G, (const unsigned short*)U,
                           (unsigned short*)Y, I, (long long)sg, (long long)su, (long long)sy, interleaved8 ? 1 : 0);
    return launch_status();
}

// Per-tenant rotary tables (the *_tab entries): s_tab is the tenant stride of cos_t / sin_t in elements, 0 = one table for every tenant.  Each
// shared-table entry is its *_tab sibling at s_tab = 0: one launcher and one kernel per pair.  The stride keeps every tenant's rows 16-byte
// aligned (the rope kernels read the tables in 16-byte chunks), so it is a multiple of 8 elements.
static inline bool tab_stride_ok(int64_t s_tab) { return s_tab >= 0 && s_tab % 8 == 0; }

extern "C" int bd_srv_rope_tab(void* X, const void* cos_t, const void* sin_t, int64_t s_tab, int rows, int heads, int head_dim, int64_t sx,
                               int seq, int pos0, int dtype, void* stream) {
    if (rows < 0 || heads < 1 || seq < 1 || pos0 < 0 || !tab_stride_ok(s_tab)) return BD_E_BAD_SHAPE;
    if (dtype != BD_F16 && dtype != BD_BF16) return BD_E_BAD_DTYPE;
    if (rows == 0) return BD_OK;
    if (!X || !cos_t || !sin_t) return BD_E_NULL;
    if (head_dim != 128 || sx % 8 || !aligned16(X) || !aligned16(cos_t) || !aligned16(sin_t)) return BD_E_BAD_SHAPE;
    hipStream_t st = (hipStream_t)stream;
    if (dtype == BD_BF16)
        hipLaunchKernelGGL((rope_kernel<DT_BF16>), dim3(rows), dim3(256), 0, st, (unsigned short*)X, (const unsigned short*)cos_t,
                           (const unsigned short*)sin_t, (long long)s_tab, heads, (long long)sx, seq, pos0);
    else
        hipLaunchKernelGGL((rope_kernel<DT_F16>), dim3(rows), dim3(256), 0, st, (unsigned short*)X, (const unsigned short*)cos_t,
                           (const unsigned short*)sin_t, (long long)s_tab, heads, (long long)sx, seq, pos0);
    return launch_status();
}

extern "C" int bd_srv_rope(void* X, const void* cos_t, const void* sin_t, int rows, int heads, int head_dim, int64_t sx, int seq,
                           int pos0, int dtype, void* stream) {
    return bd_srv_rope_tab(X, cos_t, sin_t, 0, rows, heads, head_dim, sx, seq, pos0, dtype, stream);
}

extern "C" int bd_srv_rope_kv_append_tab(void* QKV, const void* cos_t, const void* sin_t, int64_t s_tab, void* kcache, void* vcache, int T, int S,
                                         int H, int KVH, int head_dim, int64_t sx, int Lc, int pos0, int dtype, void* stream) {
    if (T < 0 || S < 0 || H < 1 || KVH < 1 || pos0 < 0 || Lc < 1 || !tab_stride_ok(s_tab)) return BD_E_BAD_SHAPE;
    if (dtype != BD_F16 && dtype != BD_BF16) return BD_E_BAD_DTYPE;
    if (T == 0 || S == 0) return BD_OK;
    if (!QKV || !cos_t || !sin_t || !kcache || !vcache) return BD_E_NULL;
    if (head_dim != 128 || sx % 8 || sx < (int64_t)(H + 2 * KVH) * 128 || (int64_t)pos0 + S > Lc || (int64_t)T * S >= (1ll << 31) ||
        !aligned16(QKV) || !aligned16(cos_t) || !aligned16(sin_t) || !aligned16(kcache) || !aligned16(vcache))
        return BD_E_BAD_SHAPE;
    hipStream_t st = (hipStream_t)stream;
    if (dtype == BD_BF16)
        hipLaunchKernelGGL((rope_kv_append_kernel<DT_BF16>), dim3((unsigned)(T * S)), dim3(256), 0, st, (unsigned short*)QKV,
                           (const unsigned short*)cos_t, (const unsigned short*)sin_t, (long long)s_tab, (unsigned short*)kcache,
                           (unsigned short*)vcache, H, KVH, (long long)sx, S, pos0, Lc);
    else
        hipLaunchKernelGGL((rope_kv_append_kernel<DT_F16>), dim3((unsigned)(T * S)), dim3(256), 0, st, (unsigned short*)QKV,
                           (const unsigned short*)cos_t, (const unsigned short*)sin_t, (long long)s_tab, (unsigned short*)kcache,
                           (unsigned short*)vcache, H, KVH, (long long)sx, S, pos0, Lc);
    return launch_status();
}

extern "C" int bd_srv_rope_kv_append(void* QKV, const void* cos_t, const void* sin_t, void* kcache, void* vcache, int T, int S, int H, int KVH,
                                     int head_dim, int64_t sx, int Lc, int pos0, int dtype, void* stream) {
    return bd_srv_rope_kv_append_tab(QKV, cos_t, sin_t, 0, kcache, vcache, T, S, H, KVH, head_dim, sx, Lc, pos0, dtype, stream);
}

extern "C" int bd_srv_step_begin(const void* embed, int64_t sEt, int64_t sEv, const int64_t* tok, void* X, int64_t sx, void* valid, int Lc,
                                 const int64_t* pos, int T, int V, int H, void* stream) {
    if (T < 0 || V < 1 || H < 1 || Lc < 1) return BD_E_BAD_SHAPE;
    if (T == 0) return BD_OK;
    if (!embed || !tok || !X || !valid || !pos) return BD_E_NULL;
    if (H % 8 || sEv % 8 || sEt % 8 || sx % 8 || sEv < H || sx < H || sEt < 0 || !aligned16(embed) || !aligned16(X)) return BD_E_BAD_SHAPE;
    hipLaunchKernelGGL(step_begin_kernel, dim3((unsigned)T), dim3(256), 0, (hipStream_t)stream, (const unsigned short*)embed, (long long)sEt,
                       (long long)sEv, (const long long*)tok, (unsigned short*)X, (long long)sx, (unsigned char*)valid, Lc, (const long long*)pos, V, H);
    return launch_status();
}

extern "C" int bd_srv_step_end(const void* logits, int64_t sl, int V, int64_t* tok, int64_t* out, int64_t s_out, int out_cap,
                               const int64_t* stop_ids, int ns, void* stopped, int64_t* pos, int64_t* step, void* ticket, int T, int dtype,
                               void* stream) {
    if (T < 0 || V < 1 || ns < 0 || out_cap < 0) return BD_E_BAD_SHAPE;
    if (dtype != BD_F16 && dtype != BD_BF16) return BD_E_BAD_DTYPE;
    if (T == 0) return BD_OK;
    if (!logits || !tok || !out || !stopped || !pos || !step || !ticket || (ns > 0 && !stop_ids)) return BD_E_NULL;
    if (V % 8 || sl % 8 || sl < V || s_out < out_cap || !aligned16(logits) || ((uintptr_t)ticket & 3)) return BD_E_BAD_SHAPE;
    hipStream_t st = (hipStream_t)stream;
    if (dtype == BD_BF16)
        hipLaunchKernelGGL((step_end_kernel<DT_BF16>), dim3((unsigned)T), dim3(256), 0, st, (const unsigned short*)logits, (long long)sl, V,
                           (long long*)tok, (long long*)out, (long long)s_out, out_cap, (const long long*)stop_ids, ns, (unsigned char*)stopped,
                           (long long*)pos, (long long*)step, (unsigned int*)ticket, T);
    else
        hipLaunchKernelGGL((step_end_kernel<DT_F16>), dim3((unsigned)T), dim3(256), 0, st, (const unsigned short*)logits, (long long)sl, V,
                           (long long*)tok, (long long*)out, (long long)s_out, out_cap, (const long long*)stop_ids, ns, (unsigned char*)stopped,
                           (long long*)pos, (long long*)step, (unsigned int*)ticket, T);
    return launch_status();
}

extern "C" int bd_srv_step_begin_ragged(const void* embed, int64_t sEt, int64_t sEv, const int64_t* tok, void* X, int64_t sx, void* valid, int Lc,
                                        const int64_t* pos, const void* active, int T, int V, int H, void* stream) {
    if (T < 0 || V < 1 || H < 1 || Lc < 1) return BD_E_BAD_SHAPE;
    if (T == 0) return BD_OK;
    if (!embed || !tok || !X || !valid || !pos || !active) return BD_E_NULL;
    if (H % 8 || sEv % 8 || sEt % 8 || sx % 8 || sEv < H || sx < H || sEt < 0 || !aligned16(embed) || !aligned16(X)) return BD_E_BAD_SHAPE;
    hipLaunchKernelGGL(step_begin_ragged_kernel, dim3((unsigned)T), dim3(256), 0, (hipStream_t)stream, (const unsigned short*)embed, (long long)sEt,
                       (long long)sEv, (const long long*)tok, (unsigned short*)X, (long long)sx, (unsigned char*)valid, Lc, (const long long*)pos,
                       (const unsigned char*)active, V, H);
    return launch_status();
}

extern "C" int bd_srv_step_end_ragged(const void* logits, int64_t sl, int V, int64_t* tok, int64_t* out, int64_t s_out, int out_cap,
                                      const int64_t* stop_ids, int ns, int64_t* pos, int64_t* n, const int64_t* limit, void* active, void* done,
                                      int Lc, int T, int dtype, void* stream) {
    if (T < 0 || V < 1 || ns < 0 || out_cap < 0 || Lc < 1) return BD_E_BAD_SHAPE;
    if (dtype != BD_F16 && dtype != BD_BF16) return BD_E_BAD_DTYPE;
    if (T == 0) return BD_OK;
    if (!logits || !tok || !out || !pos || !n || !limit || !active || !done || (ns > 0 && !stop_ids)) return BD_E_NULL;
    if (V % 8 || sl % 8 || sl < V || s_out < out_cap || !aligned16(logits)) return BD_E_BAD_SHAPE;
    hipStream_t st = (hipStream_t)stream;
    if (dtype == BD_BF16)
        hipLaunchKernelGGL((step_end_ragged_kernel<DT_BF16>), dim3((unsigned)T), dim3(256), 0, st, (const unsigned short*)logits, (long long)sl, V,
                           (long long*)tok, (long long*)out, (long long)s_out, out_cap, (const long long*)stop_ids, ns, (long long*)pos,
                           (long long*)n, (const long long*)limit, (unsigned char*)active, (unsigned char*)done, Lc);
    else
        hipLaunchKernelGGL((step_end_ragged_kernel<DT_F16>), dim3((unsigned)T), dim3(256), 0, st, (const unsigned short*)logits, (long long)sl, V,
                           (long long*)tok, (long long*)out, (long long)s_out, out_cap, (const long long*)stop_ids, ns, (long long*)pos,
                           (long long*)n, (const long long*)limit, (unsigned char*)active, (unsigned char*)done, Lc);
    return launch_status();
}

static inline bool aligned_to(const void* p, uintptr_t a) { return ((uintptr_t)p & (a - 1)) == 0; }

extern "C" int bd_srv_sample_rows(const void* logits, int64_t sl, int V, const float* temperature, const int32_t* top_k, const float* top_p,
                                  const int64_t* seed, const int64_t* draw, int64_t* tok, int32_t* dbg, int R, int dtype, void* stream) {
    if (R < 0 || V < 1) return BD_E_BAD_SHAPE;
    if (dtype != BD_F16 && dtype != BD_BF16) return BD_E_BAD_DTYPE;
    if (R == 0) return BD_OK;
    if (!logits || !temperature || !top_k || !top_p || !seed || !draw || !tok) return BD_E_NULL;
    if (V % 8 || sl % 8 || sl < V || !aligned16(logits) || !aligned_to(temperature, 4) || !aligned_to(top_k, 4) || !aligned_to(top_p, 4) ||
        !aligned_to(seed, 8) || !aligned_to(draw, 8) || !aligned_to(tok, 8) || !aligned_to(dbg, 4))
        return BD_E_BAD_SHAPE;
    hipStream_t st = (hipStream_t)stream;
    if (dtype == BD_BF16)
        hipLaunchKernelGGL((sample_rows_kernel<DT_BF16>), dim3((unsigned)R), dim3(256), 0, st, (const unsigned short*)logits, (long long)sl, V,
                           temperature, (const int*)top_k, top_p, (const long long*)seed, (const long long*)draw, (long long*)tok, (int*)dbg);
    else
        hipLaunchKernelGGL((sample_rows_kernel<DT_F16>), dim3((unsigned)R), dim3(256), 0, st, (const unsigned short*)logits, (long long)sl, V,
                           temperature, (const int*)top_k, top_p, (const long long*)seed, (const long long*)draw, (long long*)tok, (int*)dbg);
    return launch_status();
}

extern "C" int bd_srv_step_end_sample(const void* logits, int64_t sl, int V, int64_t* tok, int64_t* out, int64_t s_out, int out_cap,
                                      const int64_t* stop_ids, int ns, int64_t* pos, int64_t* n, const int64_t* limit, void* active, void* done,
                                      int Lc, const float* temperature, const int32_t* top_k, const float* top_p, const int64_t* seed,
                                      int32_t* dbg, int T, int dtype, void* stream) {
    if (T < 0 || V < 1 || ns < 0 || out_cap < 0 || Lc < 1) return BD_E_BAD_SHAPE;
    if (dtype != BD_F16 && dtype != BD_BF16) return BD_E_BAD_DTYPE;
    if (T == 0) return BD_OK;
    if (!logits || !tok || !out || !pos || !n || !limit || !active || !done || (ns > 0 && !stop_ids) || !temperature || !top_k || !top_p || !seed)
        return BD_E_NULL;
    if (V % 8 || sl % 8 || sl < V || s_out < out_cap || !aligned16(logits) || !aligned_to(temperature, 4) || !aligned_to(top_k, 4) ||
        !aligned_to(top_p, 4) || !aligned_to(seed, 8) || !aligned_to(dbg, 4))
        return BD_E_BAD_SHAPE;
    hipStream_t st = (hipStream_t)stream;
    if (dtype == BD_BF16)
        hipLaunchKernelGGL((step_end_sample_kernel<DT_BF16>), dim3((unsigned)T), dim3(256), 0, st, (const unsigned short*)logits, (long long)sl, V,
                           (long long*)tok, (long long*)out, (long long)s_out, out_cap, (const long long*)stop_ids, ns, (long long*)pos,
                           (long long*)n, (const long long*)limit, (unsigned char*)active, (unsigned char*)done, Lc, temperature,
                           (const int*)top_k, top_p, (const long long*)seed, (int*)dbg);
    else
        hipLaunchKernelGGL((step_end_sample_kernel<DT_F16>), dim3((unsigned)T), dim3(256), 0, st, (const unsigned short*)logits, (long long)sl, V,
                           (long long*)tok, (long long*)out, (long long)s_out, out_cap, (const long long*)stop_ids, ns, (long long*)pos,
                           (long long*)n, (const long long*)limit, (unsigned char*)active, (unsigned char*)done, Lc, temperature,
                           (const int*)top_k, top_p, (const long long*)seed, (int*)dbg);
    return launch_status();
}

extern "C" int bd_srv_cache_warm(const void* p0, int64_t bytes0, const void* p1, int64_t bytes1, int blocks, void* stream) {
    if (bytes0 < 0 || bytes1 < 0 || blocks < 0) return BD_E_BAD_SHAPE;
    if ((bytes0 && !p0) || (bytes1 && !p1)) return BD_E_NULL;
    if ((bytes0 && !aligned16(p0)) || (bytes1 && !aligned16(p1))) return BD_E_BAD_SHAPE;
    if (bytes0 / 16 + bytes1 / 16 == 0) return BD_OK;
    if (blocks == 0) blocks = num_cus();
    hipLaunchKernelGGL(cache_warm_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, (const u32x4_t*)p0, (long long)(bytes0 / 16),
                       (const u32x4_t*)p1, (long long)(bytes1 / 16));
    return launch_status();
}

#ifndef BD_ATTN_SPLITS
#define BD_ATTN_SPLITS 4
#endif
constexpr int ATTN_SPLITS = BD_ATTN_SPLITS;   // (a build-time knob for A/B runs; 4 measured best at 6 tenants x 8 kv heads, profiles/r03_decode_attn_splits.txt, r05_decode_step.txt)
constexpr int ATTN_SPLITS_MAX = 16;
static_assert(ATTN_SPLITS <= 4, "decode_attn_kernel<.., MAXS = 4> merges at most 4 partials");
constexpr int64_t ATTN_TICKET_BYTES = 16384;       // one arrival counter per (tenant, kv head): T * KVH <= 4096
static thread_local int g_attn_splits_max = env_int("BD_ATTN_SPLITS_MAX", ATTN_SPLITS_MAX);       // A/B hook: 4 = the fixed split count of rounds 3 - 5
// key-range splits of a launch: ATTN_SPLITS, doubled while the launch would still cover at most a QUARTER of the CUs (one or two sequences of a
// grouped-query model: a single sequence on 8 kv heads is 32 blocks at 4 splits -- and the launch is a dependent chain of memory round trips, so
// fewer rows per block = fewer load rounds), never more than one split per 32 cache rows.  Same-box A/B, Mistral-7B, 4 -> this rule (tools/gpu_r5y.sh):
// 1 tenant 3.319 -> 3.275 ms/step (-1.3 %, 16 splits), 2 tenants 3.548 -> 3.544 (8 splits); doubling up to HALF of the CUs was +0.6 % at 4 tenants
// (8 splits, 256 blocks), so 32 (tenant, kv head) pairs and more keep 4.  A function of (T, KVH, Lc) only.
inline int attn_splits(int T, int KVH, int Lc) {
    if (Lc < 256) return 1;                                       // short caches run unsplit
    int ns = ATTN_SPLITS;
    const int cap = g_attn_splits_max < ATTN_SPLITS ? ATTN_SPLITS : (g_attn_splits_max > ATTN_SPLITS_MAX ? ATTN_SPLITS_MAX : g_attn_splits_max);
    while (ns * 2 <= cap && (int64_t)T * KVH * ns * 4 <= num_cus() && ns * 2 * 32 <= Lc) ns *= 2;
    return ns;
}
extern "C" int64_t bd_srv_decode_attention_workspace_bytes(int T, int H, int KVH, int head_dim, int Lc) {
    if (T <= 0 || H <= 0 || KVH <= 0 || Lc < 256) return 0;       // short caches run unsplit
    return ATTN_TICKET_BYTES + (int64_t)T * H * ATTN_SPLITS_MAX * (head_dim + 2) * 4;      // (sized for the largest split count: independent of the A/B hook)
}

// bd_srv_decode_attention and its ragged form: ONE body, so validation, split rule, workspace layout and depth rule cannot drift apart (a ragged
// launch at equal positions has the scalar launch's geometry).  RAGGED: pos is [T] and `active` [T] bytes.
// s_tab: tenant stride of the rotary tables (the *_tab entries; the shared-table entries pass 0 and tab_entry = false, which keeps their
// validation as it was: they never asked for aligned tables, the kernel reads them element by element).
template <bool RAGGED>
static int decode_attention_launch(const void* QKV, const void* cos_t, const void* sin_t, int64_t s_tab, bool tab_entry, void* kcache, void* vcache,
                                   void* valid, const int64_t* pos, const void* active, void* out, int T, int H, int KVH, int head_dim, int Lc,
                                   int64_t s_qkv, int64_t s_out, int dtype, void* ws, int64_t ws_bytes, void* stream) {
    if (T < 0 || H < 1 || KVH < 1 || H % KVH || Lc < 1 || !tab_stride_ok(s_tab)) return BD_E_BAD_SHAPE;
    if (dtype != BD_F16 && dtype != BD_BF16) return BD_E_BAD_DTYPE;
    if (T == 0) return BD_OK;
    if (!QKV || !cos_t || !sin_t || !kcache || !vcache || !valid || !pos || !out || (RAGGED && !active)) return BD_E_NULL;
    const int G = H / KVH;
    if (head_dim != 128 || (G != 1 && G != 4 && G != 8) || s_qkv % 8 || !aligned16(QKV) || !aligned16(kcache) || !aligned16(vcache) ||
        (tab_entry && (!aligned16(cos_t) || !aligned16(sin_t))))
        return BD_E_BAD_SHAPE;                         // other head geometries: the caller keeps its torch attention
    AttnParams p;
    p.qkv = (const unsigned short*)QKV; p.cos = (const unsigned short*)cos_t; p.sin = (const unsigned short*)sin_t; p.s_tab = s_tab;
    p.kc = (unsigned short*)kcache; p.vc = (unsigned short*)vcache; p.valid = (unsigned char*)valid; p.pos = (const long long*)pos;
    p.active = (const unsigned char*)active;
    p.out = (unsigned short*)out; p.T = T; p.H = H; p.KVH = KVH; p.Lc = Lc; p.s_qkv = s_qkv; p.s_out = s_out;
    p.scale = 1.0f / sqrtf((float)head_dim);
    // split the key range over 4 blocks per (tenant, kv head) when the cache is long enough and a workspace is given: T * KVH blocks
    // alone leave most CUs (and most of HBM) idle -- one CU streams only ~12-25 GB/s
    // A workspace smaller than bd_srv_decode_attention_workspace_bytes() -- e.g. sized by a caller with the round-4 formula, which covered 4
    // splits -- gets the LARGEST split count it holds (16 -> 8 -> 4 -> 2), not a silent fall to the unsplit launch: partials are
    // indexed [tenant][head][split of nsplit], so any count whose T * H * nsplit records fit behind the ticket area is valid.
    const int64_t need = bd_srv_decode_attention_workspace_bytes(T, H, KVH, head_dim, Lc);
    p.nsplit = 1;
    if (need > 0 && ws && ws_bytes > ATTN_TICKET_BYTES && (int64_t)T * KVH * 4 <= ATTN_TICKET_BYTES) {
        const int64_t fit = (ws_bytes - ATTN_TICKET_BYTES) / ((int64_t)T * H * (head_dim + 2) * 4);
        int ns = attn_splits(T, KVH, Lc);
        while (ns > 1 && ns > fit) ns >>= 1;
        p.nsplit = ns;
    }
    p.tickets = (unsigned*)ws;
    p.ws = (float*)((char*)ws + ATTN_TICKET_BYTES);
    hipStream_t st = (hipStream_t)stream;
    dim3 grid((unsigned)(T * KVH), (unsigned)p.nsplit);
#define BD_ATT(DT, GG)                                                                                      \
    do {                                                                                                    \
        const bool d2_ = g_attn_depth ? g_attn_depth == 2 : Lc <= 2048;                                                    \
        t_last_attention_form = p.nsplit | (d2_ ? 2 : 4) << 8 | (p.nsplit <= 4 ? 4 : 16) << 16 | GG << 24;                 \
        if (p.nsplit <= 4) {                                                                                               \
            if (d2_) hipLaunchKernelGGL((decode_attn_kernel<DT, GG, 2, 4, RAGGED>), grid, dim3(512), 0, st, p);                    \
            else hipLaunchKernelGGL((decode_attn_kernel<DT, GG, 4, 4, RAGGED>), grid, dim3(512), 0, st, p);                        \
        } else {                                                                                                           \
            if (d2_) hipLaunchKernelGGL((decode_attn_kernel<DT, GG, 2, 16, RAGGED>), grid, dim3(512), 0, st, p);                   \
            else hipLaunchKernelGGL((decode_attn_kernel<DT, GG, 4, 16, RAGGED>), grid, dim3(512), 0, st, p);                       \
        }                                                                                                                  \
    } while (0)
    // G = query heads per kv head: 1 (Llama-2-7B), 4 (Mistral-7B), 8 (Llama-2-70B -- also per rank under tensor parallelism).
    // Depth of the K / V row ring: 2 iterations for caches of up to 2048 positions (a split is then <= 16 iterations; 4.698 -> 4.661 ms on the
    // 6-tenant step at 512 keys, one iteration: 4.649 but exposed to the full load latency on long splits), 4 beyond
    if (dtype == BD_BF16) { if (G == 1) BD_ATT(DT_BF16, 1); else if (G == 4) BD_ATT(DT_BF16, 4); else BD_ATT(DT_BF16, 8); }
    else { if (G == 1) BD_ATT(DT_F16, 1); else if (G == 4) BD_ATT(DT_F16, 4); else BD_ATT(DT_F16, 8); }
#undef BD_ATT
    return launch_status();
}

extern "C" int bd_srv_decode_attention(const void* QKV, const void* cos_t, const void* sin_t, void* kcache, void* vcache,
                                       void* valid, const int64_t* pos, void* out, int T, int H, int KVH, int head_dim, int Lc,
                                       int64_t s_qkv, int64_t s_out, int dtype, void* ws, int64_t ws_bytes, void* stream) {
    return decode_attention_launch<false>(QKV, cos_t, sin_t, 0, false, kcache, vcache, valid, pos, nullptr, out, T, H, KVH, head_dim, Lc, s_qkv, s_out,
                                          dtype, ws, ws_bytes, stream);
}

extern "C" int bd_srv_decode_attention_ragged(const void* QKV, const void* cos_t, const void* sin_t, void* kcache, void* vcache,
                                              void* valid, const int64_t* pos, const void* active, void* out, int T, int H, int KVH, int head_dim,
                                              int Lc, int64_t s_qkv, int64_t s_out, int dtype, void* ws, int64_t ws_bytes, void* stream) {
    return decode_attention_launch<true>(QKV, cos_t, sin_t, 0, false, kcache, vcache, valid, pos, active, out, T, H, KVH, head_dim, Lc, s_qkv, s_out,
                                         dtype, ws, ws_bytes, stream);
}

extern "C" int bd_srv_decode_attention_tab(const void* QKV, const void* cos_t, const void* sin_t, int64_t s_tab, void* kcache, void* vcache,
                                           void* valid, const int64_t* pos, void* out, int T, int H, int KVH, int head_dim, int Lc,
                                           int64_t s_qkv, int64_t s_out, int dtype, void* ws, int64_t ws_bytes, void* stream) {
    return decode_attention_launch<false>(QKV, cos_t, sin_t, s_tab, true, kcache, vcache, valid, pos, nullptr, out, T, H, KVH, head_dim, Lc, s_qkv,
                                          s_out, dtype, ws, ws_bytes, stream);
}

extern "C" int bd_srv_decode_attention_ragged_tab(const void* QKV, const void* cos_t, const void* sin_t, int64_t s_tab, void* kcache, void* vcache,
                                                  void* valid, const int64_t* pos, const void* active, void* out, int T, int H, int KVH,
                                                  int head_dim, int Lc, int64_t s_qkv, int64_t s_out, int dtype, void* ws, int64_t ws_bytes,
                                                  void* stream) {
    return decode_attention_launch<true>(QKV, cos_t, sin_t, s_tab, true, kcache, vcache, valid, pos, active, out, T, H, KVH, head_dim, Lc, s_qkv,
                                         s_out, dtype, ws, ws_bytes, stream);
}

extern "C" int bd_srv_prefill_attention(const void* Q, const void* K, const void* V, void* O, int B, int S, int H, int KVH, int head_dim,
                                        int64_t sqb, int64_t sqs, int64_t skb, int64_t sks, int64_t svb, int64_t svs,
                                        int64_t sob, int64_t sos, const int32_t* kv_start, float scale, int causal, int dtype,
                                        void* stream) {
    if (B < 0 || S < 0 || H < 1 || KVH < 1 || H % KVH) return BD_E_BAD_SHAPE;
    if (dtype != BD_F16 && dtype != BD_BF16) return BD_E_BAD_DTYPE;
    if (B == 0 || S == 0) return BD_OK;
    if (!Q || !K || !V || !O) return BD_E_NULL;
    // other geometries: the caller keeps its torch attention
    if (head_dim != 128 || S % 64 || (sqs | sks | svs | sos | sqb | skb | svb | sob) % 8 || !aligned16(Q) || !aligned16(K) || !aligned16(V) ||
        !aligned16(O) || (int64_t)B * H * ((S + 127) / 128) > 0x7fffffffLL)
        return BD_E_BAD_SHAPE;
    PrefillAttnParams p;
    p.q = (const unsigned short*)Q; p.k = (const unsigned short*)K; p.v = (const unsigned short*)V; p.o = (unsigned short*)O;
    p.sqb = sqb; p.sqs = sqs; p.skb = skb; p.sks = sks; p.svb = svb; p.svs = svs; p.sob = sob; p.sos = sos;
    p.kv_start = kv_start; p.B = B; p.S = S; p.H = H; p.KVH = KVH; p.nqb = (S + 127) / 128;
    p.c = scale * 1.4426950408889634f; p.causal = causal ? 1 : 0;
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid((unsigned)(p.nqb * H * B));
    static std::atomic<uint64_t> lds_done[2];               // the kernel needs more than the default dynamic LDS limit
    const int di = dtype == BD_BF16 ? 1 : 0;
    const void* fn = di ? (const void*)prefill_attn_kernel<DT_BF16> : (const void*)prefill_attn_kernel<DT_F16>;
    if (!ensure_dyn_lds(fn, PREFILL_ATTN_LDS, lds_done[di])) return BD_E_LAUNCH;
    if (di) hipLaunchKernelGGL((prefill_attn_kernel<DT_BF16>), grid, dim3(256), PREFILL_ATTN_LDS, st, p);
    else hipLaunchKernelGGL((prefill_attn_kernel<DT_F16>), grid, dim3(256), PREFILL_ATTN_LDS, st, p);
    return launch_status();
}

// ------------------------------------------------------------------ binarize / merge
extern "C" int64_t bd_binarize_workspace_bytes(int64_t N, int64_t K) {
    if (N <= 0 || K <= 0) return 0;
    return ((N + 63) / 64) * ((K + 255) / 256) * 4;
}

extern "C" int bd_binarize(const void* base, const void* fine, int64_t N, int64_t K, int64_t ld, int dtype, int32_t* mask,
                           float* coeff, void* ws, int64_t ws_bytes, void* stream) {
    if (N < 0 || K < 0 || N > (1LL << 30) || K > (1LL << 30)) return BD_E_BAD_SHAPE;
    if (K % 32) return BD_E_K_NOT_MULTIPLE;
    if (dtype != BD_F16 && dtype != BD_BF16) return BD_E_BAD_DTYPE;
    if (N == 0 || K == 0) return BD_OK;
    if (!base || !fine || !mask || !coeff) return BD_E_NULL;
    const int64_t need = bd_binarize_workspace_bytes(N, K);
    if (!ws || ws_bytes < need) return BD_E_WORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    dim3 grid((unsigned)((N + 63) / 64), (unsigned)((K + 255) / 256));
    if (grid.y > 65535) return BD_E_BAD_SHAPE;
    const int nparts = (int)(grid.x * grid.y);
    if (dtype == BD_BF16)
        hipLaunchKernelGGL((binarize_kernel<DT_BF16>), grid, dim3(256), 0, st, (const unsigned short*)base,
                           (const unsigned short*)fine, (uint32_t*)mask, (float*)ws, (int)N, (int)K, (long long)ld);
    else
        hipLaunchKernelGGL((binarize_kernel<DT_F16>), grid, dim3(256), 0, st, (const unsigned short*)base,
                           (const unsigned short*)fine, (uint32_t*)mask, (float*)ws, (int)N, (int)K, (long long)ld);
    hipLaunchKernelGGL(binarize_finish_kernel, dim3(1), dim3(256), 0, st, (const float*)ws, nparts,
                       1.0 / ((double)N * (double)K), coeff);
    return launch_status();
}

extern "C" int bd_merge_delta(void* W, int64_t ldw, const int32_t* P, const float* coeff, int64_t N, int64_t K, int dtype,
                              void* stream) {
    if (N < 0 || K < 0 || N > (1LL << 30) || K > (1LL << 30)) return BD_E_BAD_SHAPE;
    if (K % 32) return BD_E_K_NOT_MULTIPLE;
    if (dtype != BD_F16 && dtype != BD_BF16) return BD_E_BAD_DTYPE;
    if (N == 0 || K == 0) return BD_OK;
    if (!W || !P || !coeff) return BD_E_NULL;
    hipStream_t st = (hipStream_t)stream;
    dim3 grid((unsigned)((N + 63) / 64), (unsigned)((K + 255) / 256));
    if (grid.y > 65535) return BD_E_BAD_SHAPE;
    if (dtype == BD_BF16)
        hipLaunchKernelGGL((merge_kernel<DT_BF16>), grid, dim3(256), 0, st, (unsigned short*)W, (const uint32_t*)P, coeff,
                           (int)N, (int)K, (long long)ldw);
    else
        hipLaunchKernelGGL((merge_kernel<DT_F16>), grid, dim3(256), 0, st, (unsigned short*)W, (const uint32_t*)P, coeff,
                           (int)N, (int)K, (long long)ldw);
    return launch_status();
}

// (last in the file: the kernels of a code object lie in the order the host code asks for them, and the decode step is sensitive to where
// its kernels lie -- profiles/decode_dispatch_refactor.txt; a new entry goes behind every kernel that exists)
extern "C" int bd_srv_prefill_attention_cached(const void* Q, const void* Kc, const void* Vc, void* O, int B, int Sq, int H, int KVH, int head_dim,
                                               int q0, int Lc, int64_t sqb, int64_t sqs, int64_t skb, int64_t skh, int64_t sks, int64_t svb,
                                               int64_t svh, int64_t svs, int64_t sob, int64_t sos, const int32_t* kv_start, float scale, int dtype,
                                               void* stream) {
    // every check below is host arithmetic: nothing touches the device before the geometry is known to be the kernel's
    if (B < 0 || H < 1 || KVH < 1 || H % KVH || Sq < 1 || q0 < 0 || Lc < 1 || (int64_t)q0 + Sq > Lc) return BD_E_BAD_SHAPE;
    if (dtype != BD_F16 && dtype != BD_BF16) return BD_E_BAD_DTYPE;
    if (B == 0) return BD_OK;
    if (!Q || !Kc || !Vc || !O) return BD_E_NULL;
    if (head_dim != 128 || (sqb | sqs | skb | skh | sks | svb | svh | svs | sob | sos) % 8 || !aligned16(Q) || !aligned16(Kc) || !aligned16(Vc) ||
        !aligned16(O) || (int64_t)B * H * ((Sq + 127) / 128) > 0x7fffffffLL)
        return BD_E_BAD_SHAPE;
    PrefillAttnCachedParams p;
    p.q = (const unsigned short*)Q; p.k = (const unsigned short*)Kc; p.v = (const unsigned short*)Vc; p.o = (unsigned short*)O;
    p.sqb = sqb; p.sqs = sqs; p.skb = skb; p.skh = skh; p.sks = sks; p.svb = svb; p.svh = svh; p.svs = svs; p.sob = sob; p.sos = sos;
    p.kv_start = kv_start; p.B = B; p.Sq = Sq; p.H = H; p.KVH = KVH; p.nqb = (Sq + 127) / 128; p.q0 = q0; p.Lc = Lc;
    p.c = scale * 1.4426950408889634f;
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid((unsigned)(p.nqb * H * B));
    static std::atomic<uint64_t> lds_done[2];               // the kernel needs more than the default dynamic LDS limit
    const int di = dtype == BD_BF16 ? 1 : 0;
    const void* fn = di ? (const void*)prefill_attn_kernel<DT_BF16, true> : (const void*)prefill_attn_kernel<DT_F16, true>;
    if (!ensure_dyn_lds(fn, PREFILL_ATTN_LDS, lds_done[di])) return BD_E_LAUNCH;
    if (di) hipLaunchKernelGGL((prefill_attn_kernel<DT_BF16, true>), grid, dim3(256), PREFILL_ATTN_LDS, st, p);
    else hipLaunchKernelGGL((prefill_attn_kernel<DT_F16, true>), grid, dim3(256), PREFILL_ATTN_LDS, st, p);
    return launch_status();
}

// (behind every kernel that existed before it: see the note above bd_srv_prefill_attention_cached)
extern "C" int bd_srv_token_nll(const void* logits, int64_t sl, int V, const int64_t* labels, float* nll, float* lse, int R, int dtype,
                                void* stream) {
    if (R < 0 || V < 1 || V > NLL_V_MAX) return BD_E_BAD_SHAPE;
    if (dtype != BD_F16 && dtype != BD_BF16) return BD_E_BAD_DTYPE;
    if (R == 0) return BD_OK;
    if (!logits || !labels || !nll) return BD_E_NULL;
    if (sl % 8 || sl < V || !aligned16(logits) || !aligned_to(labels, 8) || !aligned_to(nll, 4) || !aligned_to(lse, 4)) return BD_E_BAD_SHAPE;
    hipStream_t st = (hipStream_t)stream;
    // the form depends on V alone: <= 8192 / <= 32768 hold the row in 4 / 16 sixteen-byte registers per thread, longer rows are read twice
#define BD_NLL_LAUNCH(DT, NV)                                                                                                           \
    hipLaunchKernelGGL((token_nll_kernel<DT, NV>), dim3((unsigned)R), dim3(256), 0, st, (const unsigned short*)logits, (long long)sl, V, \
                       (const long long*)labels, nll, lse)
    const int nv = V <= 2048 * 4 ? 4 : V <= 2048 * NLL_NV_MAX ? NLL_NV_MAX : 0;
    if (dtype == BD_BF16) {
        if (nv == 4) BD_NLL_LAUNCH(DT_BF16, 4); else if (nv == NLL_NV_MAX) BD_NLL_LAUNCH(DT_BF16, NLL_NV_MAX); else BD_NLL_LAUNCH(DT_BF16, 0);
    } else {
        if (nv == 4) BD_NLL_LAUNCH(DT_F16, 4); else if (nv == NLL_NV_MAX) BD_NLL_LAUNCH(DT_F16, NLL_NV_MAX); else BD_NLL_LAUNCH(DT_F16, 0);
    }
#undef BD_NLL_LAUNCH
    return launch_status();
}

// (behind every kernel that existed before them: see the note above bd_srv_prefill_attention_cached)
// One body for the two entry points: n == NULL is bd_srv_token_logprobs (R rows), otherwise bd_srv_step_logprobs (T tenants, cap entries each).
static int token_logprobs_launch(const void* logits, int64_t sl, int V, const int64_t* tok, const int64_t* n, int64_t* lp_n, float* lp,
                                 int32_t* top_id, float* top_lp, int cap, int top_n, int R, int dtype, bool step, void* stream) {
    if (R < 0 || V < 1 || V > NLL_V_MAX || cap < 0) return BD_E_BAD_SHAPE;
    if (dtype != BD_F16 && dtype != BD_BF16) return BD_E_BAD_DTYPE;
    if (R == 0) return BD_OK;
    if (top_n < 0 || top_n > LP_TOP_MAX || top_n > V) return BD_E_BAD_SHAPE;
    if (!logits || !tok || !lp || (step && (!n || !lp_n)) || (top_n > 0 && (!top_id || !top_lp))) return BD_E_NULL;
    if (V % 8 || sl % 8 || sl < V || !aligned16(logits) || !aligned_to(tok, 8) || !aligned_to(n, 8) || !aligned_to(lp_n, 8) || !aligned_to(lp, 4) ||
        !aligned_to(top_id, 4) || !aligned_to(top_lp, 4))
        return BD_E_BAD_SHAPE;
    hipStream_t st = (hipStream_t)stream;
    // the form depends on V alone, as in bd_srv_token_nll: <= 8192 / <= 32768 hold the row in 4 / 16 sixteen-byte registers per thread
#define BD_LP_LAUNCH(DT, NV)                                                                                                                 \
    hipLaunchKernelGGL((token_logprobs_kernel<DT, NV>), dim3((unsigned)R), dim3(256), 0, st, (const unsigned short*)logits, (long long)sl, V, \
                       (const long long*)tok, (const long long*)n, (long long*)lp_n, lp, (int*)top_id, top_lp, cap, top_n)
    const int nv = V <= 2048 * 4 ? 4 : V <= 2048 * NLL_NV_MAX ? NLL_NV_MAX : 0;
    if (dtype == BD_BF16) {
        if (nv == 4) BD_LP_LAUNCH(DT_BF16, 4); else if (nv == NLL_NV_MAX) BD_LP_LAUNCH(DT_BF16, NLL_NV_MAX); else BD_LP_LAUNCH(DT_BF16, 0);
    } else {
        if (nv == 4) BD_LP_LAUNCH(DT_F16, 4); else if (nv == NLL_NV_MAX) BD_LP_LAUNCH(DT_F16, NLL_NV_MAX); else BD_LP_LAUNCH(DT_F16, 0);
    }
#undef BD_LP_LAUNCH
    return launch_status();
}

extern "C" int bd_srv_token_logprobs(const void* logits, int64_t sl, int V, const int64_t* tok, float* lp, int32_t* top_id, float* top_lp,
                                     int top_n, int R, int dtype, void* stream) {
    return token_logprobs_launch(logits, sl, V, tok, nullptr, nullptr, lp, top_id, top_lp, 0, top_n, R, dtype, false, stream);
}

extern "C" int bd_srv_step_logprobs(const void* logits, int64_t sl, int V, const int64_t* tok, const int64_t* n, int64_t* lp_n, float* lp,
                                    int32_t* top_id, float* top_lp, int cap, int top_n, int T, int dtype, void* stream) {
    return token_logprobs_launch(logits, sl, V, tok, n, lp_n, lp, top_id, top_lp, cap, top_n, T, dtype, true, stream);
}

// (behind every kernel that existed before them: see the note above bd_srv_prefill_attention_cached)
// One body for the two entry points: step == false is bd_srv_penalize_rows (R live rows, hist read only), true bd_srv_step_penalize (T tenants).
static int penalize_launch(const void* logits, int64_t sl, int V, void* out, int64_t so, const int16_t* hist, int64_t sh, const int64_t* tok,
                           const uint8_t* active, const float* pen, const int32_t* bias_id, const float* bias_val, int nb, int R, int dtype,
                           bool step, void* stream) {
    if (R < 0 || V < 1 || V > NLL_V_MAX) return BD_E_BAD_SHAPE;
    if (dtype != BD_F16 && dtype != BD_BF16) return BD_E_BAD_DTYPE;
    if (R == 0) return BD_OK;
    if (nb < 0 || nb > PEN_BIAS_MAX || R > 65535) return BD_E_BAD_SHAPE;
    if (!logits || !out || !hist || !pen || (step && (!tok || !active)) || (nb > 0 && (!bias_id || !bias_val))) return BD_E_NULL;
    if (V % 8 || sl % 8 || so % 8 || sh % 8 || sl < V || so < V || sh < V || !aligned16(logits) || !aligned16(out) || !aligned16(hist) ||
        !aligned16(pen) || !aligned_to(tok, 8) || !aligned_to(bias_id, 4) || !aligned_to(bias_val, 4))
        return BD_E_BAD_SHAPE;
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid((unsigned)((V + PEN_BLOCK_ELEMS - 1) / PEN_BLOCK_ELEMS), (unsigned)R);
#define BD_PEN_LAUNCH(DT, STEP)                                                                                                              \
    hipLaunchKernelGGL((penalize_kernel<DT, STEP>), grid, dim3(256), 0, st, (const unsigned short*)logits, (long long)sl, V,                 \
                       (unsigned short*)out, (long long)so, (unsigned short*)const_cast<int16_t*>(hist), (long long)sh, (const long long*)tok, \
                       (const unsigned char*)active, pen, (const int*)bias_id, bias_val, nb)
    if (dtype == BD_BF16) {
        if (step) BD_PEN_LAUNCH(DT_BF16, true); else BD_PEN_LAUNCH(DT_BF16, false);
    } else {
        if (step) BD_PEN_LAUNCH(DT_F16, true); else BD_PEN_LAUNCH(DT_F16, false);
    }
#undef BD_PEN_LAUNCH
    return launch_status();
}

extern "C" int bd_srv_penalize_rows(const void* logits, int64_t sl, int V, void* out, int64_t so, const int16_t* hist, int64_t sh,
                                    const float* pen, const int32_t* bias_id, const float* bias_val, int nb, int R, int dtype, void* stream) {
    return penalize_launch(logits, sl, V, out, so, hist, sh, nullptr, nullptr, pen, bias_id, bias_val, nb, R, dtype, false, stream);
}

extern "C" int bd_srv_step_penalize(const void* logits, int64_t sl, int V, void* out, int64_t so, int16_t* hist, int64_t sh, const int64_t* tok,
                                    const uint8_t* active, const float* pen, const int32_t* bias_id, const float* bias_val, int nb, int T,
                                    int dtype, void* stream) {
    return penalize_launch(logits, sl, V, out, so, hist, sh, tok, active, pen, bias_id, bias_val, nb, T, dtype, true, stream);
}

// (behind every kernel that existed before them: see the note above bd_srv_prefill_attention_cached)
// One body for the two mask entry points: step == false is bd_srv_constrain_rows (R live rows), true bd_srv_step_constrain (T tenants).
static int constrain_launch(const void* logits, int64_t sl, int V, void* out, int64_t so, const int32_t* state, const int32_t* off,
                            const int32_t* edge_tok, const uint8_t* accepting, int S, int E, const int64_t* stop_ids, int ns,
                            const uint8_t* active, int R, int dtype, bool step, void* stream) {
    if (R < 0 || V < 1 || V > NLL_V_MAX) return BD_E_BAD_SHAPE;
    if (dtype != BD_F16 && dtype != BD_BF16) return BD_E_BAD_DTYPE;
    if (R == 0) return BD_OK;
    if (S < 1 || S > CON_STATES_MAX || E < 0 || E > CON_EDGES_MAX || ns < 0 || ns > CON_STOP_MAX || R > 65535) return BD_E_BAD_SHAPE;
    if (!logits || !out || !state || !off || !accepting || (E > 0 && !edge_tok) || (ns > 0 && !stop_ids) || (step && !active)) return BD_E_NULL;
    if (V % 8 || sl % 8 || so % 8 || sl < V || so < V || !aligned16(logits) || !aligned16(out) || !aligned_to(state, 4) || !aligned_to(off, 4) ||
        !aligned_to(edge_tok, 4) || !aligned_to(stop_ids, 8))
        return BD_E_BAD_SHAPE;
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid((unsigned)((V + CON_BLOCK_ELEMS - 1) / CON_BLOCK_ELEMS), (unsigned)R);
#define BD_CON_LAUNCH(DT, STEP)                                                                                                           \
    hipLaunchKernelGGL((constrain_kernel<DT, STEP>), grid, dim3(256), 0, st, (const unsigned short*)logits, (long long)sl, V,              \
                       (unsigned short*)out, (long long)so, (const int*)state, (const int*)off, (const int*)edge_tok,                      \
                       (const unsigned char*)accepting, S, E, (const long long*)stop_ids, ns, (const unsigned char*)active)
    if (dtype == BD_BF16) {
        if (step) BD_CON_LAUNCH(DT_BF16, true); else BD_CON_LAUNCH(DT_BF16, false);
    } else {
        if (step) BD_CON_LAUNCH(DT_F16, true); else BD_CON_LAUNCH(DT_F16, false);
    }
#undef BD_CON_LAUNCH
    return launch_status();
}

extern "C" int bd_srv_constrain_rows(const void* logits, int64_t sl, int V, void* out, int64_t so, const int32_t* state, const int32_t* off,
                                     const int32_t* edge_tok, const uint8_t* accepting, int S, int E, const int64_t* stop_ids, int ns, int R,
                                     int dtype, void* stream) {
    return constrain_launch(logits, sl, V, out, so, state, off, edge_tok, accepting, S, E, stop_ids, ns, nullptr, R, dtype, false, stream);
}

extern "C" int bd_srv_step_constrain(const void* logits, int64_t sl, int V, void* out, int64_t so, const int32_t* state, const int32_t* off,
                                     const int32_t* edge_tok, const uint8_t* accepting, int S, int E, const int64_t* stop_ids, int ns,
                                     const uint8_t* active, int T, int dtype, void* stream) {
    return constrain_launch(logits, sl, V, out, so, state, off, edge_tok, accepting, S, E, stop_ids, ns, active, T, dtype, true, stream);
}

extern "C" int bd_srv_step_constrain_advance(const int64_t* tok, const int64_t* n, int64_t* c_n, int32_t* state, const int32_t* off,
                                             const int32_t* edge_tok, const int32_t* edge_next, const uint8_t* accepting, int S, int E,
                                             uint8_t* active, uint8_t* done, int T, void* stream) {
    if (T < 0) return BD_E_BAD_SHAPE;
    if (T == 0) return BD_OK;
    if (S < 1 || S > CON_STATES_MAX || E < 0 || E > CON_EDGES_MAX || T > CON_ADVANCE_T_MAX) return BD_E_BAD_SHAPE;
    if (!tok || !n || !c_n || !state || !off || !accepting || !active || !done || (E > 0 && (!edge_tok || !edge_next))) return BD_E_NULL;
    if (!aligned_to(tok, 8) || !aligned_to(n, 8) || !aligned_to(c_n, 8) || !aligned_to(state, 4) || !aligned_to(off, 4) ||
        !aligned_to(edge_tok, 4) || !aligned_to(edge_next, 4))
        return BD_E_BAD_SHAPE;
    hipLaunchKernelGGL((constrain_advance_kernel<CON_ADVANCE_T_MAX>), dim3(1), dim3((unsigned)((T + 63) / 64 * 64)), 0, (hipStream_t)stream, (const long long*)tok,
                       (const long long*)n, (long long*)c_n, (int*)state, (const int*)off, (const int*)edge_tok, (const int*)edge_next,
                       (const unsigned char*)accepting, S, E, (unsigned char*)active, (unsigned char*)done, T);
    return launch_status();
}

// (behind every kernel that existed before it: see the note above bd_srv_prefill_attention_cached)
extern "C" int bd_srv_step_stop_sequences(const int64_t* out, int64_t s_out, int out_cap, const int64_t* n, int64_t* ss_n, const int32_t* seq_tok,
                                          const int32_t* seq_len, int Q, int W, int32_t* hit, int32_t* hold, uint8_t* active, uint8_t* done, int T,
                                          void* stream) {
    if (T < 0 || T > SS_T_MAX || Q < 1 || Q > SS_Q_MAX || W < 1 || W > SS_W_MAX || out_cap < 0 || s_out < out_cap) return BD_E_BAD_SHAPE;
    if (T == 0) return BD_OK;
    if (!out || !n || !ss_n || !seq_tok || !seq_len || !hit || !hold || !active || !done) return BD_E_NULL;
    if (!aligned_to(out, 8) || !aligned_to(n, 8) || !aligned_to(ss_n, 8) || !aligned_to(seq_tok, 4) || !aligned_to(seq_len, 4) ||
        !aligned_to(hit, 4) || !aligned_to(hold, 4))
        return BD_E_BAD_SHAPE;
    // one thread per (sequence, length) pair at a pitch of SS_W_MAX lengths per sequence, whole waves
    hipLaunchKernelGGL((stop_sequences_kernel<SS_Q_MAX, SS_W_MAX>), dim3((unsigned)T), dim3((unsigned)((Q * SS_W_MAX + 63) / 64 * 64)), 0,
                       (hipStream_t)stream, (const long long*)out, (long long)s_out, out_cap, (const long long*)n, (long long*)ss_n,
                       (const int*)seq_tok, (const int*)seq_len, Q, W, (int*)hit, (int*)hold, (unsigned char*)active, (unsigned char*)done);
    return launch_status();
}

// (behind every kernel that existed before them: see the note above bd_srv_prefill_attention_cached)
// One body for the two ban entry points: step == false is bd_srv_ban_rows (R live rows; n may be NULL: no turn tokens yet), true bd_srv_step_ban
// (T tenants).
static int ban_launch(const void* logits, int64_t sl, int V, void* out, int64_t so, const int32_t* ctx, int Lc, const int32_t* ctx_len,
                      const int64_t* toks, int64_t s_tok, int tok_cap, const int64_t* n, const int32_t* ban_ngram, const int32_t* ban_tok,
                      const int32_t* ban_len, int Q, int W, const int32_t* ban_min, const int64_t* stop_ids, int ns, const uint8_t* active, int R,
                      int dtype, bool step, void* stream) {
    if (R < 0 || V < 1 || V > NLL_V_MAX) return BD_E_BAD_SHAPE;
    if (dtype != BD_F16 && dtype != BD_BF16) return BD_E_BAD_DTYPE;
    if (R == 0) return BD_OK;
    if (Q < 1 || Q > BAN_WORDS_MAX || W < 1 || W > BAN_WORD_LEN_MAX || ns < 0 || ns > BAN_STOP_MAX || Lc < 0 || tok_cap < 0 ||
        s_tok < (int64_t)tok_cap || (int64_t)Lc + (int64_t)tok_cap > 0x7fffffffll || R > 65535)
        return BD_E_BAD_SHAPE;
    if (!logits || !out || !ctx_len || !ban_ngram || !ban_tok || !ban_len || !ban_min || (Lc > 0 && !ctx) || (ns > 0 && !stop_ids) ||
        (step && (!active || !n)) || (n && tok_cap > 0 && !toks))
        return BD_E_NULL;
    if (V % 8 || sl % 8 || so % 8 || sl < V || so < V || !aligned16(logits) || !aligned16(out) || !aligned_to(ctx, 4) || !aligned_to(ctx_len, 4) ||
        !aligned_to(toks, 8) || !aligned_to(n, 8) || !aligned_to(ban_ngram, 4) || !aligned_to(ban_tok, 4) || !aligned_to(ban_len, 4) ||
        !aligned_to(ban_min, 4) || !aligned_to(stop_ids, 8))
        return BD_E_BAD_SHAPE;
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid((unsigned)((V + BAN_BLOCK_ELEMS - 1) / BAN_BLOCK_ELEMS), (unsigned)R);
#define BD_BAN_LAUNCH(DT, STEP)                                                                                                          \
    hipLaunchKernelGGL((ban_kernel<DT, STEP>), grid, dim3(256), 0, st, (const unsigned short*)logits, (long long)sl, V,                   \
                       (unsigned short*)out, (long long)so, (const int*)ctx, Lc, (const int*)ctx_len, (const long long*)toks,             \
                       (long long)s_tok, tok_cap, (const long long*)n, (const int*)ban_ngram, (const int*)ban_tok, (const int*)ban_len,   \
                       Q, W, (const int*)ban_min, (const long long*)stop_ids, ns, (const unsigned char*)active)
    if (dtype == BD_BF16) {
        if (step) BD_BAN_LAUNCH(DT_BF16, true); else BD_BAN_LAUNCH(DT_BF16, false);
    } else {
        if (step) BD_BAN_LAUNCH(DT_F16, true); else BD_BAN_LAUNCH(DT_F16, false);
    }
#undef BD_BAN_LAUNCH
    return launch_status();
}

extern "C" int bd_srv_ban_rows(const void* logits, int64_t sl, int V, void* out, int64_t so, const int32_t* ctx, int Lc, const int32_t* ctx_len,
                               const int64_t* toks, int64_t s_tok, int tok_cap, const int64_t* n, const int32_t* ban_ngram,
                               const int32_t* ban_tok, const int32_t* ban_len, int Q, int W, const int32_t* ban_min, const int64_t* stop_ids,
                               int ns, int R, int dtype, void* stream) {
    return ban_launch(logits, sl, V, out, so, ctx, Lc, ctx_len, toks, s_tok, tok_cap, n, ban_ngram, ban_tok, ban_len, Q, W, ban_min, stop_ids, ns,
                      nullptr, R, dtype, false, stream);
}

extern "C" int bd_srv_step_ban(const void* logits, int64_t sl, int V, void* out, int64_t so, const int32_t* ctx, int Lc, const int32_t* ctx_len,
                               const int64_t* toks, int64_t s_tok, int tok_cap, const int64_t* n, const int32_t* ban_ngram,
                               const int32_t* ban_tok, const int32_t* ban_len, int Q, int W, const int32_t* ban_min, const int64_t* stop_ids,
                               int ns, const uint8_t* active, int T, int dtype, void* stream) {
    return ban_launch(logits, sl, V, out, so, ctx, Lc, ctx_len, toks, s_tok, tok_cap, n, ban_ngram, ban_tok, ban_len, Q, W, ban_min, stop_ids, ns,
                      active, T, dtype, true, stream);
}

// (behind every kernel that existed before them: see the note above bd_srv_prefill_attention_cached)
// One body for the two truncation entry points: step == false is bd_srv_truncate_rows (R live rows), true bd_srv_step_truncate (T tenants).
static int truncate_launch(const void* logits, int64_t sl, int V, void* out, int64_t so, const float* tau, const float* params,
                           const uint8_t* active, int R, int dtype, bool step, void* stream) {
    if (R < 0 || V < 1 || V > NLL_V_MAX) return BD_E_BAD_SHAPE;
    if (dtype != BD_F16 && dtype != BD_BF16) return BD_E_BAD_DTYPE;
    if (R == 0) return BD_OK;
    if (!logits || !out || !tau || !params || (step && !active)) return BD_E_NULL;
    if (V % 8 || sl % 8 || so % 8 || sl < V || so < V || !aligned16(logits) || !aligned16(out) || !aligned_to(tau, 4) || !aligned_to(params, 4))
        return BD_E_BAD_SHAPE;
    hipStream_t st = (hipStream_t)stream;
    // the form depends on V alone, as in bd_srv_token_nll: <= 8192 / <= 32768 hold the row in 4 / 16 sixteen-byte registers per thread
#define BD_TRUNC_LAUNCH(DT, NV)                                                                                                            \
    hipLaunchKernelGGL((truncate_kernel<DT, NV>), dim3((unsigned)R), dim3(256), 0, st, (const unsigned short*)logits, (long long)sl, V,    \
                       (unsigned short*)out, (long long)so, tau, params, (const unsigned char*)(step ? active : nullptr))
    const int nv = V <= 2048 * 4 ? 4 : V <= 2048 * NLL_NV_MAX ? NLL_NV_MAX : 0;
    if (dtype == BD_BF16) {
        if (nv == 4) BD_TRUNC_LAUNCH(DT_BF16, 4); else if (nv == NLL_NV_MAX) BD_TRUNC_LAUNCH(DT_BF16, NLL_NV_MAX); else BD_TRUNC_LAUNCH(DT_BF16, 0);
    } else {
        if (nv == 4) BD_TRUNC_LAUNCH(DT_F16, 4); else if (nv == NLL_NV_MAX) BD_TRUNC_LAUNCH(DT_F16, NLL_NV_MAX); else BD_TRUNC_LAUNCH(DT_F16, 0);
    }
#undef BD_TRUNC_LAUNCH
    return launch_status();
}

extern "C" int bd_srv_truncate_rows(const void* logits, int64_t sl, int V, void* out, int64_t so, const float* tau, const float* params, int R,
                                    int dtype, void* stream) {
    return truncate_launch(logits, sl, V, out, so, tau, params, nullptr, R, dtype, false, stream);
}

extern "C" int bd_srv_step_truncate(const void* logits, int64_t sl, int V, void* out, int64_t so, const float* tau, const float* params,
                                    const uint8_t* active, int T, int dtype, void* stream) {
    return truncate_launch(logits, sl, V, out, so, tau, params, active, T, dtype, true, stream);
}
