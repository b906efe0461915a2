"""Exact tests of the RMSNorm, SwiGLU and RoPE glue kernels of csrc/bd_serving.h: every output element against the fp64 models of
tests/glue_ref.py (the kernels' documented rounding points, everything else exact) under that module's ONE acceptance rule -- a per-element ulp
limit AND a minimum share of bit-equal elements (tests/test_glue_ref_host.py shows, without a GPU, that the rule passes an fp32 emulation of the
kernels and fails one that drops eps, skips or moves a rounding point, or divides by the wrong H).

The C entry points are called directly (bitdelta_amd._lib), outputs sit inside canary.CanaryOut with a row stride above the row length, inputs
have a row stride of H + 64 with poisoned padding, and every launch is followed by untouched_outside().  Shapes are the smallest that reach each
code path (glue_ref.NORM_BLOCK_H / NORM_WAVE_H and the tables below); the models run on the CPU in float64 from the exact 16-bit inputs.

Limits (glue_ref.*_LIMITS): norm family 2 ulps / 0.99 bit-equal, SwiGLU 2 / 0.99, RoPE 1 / 0.999.  Every check prints `GLUE <case>: worst ulp,
bit-equal share` before it asserts (pytest -s shows the figures).

Measured on an MI355X, worst ulp distance / lowest bit-equal share over a kernel's cases, fp16 | bf16:
    rmsnorm block-per-row 1 / 0.999837 | 0 / 1      rmsnorm wave-per-row 2 / 0.999931 | 0 / 1      add_rmsnorm x 0 / 1 | 0 / 1, h 2 / 0.999837 | 0 / 1
    split-k reduce + norm 2 / 0.999912 | 0 / 1      SwiGLU (each of the three layouts alike) 2 / 0.999951 | 0 / 1      rope_, rope_kv_append 0 / 1 | 0 / 1
    (SwiGLU fp16: 100 ulps at elements whose round16(silu(g)) is subnormal and sits one quantum off, times u = 100 -- inside the derived band;
    2 where that intermediate is a normal number.)  Rotation check: spread 1.6e-2 of 2.7e-1 allowed (fp16), 1.2e-1 of 2.2 (bf16).
    The fp32 CPU emulation of tests/test_glue_ref_host.py gives the same picture (bf16 all equal, fp16 ~10 elements of 540 000 off).
Wall time of the module: 4 s for its 62 cases."""
import ctypes

import numpy as np
import pytest
import torch

import glue_ref as ref
from canary import POISON, CanaryOut

pytestmark = pytest.mark.gpu

DEV = "cuda"
DTYPES = [torch.float16, torch.bfloat16]
DT_ID = {torch.float16: "f16", torch.bfloat16: "bf16"}
PAD = 64


@pytest.fixture(scope="module")
def L():
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    from bitdelta_amd import _lib
    return _lib.lib()


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr())


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _code(dtype):
    from bitdelta_amd._lib import DTYPE_CODE
    return DTYPE_CODE[dtype]


def padded(t, pad=PAD):
    """t [rows, n] (CPU) on the device as a view with row stride n + pad; the padding carries the canary's poison, so a stray read shows"""
    buf = torch.empty(t.shape[0], t.shape[1] + pad, dtype=t.dtype, device=DEV)
    buf.view(torch.uint8).fill_(POISON)
    view = buf[:, :t.shape[1]]
    view.copy_(t)
    return view


def out_canary(rows, n, dtype):
    """a [rows, n] output inside a poisoned buffer: 8 rows above and below, 64 columns left and right (row stride n + 128), a whole entry each side"""
    return CanaryOut(1, rows, n, dtype, row_margin=8, col_margin=PAD)


def check(case, got16, model, inter, mult, dtype, limits):
    """the one acceptance rule; prints the figures, and on failure names the case, the worst ulp distance, the bit-equal share and the first
    offending index"""
    got16 = got16.detach().cpu()
    v = ref.accept(got16, model, inter, mult, dtype, *limits)
    print(f"GLUE {case} {DT_ID[dtype]}: worst ulp {v.worst_ulp} ({v.worst_ulp_normal} where the intermediate is normal), "
          f"bit-equal share {v.equal_share:.6f}")
    where = tuple(int(i) for i in np.unravel_index(v.first_bad, got16.shape)) if v.first_bad >= 0 else None
    detail = ""
    if where is not None:
        detail = f"; got {float(got16[where])!r}, model {float(np.broadcast_to(model, got16.shape)[where])!r}"
    assert v.ok, (f"{case} {DT_ID[dtype]}: worst ulp distance {v.worst_ulp} (limit {limits[0]}; {v.worst_ulp_normal} where the intermediate is "
                  f"normal), bit-equal share {v.equal_share:.6f} (at least {limits[1]}), {v.n_bad} elements outside the rule, "
                  f"first offending index {where}{detail}")
    return v


def bit_equal(a, b):
    return torch.equal(a.contiguous().view(torch.int16), b.contiguous().view(torch.int16))


# ------------------------------------------------------------------------------------------------------------------------ RMSNorm
def launch_norm(L, x, w, y, rows, H, rows_per_tenant, eps, dtype):
    rc = L.bd_srv_rmsnorm(_ptr(x), _ptr(w), _ptr(y), rows, H, x.stride(0), y.stride(0), w.stride(0), rows_per_tenant, float(eps), _code(dtype),
                          _stream())
    assert rc == 0, rc


def check_special_rows(case, got, classes):
    """what the row classes promise, spelled out (the model says the same): a zero row gives exact zeros and never NaN, a NaN takes its whole row,
    an inf leaves one NaN and signed zeros, and every other row -- the neighbours of those two included -- is finite"""
    got = ref.to64(got)
    for r, c in enumerate(classes):
        if c == ref.ZERO_ROW:
            assert not got[r].any() and not np.isnan(got[r]).any(), (case, r, "zero row")
        elif c == ref.NAN_ROW:
            assert np.isnan(got[r]).all(), (case, r, "NaN row")
        elif c == ref.INF_ROW:
            assert np.isnan(got[r]).sum() == 1 and not np.nan_to_num(got[r]).any(), (case, r, "inf row")
        else:
            assert np.isfinite(got[r]).all(), (case, r, "ordinary row")
    if "e" in classes:                                                      # fp16 subnormal inputs were not flushed: the row is not zero
        assert all(got[r].any() for r, c in enumerate(classes) if c == "e"), (case, "subnormal row flushed")


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_ID.get)
@pytest.mark.parametrize("H", ref.NORM_BLOCK_H)
def test_rmsnorm_block_per_row_kernel(L, dtype, H):
    rows, rpt = ref.NORM_BLOCK_ROWS, ref.NORM_BLOCK_ROWS // ref.NORM_TENANTS
    x, w, classes = ref.norm_inputs(dtype, H, rows)
    xd, wd = padded(x), padded(w)
    x64, w64 = ref.to64(x), ref.to64(w)
    wr = w64[np.arange(rows) // rpt]
    for eps in ref.NORM_EPS:
        out = out_canary(rows, H, dtype)
        launch_norm(L, xd, wd, out.view[0], rows, H, rpt, eps, dtype)
        torch.cuda.synchronize()
        got = out.result()[0]
        assert out.untouched_outside(), f"rmsnorm block H={H} eps={eps}: stored outside its output"
        want, a = ref.rmsnorm(x64, w64, eps, rpt, dtype)
        check(f"rmsnorm block-per-row H={H} eps={eps}", got, want, a, wr, dtype, ref.NORM_LIMITS)
        check_special_rows((H, eps), got, classes)


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_ID.get)
@pytest.mark.parametrize("H", ref.NORM_WAVE_H)
def test_rmsnorm_wave_per_row_kernel_and_its_identity_with_the_block_kernel(L, dtype, H):
    rows, rpt = ref.NORM_WAVE_ROWS, ref.NORM_WAVE_ROWS // ref.NORM_TENANTS
    assert rows >= 64 and rows % 4 and rpt % 4                              # the wave kernel; idle waves in the last block; a block straddles tenants
    x, w, classes = ref.norm_inputs(dtype, H, rows)
    xd, wd = padded(x), padded(w)
    x64, w64 = ref.to64(x), ref.to64(w)
    wr = w64[np.arange(rows) // rpt]
    for eps in ref.NORM_EPS:
        out = out_canary(rows, H, dtype)
        launch_norm(L, xd, wd, out.view[0], rows, H, rpt, eps, dtype)       # 66 rows: one wave per row
        torch.cuda.synchronize()
        got = out.result()[0]
        assert out.untouched_outside(), f"rmsnorm wave H={H} eps={eps}: stored outside its output"
        want, a = ref.rmsnorm(x64, w64, eps, rpt, dtype)
        check(f"rmsnorm wave-per-row H={H} eps={eps}", got, want, a, wr, dtype, ref.NORM_LIMITS)
        check_special_rows((H, eps), got, classes)
        # the same rows as 63 + 3: both launches are under the 64-row switch and take the block-per-row kernel (the last 3 rows are tenant 2's)
        two = out_canary(rows, H, dtype)
        launch_norm(L, xd, wd, two.view[0], 63, H, rpt, eps, dtype)
        launch_norm(L, xd[63:], wd[2:], two.view[0][63:], 3, H, rpt, eps, dtype)
        torch.cuda.synchronize()
        assert two.untouched_outside()
        assert bit_equal(two.result()[0], got), f"rmsnorm H={H} eps={eps}: the wave-per-row and block-per-row kernels differ"


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_ID.get)
@pytest.mark.parametrize("H", [8, 264, 2056, 8192])
def test_add_rmsnorm_kernel(L, dtype, H):
    rows, rpt = ref.NORM_BLOCK_ROWS, ref.NORM_BLOCK_ROWS // ref.NORM_TENANTS
    resid, w, classes = ref.norm_inputs(dtype, H, rows)
    y32 = ref.add_norm_y32(resid, classes)
    rd, yd, wd = padded(resid), padded(y32), padded(w)
    w64 = ref.to64(w)
    wr = w64[np.arange(rows) // rpt]
    for eps in ref.NORM_EPS:
        xo, ho = out_canary(rows, H, dtype), out_canary(rows, H, dtype)
        rc = L.bd_srv_add_rmsnorm(_ptr(rd), _ptr(yd), _ptr(wd), _ptr(xo.view[0]), _ptr(ho.view[0]), rows, H, rd.stride(0), yd.stride(0),
                                  xo.view.stride(1), ho.view.stride(1), wd.stride(0), rpt, float(eps), _code(dtype), _stream())
        assert rc == 0, rc
        torch.cuda.synchronize()
        x_got, h_got = xo.result()[0], ho.result()[0]
        assert xo.untouched_outside() and ho.untouched_outside(), f"add_rmsnorm H={H} eps={eps}: stored outside its outputs"
        x_want, _, _ = ref.add_rmsnorm(ref.to64(resid), ref.to64(y32), w64, eps, rpt, dtype)
        check(f"add_rmsnorm x H={H} eps={eps}", x_got, x_want, ref.round16(ref.to64(y32), dtype), np.ones(1), dtype, ref.NORM_LIMITS)
        # h against the norm of the x the launch itself stored: an element of x that legitimately sits one ulp off moves its whole row of h
        h_want, a = ref.rmsnorm(ref.to64(x_got), w64, eps, rpt, dtype)
        check(f"add_rmsnorm h H={H} eps={eps}", h_got, h_want, a, wr, dtype, ref.NORM_LIMITS)
        # (the zero and subnormal rows of the residual are ordinary rows of x = residual + y32; the NaN and inf rows keep their promises)
        check_special_rows((H, eps), h_got, ["a" if c in (ref.ZERO_ROW, "e") else c for c in classes])


# (T, M, N, K) of test_gpu_serving.test_residual_linear_with_following_norm_is_bit_identical_to_the_two_launches, smallest first
RESIDUAL_NORM_SHAPES = sorted([(6, 64, 4096, 4096), (6, 64, 4096, 14336), (5, 40, 4096, 4096), (2, 64, 2048, 2048), (6, 17, 1024, 512),
                               (3, 128, 4096, 4096), (6, 64, 8192, 1024), (1, 64, 4096, 4096)], key=lambda s: s[0] * s[1] * s[2] * s[3])


def residual_norm_call(L, x, w, mask, alpha, resid, nw, eps, h, ws, ws_bytes, dtype):
    T, M, K = x.shape
    N = w.shape[0]
    return L.bd_binary_linear_residual_norm(_ptr(x), _ptr(w), _ptr(mask), _ptr(alpha), _ptr(resid), T, M, N, K, x.stride(0), x.stride(1), w.stride(0),
                                            mask.stride(0), 1, 1, resid.stride(0), resid.stride(1), _code(dtype), _ptr(nw), nw.stride(0),
                                            float(eps), _ptr(h), h.stride(0), h.stride(1), _ptr(ws), ws_bytes, _stream())


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_ID.get)
def test_splitk_reduce_norm_launch(L, dtype):
    """bd_binary_linear_residual_norm where the split-k reduce launch carries the norm (bd_last_gemm_plan field [6]): h against the model's norm
    of the x the call itself stored (the Linear is pinned elsewhere), with eps = 1e-2, as the identity test draws its inputs and with residual and
    activations scaled by 2^-10 so that eps dominates.  The shape is the smallest of the identity test's whose plan splits."""
    from bitdelta_amd import _lib
    rec = (ctypes.c_int32 * _lib.BD_GEMM_PLAN_INTS)()
    eps = 1e-2
    done = False
    for T, M, N, K in RESIDUAL_NORM_SHAPES:
        g = torch.Generator(device=DEV).manual_seed(T * 1000 + M + N + K)
        x = torch.randn(T, M, K, device=DEV, generator=g).to(dtype)
        w = (torch.randn(N, K, device=DEV, generator=g) * 0.02).to(dtype)
        mask = torch.randint(-2 ** 31, 2 ** 31 - 1, (T, K // 32, N), device=DEV, generator=g, dtype=torch.int64).to(torch.int32)
        alpha = (torch.rand(T, 1, device=DEV, generator=g) * 1e-3 + 2e-4)
        resid = torch.randn(T, M, N, device=DEV, generator=g).to(dtype)
        nw = (1 + 0.1 * torch.randn(T, N, device=DEV, generator=g)).to(dtype)
        ws, ws_bytes = _lib.workspace(L.bd_gemm_workspace_bytes(T, M, N, K), torch.device(DEV), zeroed=True)
        ws = ws if ws is not None else torch.zeros(16, dtype=torch.uint8, device=DEV)
        ho = CanaryOut(T, M, N, dtype, row_margin=0, col_margin=PAD)                       # (the norm wants a dense [T, M] row grid)
        L.bd_set_gemm_dry_run(1)
        try:
            rc = residual_norm_call(L, x, w, mask, alpha, resid, nw, eps, ho.view, ws, ws_bytes, dtype)
        finally:
            L.bd_set_gemm_dry_run(0)
        assert rc == 0 and L.bd_last_gemm_plan(rec, len(rec)) == _lib.BD_GEMM_PLAN_INTS
        if rec[6] != 1:
            continue                                                                       # not split: the norm would be bd_srv_rmsnorm's launch
        for scale, name in ((1.0, "as drawn"), (2.0 ** -10, "scaled 2^-10")):
            xs, r = (x.float() * scale).to(dtype), (resid.float() * scale).to(dtype)
            rc = residual_norm_call(L, xs, w, mask, alpha, r, nw, eps, ho.view, ws, ws_bytes, dtype)
            assert rc == 0 and L.bd_last_gemm_plan(rec, len(rec)) == _lib.BD_GEMM_PLAN_INTS
            assert rec[6] == 1 and rec[2] > 1, list(rec)[:7]
            torch.cuda.synchronize()
            h_got = ho.result().reshape(T * M, N)
            assert ho.untouched_outside(), f"residual_norm {name}: stored outside h"
            assert bool(torch.isfinite(r.float()).all()) and not bit_equal(r, (resid.float() * scale).to(dtype))     # x = residual + Linear was stored
            h_want, a = ref.rmsnorm(ref.to64(r).reshape(T * M, N), ref.to64(nw), eps, M, dtype)
            check(f"splitk_reduce_norm ({T}, {M}, {N}, {K}) {name}", h_got, h_want, a, ref.to64(nw)[np.arange(T * M) // M], dtype, ref.NORM_LIMITS)
        done = True
        break
    assert done, "no shape of the identity test puts the norm on the reduce launch"


# ------------------------------------------------------------------------------------------------------------------------ SwiGLU
SWIGLU_LAYOUTS = ("swiglu2", "swiglu", "swiglu_interleaved8")


def launch_swiglu(L, layout, g, u, dtype):
    """g, u [rows, I] CPU tensors -> (result [rows, I], canary) through one of the three layouts of bd_srv_swiglu"""
    rows, I = g.shape
    out = out_canary(rows, I, dtype)
    y = out.view[0]
    if layout == "swiglu2":                                                 # two separate strided views
        gd, ud = padded(g), padded(u, 2 * PAD)
        rc = L.bd_srv_swiglu(_ptr(gd), _ptr(ud), _ptr(y), rows, I, gd.stride(0), ud.stride(0), y.stride(0), 0, _code(dtype), _stream())
    elif layout == "swiglu":                                                # gate | up halves of one projection output
        gu = padded(torch.cat([g, u], 1))
        rc = L.bd_srv_swiglu(_ptr(gu), _ptr(gu[:, I:]), _ptr(y), rows, I, gu.stride(0), gu.stride(0), y.stride(0), 0, _code(dtype), _stream())
    else:                                                                   # [g0..7 | u0..7 | g8..15 | u8..15 | ...]
        gu = padded(torch.stack([g.reshape(rows, I // 8, 8), u.reshape(rows, I // 8, 8)], 2).reshape(rows, 2 * I))
        rc = L.bd_srv_swiglu(_ptr(gu), _ptr(gu), _ptr(y), rows, I, gu.stride(0), gu.stride(0), y.stride(0), 1, _code(dtype), _stream())
    assert rc == 0, rc
    torch.cuda.synchronize()
    return out.result()[0], out


@pytest.fixture(scope="module")
def swiglu_exhaustive():
    made = {}

    def get(dtype):
        if dtype not in made:
            g, u = ref.swiglu_exhaustive_inputs(dtype)
            made[dtype] = (g, u) + ref.swiglu(ref.to64(g), ref.to64(u), dtype)
        return made[dtype]
    return get


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_ID.get)
@pytest.mark.parametrize("layout", SWIGLU_LAYOUTS)
def test_swiglu_every_gate_up_to_80(L, swiglu_exhaustive, dtype, layout):
    g, u, want, a = swiglu_exhaustive(dtype)
    got, out = launch_swiglu(L, layout, g, u, dtype)
    assert out.untouched_outside(), f"{layout}: stored outside its output"
    check(f"{layout} exhaustive |g| <= 80", got, want, a, ref.to64(u), dtype, ref.SWIGLU_LIMITS)


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_ID.get)
@pytest.mark.parametrize("layout", SWIGLU_LAYOUTS)
def test_swiglu_grid_edges(L, dtype, layout):
    for I in (8, 264, 2048, 2056):                                          # one thread; 33 threads; one full block; one thread in a second block
        gen = torch.Generator().manual_seed(I)
        g = (torch.rand(3, I, generator=gen) * 40 - 20).to(dtype)
        u = (torch.randn(3, I, generator=gen) * 3).to(dtype)
        got, out = launch_swiglu(L, layout, g, u, dtype)
        assert out.untouched_outside(), f"{layout} I={I}: stored outside its output"
        want, a = ref.swiglu(ref.to64(g), ref.to64(u), dtype)
        check(f"{layout} I={I}", got, want, a, ref.to64(u), dtype, ref.SWIGLU_LIMITS)


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_ID.get)
@pytest.mark.parametrize("layout", SWIGLU_LAYOUTS)
def test_swiglu_extreme_gates(L, dtype, layout):
    """Gates where exp(-g) leaves fp32 (below about -88.7 the kernel returns -0 where the exact value is about -1e-37, as torch does), the largest
    finite values and the smallest subnormals: not ulp-compared.  The output is 0 or carries the sign of g u, lies within one ulp of the model
    (+ 1e-30 for the flushed tail), and is finite wherever the model is; where g u itself exceeds the format (65504 x -3 in fp16, the largest
    bf16 x -3) the model says inf, and so must the kernel.
    The smallest subnormal q itself meets u = 1 only; the u = -3 row has 2 q in its place.  silu(q) = q / (2 - q + ...) lies 2^-26 (relative)
    ABOVE q / 2, the midpoint of 0 and q, so the model rounds it up to q; in fp32 1 + exp(-q) is 2 exactly (as in torch's fp32 silu), q / 2 is
    the exact tie and goes to the even side, 0.  That is the intermediate one quantum away -- accept()'s derived band, which this case does not
    use -- and times |u| = 3 it is three ulps of the model's -3 q."""
    mbits, emin, emax = ref._FORMAT[dtype]
    mags = [88.0, 89.0, 100.0, 1e3, 1e4, 65504.0, 2.0 ** (emin - mbits), 3 * 2.0 ** (emin - mbits)]
    if dtype == torch.bfloat16:
        mags.append(float(torch.finfo(dtype).max))
    gates = ref.round16(np.array(mags + [-m for m in mags]), dtype)
    gates = np.concatenate([gates, np.zeros((-len(gates)) % 8)])
    q = 2.0 ** (emin - mbits)
    g = ref.from_bits(ref.bits16(np.stack([gates, np.where(np.abs(gates) == q, 2 * gates, gates)]), dtype), dtype)
    u = torch.tensor([[1.0], [-3.0]]).expand(2, g.shape[1]).to(dtype).contiguous()
    got16, out = launch_swiglu(L, layout, g, u, dtype)
    assert out.untouched_outside()
    got, g64, u64 = ref.to64(got16), ref.to64(g), ref.to64(u)
    want, _ = ref.swiglu(g64, u64, dtype)
    fin = np.isfinite(want)
    assert not np.isnan(want).any() and (np.abs(g64[~fin]) >= 65504).all()
    case = f"{layout} extremes {DT_ID[dtype]}"
    assert np.isfinite(got[fin]).all(), (case, g64[fin][~np.isfinite(got[fin])])
    assert np.array_equal(got[~fin], want[~fin]), (case, got[~fin], want[~fin])
    assert ((got == 0) | (np.sign(got) == np.sign(g64 * u64))).all(), (case, g64[(got != 0) & (np.sign(got) != np.sign(g64 * u64))])
    err, lim = np.abs(got[fin] - want[fin]), ref.ulp16(want[fin], dtype) + 1e-30
    print(f"GLUE {case}: largest |got - model| / (ulp + 1e-30) = {(err / lim).max():.3f}")
    assert (err <= lim).all(), (case, g64[fin][err > lim], got[fin][err > lim], want[fin][err > lim])


# ------------------------------------------------------------------------------------------------------------------------ RoPE
@pytest.fixture(scope="module")
def tables():
    from bitdelta_amd.serving_loop import _rope_tables
    made = {}

    def get(dtype):
        if dtype not in made:
            cos, sin = _rope_tables(256, 128, DEV, dtype)
            made[dtype] = (cos.contiguous(), sin.contiguous(), ref.to64(cos), ref.to64(sin))
        return made[dtype]
    return get


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_ID.get)
def test_rope_tables_against_first_principles(tables, dtype):
    _, _, cos16, sin16 = tables(dtype)
    cos, sin, ang = ref.rope_tables(256)
    pos = np.arange(256)[:, None]
    for name, table, model in (("cos", cos16, cos), ("sin", sin16, sin)):
        # the tables form the angle as a float32 product, as HF does: at most 3 * 2^-24 * angle <= pos * 2^-22 off
        excess = np.abs(table - model) - (0.5 * ref.ulp16(model, dtype) + pos * 2.0 ** -22)
        assert (excess <= 0).all(), (name, np.unravel_index(excess.argmax(), excess.shape), excess.max())
    clear = np.abs(np.sin(ang)) > 2.0 ** -6
    positive = clear & (np.sin(ang) > 0)
    assert positive[:, :64].sum() > 1000
    assert (sin16[:, :64][positive[:, :64]] < 0).all() and (sin16[:, 64:][positive[:, 64:]] > 0).all()      # sin[p, :64] <= 0 <= sin[p, 64:]
    negative = clear & (np.sin(ang) < 0)
    assert (sin16[:, :64][negative[:, :64]] > 0).all() and (sin16[:, 64:][negative[:, 64:]] < 0).all()


def launch_rope(L, buf, rows_at, rows, heads, seq, pos0, cos, sin, dtype):
    x = buf[rows_at:rows_at + rows, :heads * 128]
    rc = L.bd_srv_rope(_ptr(x), _ptr(cos), _ptr(sin), rows, heads, 128, buf.stride(0), seq, pos0, _code(dtype), _stream())
    assert rc == 0, rc
    torch.cuda.synchronize()


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_ID.get)
@pytest.mark.parametrize("pos0", [0, 3, 219])
def test_rope_in_place(L, tables, dtype, pos0):
    cos, sin, cos16, sin16 = tables(dtype)
    B, S, heads, guard = 2, 37, 5, 8                                        # 219 + 37 = 256: the last table row
    W = heads * 128
    gen = torch.Generator().manual_seed(pos0 + 1)
    full = torch.randn(B * S + 2 * guard, W + PAD, generator=gen).to(dtype)
    buf = full.to(DEV)
    launch_rope(L, buf, guard, B * S, heads, S, pos0, cos, sin, dtype)
    after = buf.cpu()
    keep = torch.ones_like(full, dtype=torch.bool)
    keep[guard:guard + B * S, :W] = False
    assert torch.equal(after.view(torch.int16)[keep], full.view(torch.int16)[keep]), "rope_: bytes between or around the rows changed"
    x64 = ref.to64(full[guard:guard + B * S, :W]).reshape(B * S, heads, 128)
    want, inter = ref.rope(x64, cos16, sin16, pos0 + np.arange(B * S) % S, dtype)
    check(f"rope_ pos0={pos0}", after[guard:guard + B * S, :W].reshape(B * S, heads, 128), want, inter, np.ones(1), dtype, ref.ROPE_LIMITS)


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_ID.get)
@pytest.mark.parametrize("T,S,H,KVH,Lc,pos0", [(3, 17, 8, 2, 64, 5), (1, 64, 4, 4, 96, 32)])
def test_rope_kv_append(L, tables, dtype, T, S, H, KVH, Lc, pos0):
    cos, sin, cos16, sin16 = tables(dtype)
    W, guard, margin = (H + 2 * KVH) * 128, 8, 4096
    gen = torch.Generator().manual_seed(T + S + H)
    full = torch.randn(T * S + 2 * guard, W + PAD, generator=gen).to(dtype)
    buf = full.to(DEV)
    n_cache = T * KVH * Lc * 128
    caches = torch.empty(2, n_cache + 2 * margin, dtype=dtype, device=DEV)                 # each cache inside its own poisoned margins
    caches.view(torch.uint8).fill_(POISON)
    kc, vc = (caches[i, margin:margin + n_cache].view(T, KVH, Lc, 128) for i in range(2))
    qkv = buf[guard:guard + T * S, :W]
    rc = L.bd_srv_rope_kv_append(_ptr(qkv), _ptr(cos), _ptr(sin), _ptr(kc), _ptr(vc), T, S, H, KVH, 128, buf.stride(0), Lc, pos0, _code(dtype),
                                 _stream())
    assert rc == 0, rc
    torch.cuda.synchronize()
    after = buf.cpu()
    keep = torch.ones_like(full, dtype=torch.bool)
    keep[guard:guard + T * S, :(H + KVH) * 128] = False                                    # the v heads, the padding and the guard rows: bit-untouched
    assert torch.equal(after.view(torch.int16)[keep], full.view(torch.int16)[keep]), "rope_kv_append: v heads, padding or neighbouring rows changed"
    rows = after[guard:guard + T * S]
    x64 = ref.to64(full[guard:guard + T * S, :(H + KVH) * 128]).reshape(T * S, H + KVH, 128)
    want, inter = ref.rope(x64, cos16, sin16, pos0 + np.arange(T * S) % S, dtype)             # q and k heads: the same model
    check(f"rope_kv_append ({T}, {S}, {H}, {KVH}, {Lc}, {pos0})", rows[:, :(H + KVH) * 128].reshape(T * S, H + KVH, 128), want, inter, np.ones(1), dtype,
          ref.ROPE_LIMITS)
    # the caches: exactly the rotated k rows and the raw v rows at pos0 .. pos0 + S - 1, poison everywhere else (margins included)
    expect = torch.empty(2, n_cache + 2 * margin, dtype=dtype)
    expect.view(torch.uint8).fill_(POISON)
    for i, first in enumerate((H, H + KVH)):
        heads = rows[:, first * 128:(first + KVH) * 128].reshape(T, S, KVH, 128).transpose(1, 2)
        expect[i, margin:margin + n_cache].view(T, KVH, Lc, 128)[:, :, pos0:pos0 + S] = heads
    assert torch.equal(caches.cpu().view(torch.int16), expect.view(torch.int16)), "rope_kv_append: a cache holds something else than the appended rows"


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_ID.get)
def test_rope_scores_depend_on_the_position_difference_only(L, tables, dtype):
    """one vector rotated to every position 0 .. 255 (as a q and as a k: rope_ treats them alike): q(m) . k(n) in float64 from the outputs is the
    same for three (m, n) with m - n = 7, within the half ulps of the vectors involved (glue_ref.rotation_spread) -- whatever the tables'
    convention.  A wrong partner or sign breaks this by far more (tests/test_glue_ref_host.py)."""
    cos, sin, _, _ = tables(dtype)
    vec = torch.randn(128, generator=torch.Generator().manual_seed(5)).to(dtype)
    buf = vec[None, :].expand(256, 128).contiguous().to(DEV)
    launch_rope(L, buf, 0, 256, 1, 256, 0, cos, sin, dtype)
    spread, tol = ref.rotation_spread(ref.to64(buf), ref.ROTATION_PAIRS, dtype)
    print(f"GLUE rope rotation {DT_ID[dtype]}: spread {spread:.3e}, tolerance {tol:.3e}")
    assert spread <= tol, (spread, tol)
