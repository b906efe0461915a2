"""Dispatch matrix of the decode Linear (launch_gemv_stream_chunk in csrc/bd_api.hip).

One decode Linear runs as one of several forms of gemv_stream_kernel -- per-stage loads, resident activation rows (XL = 2), the fine grid
of single-tile blocks (FG), the RMSNorm prologue (XL = 1), the hand-off producer / consumer (XL = 3), the SwiGLU epilogue -- each with the
row-major or the tile-major base weight, and bd_set_stream_tuning switches forms on and off at run time (16 / 32 nt weight loads,
64 / 128 resident rows, 256 / 512 fine grid, 1024 residual prefetch).  The design promises the same bits from every form.  Here every
launch kind of the three decode entry points runs under every flag set, on shapes at the edges of the dispatch rules (derived from the
device's CU count), and is checked against
  * its own flag-0 result, bit for bit (and the tile-major result against the row-major one);
  * a plain fp64 evaluation on the device (signs unpacked by shifts and masks, no kernel under test), tied to the C oracle below;
  * the separate launches it replaces (RMSNorm prologue, SwiGLU epilogue), bit for bit under the same flags;
  * poisoned margins around the outputs (CanaryOut) and poisoned outputs, so a stray or a missing store is caught;
  * bd_last_decode_form(), which must report the form that actually ran.
Launch kinds outside the envelope must be refused, never answered."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from canary import CanaryOut  # noqa: E402
from test_gpu_parity import within_one_ulp  # noqa: E402

pytestmark = pytest.mark.gpu

# product-build bits of bd_set_stream_tuning (the harness-only bits 0-3, 8192, 16384 are not in the shipped library)
FLAGS = (0, 16, 32, 64, 128, 256, 512, 1024, 128 | 512, 64 | 256, 16 | 128 | 1024, 32 | 64 | 512)
STREAM_XS_OFF, STREAM_LDS_MAX = 83968, 160 * 1024          # bd_gemv_stream.h: resident rows after the kernel's own LDS
STREAM_FG_XS_OFF, STREAM_FG_LDS_MAX = 22528, 80 * 1024     # ... and in the fine-grid kernels (two blocks per CU)
EPS = 1e-5
NORM_TOL = {torch.float16: 1.5e-3, torch.bfloat16: 8e-3}    # the hand-off tests' bound for the norm / SwiGLU forms (test_gpu_serving.py)


@pytest.fixture(scope="module")
def bd():
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    import bitdelta_amd
    from bitdelta_amd import _lib
    _lib.lib()
    return bitdelta_amd


def num_cus():
    return torch.cuda.get_device_properties(torch.cuda.current_device()).multi_processor_count


def t_pad_of(T):
    return next(v for v in (1, 2, 4, 6, 8, 12, 16) if v >= T)


def resident_rows_ok(T, K):
    """xres_ok of launch_gemv_stream_chunk for a tile-major M = 1 launch without a norm prologue"""
    nit = (K + 127) // 128
    return (T <= 8 and K >= 1024 and 3 * ((nit + 3) // 4) < nit and T * K <= 16 * 2048 and
            STREAM_XS_OFF + T * (2 * K + 16) <= STREAM_LDS_MAX)


def fine_grid_ok(T, K, N, C):
    """fg_ok of launch_gemv_stream_chunk: a resident-row launch of at most two 16-column tiles per CU whose rows fit the FG kernel's LDS"""
    return (resident_rows_ok(T, K) and N % 16 == 0 and t_pad_of(T) <= 6 and N // 16 <= 2 * C and
            STREAM_FG_XS_OFF + T * (2 * K + 16) <= STREAM_FG_LDS_MAX)


def expected_form(flags, eligible, consumer, tiles, C):
    """bd_last_decode_form() after one launch: 1 = the fine grid ran.  256 turns it off; so does 128 (no resident rows), except on the
    hand-off consumer, which is a resident-row form whatever the flags say; 512 takes it wherever eligible; by default it runs where
    the tile count is between one and two per CU."""
    if not eligible or flags & 256 or (flags & 128 and not consumer):
        return 0
    return 1 if (flags & 512 or tiles > C) else 0


def fp64_parts(xs, w, mask, max_elems=1 << 24):
    """xs [V, T, K] fp64 -> (base, delta), each [V, T, N] fp64: base = xs . W^T and delta = xs . S_t, with S_t = +-1 from tenant t's sign
    words mask [T, K/32, N] (bit i of word j is row k = 32 j + i) unpacked here by shifts and masks.  Column chunks keep every temporary
    at or below max_elems elements (128 MB of fp64)."""
    V, T, K = xs.shape
    N = w.shape[0]
    cols = max(16, max_elems // K)
    shifts = torch.arange(32, device=mask.device, dtype=torch.int32).view(1, 32, 1)
    base = torch.empty(V, T, N, dtype=torch.float64, device=xs.device)
    delta = torch.empty_like(base)
    for c0 in range(0, N, cols):
        c1 = min(N, c0 + cols)
        base[:, :, c0:c1] = xs @ w[c0:c1].double().T
        for t in range(T):
            bits = (mask[t, :, c0:c1].unsqueeze(1) >> shifts) & 1                  # [K/32, 32, n]
            s = bits.reshape(K, c1 - c0).double().mul_(2).sub_(1)
            delta[:, t, c0:c1] = xs[:, t] @ s
            del bits, s
    return base, delta


def rmsnorm64(x, nw):
    """HF RMSNorm in fp64: x [T, K] fp64, nw [T or 1, K]"""
    return x * torch.rsqrt(x.pow(2).mean(-1, keepdim=True) + EPS) * nw.double()


def swiglu64(y):
    """act_fn(gate) * up on the 8-interleaved gate|up layout ([g0..7 | u0..7 | g8..15 | ...]): y [T, N] -> [T, N/2]"""
    T, N = y.shape
    v = y.view(T, N // 16, 2, 8)
    return (torch.nn.functional.silu(v[:, :, 0]) * v[:, :, 1]).reshape(T, N // 2)


def rel(a, ref):
    a, ref = a.double(), ref.double()
    return ((a - ref).norm() / ref.norm()).item()


def poisoned(shape, dtype):
    """a fresh output that starts as large finite values: a column the launch never writes misses the reference"""
    if dtype == torch.float32:
        return torch.full(shape, 0x7F7F7F7F, dtype=torch.int32, device="cuda").view(torch.float32)
    return torch.full(shape, 0x7F7F, dtype=torch.int16, device="cuda").view(dtype)


def first_difference(v, ref):
    bad = (v != ref).reshape(-1, v.shape[-1]).any(0).nonzero()
    return f"first differing column {int(bad[0])} of {v.shape[-1]}" if len(bad) else "?"


def run_matrix(dtype, T, K, N, seed=0):
    """Every launch kind under every flag set for one shape.  Returns (flag-0 outputs keyed "layout/kind/name", list of problems)."""
    from bitdelta_amd import _lib
    from bitdelta_amd import serving_ops as ops
    from bitdelta_amd._lib import BitDeltaHipError
    from bitdelta_amd.binary_gemm_kernel import binary_linear_decode, fused_norm_ok, handoff_ok, pack_decode_masks, tile_weight
    L = _lib.lib()
    C = num_cus()
    tiles = N // 16
    g = torch.Generator(device="cuda").manual_seed(seed + 7 * K + N + T)
    x = (torch.randn(T, 1, K, device="cuda", generator=g) * 1.5).to(dtype)
    w = (torch.randn(N, K, device="cuda", generator=g) * 0.02).to(dtype)
    mask = torch.randint(-2**31, 2**31 - 1, (T, K // 32, N), device="cuda", generator=g, dtype=torch.int64).to(torch.int32)
    alpha = torch.rand(T, 2, device="cuda", generator=g) * 1e-3 + 2e-4          # (gate, up) scales of the SwiGLU forms
    a1 = alpha[:, :1].contiguous()
    res = torch.randn(T, 1, N, device="cuda", generator=g).to(dtype)
    nw = (1 + 0.1 * torch.randn(T, K, device="cuda", generator=g)).to(dtype)      # the norm in front of this Linear
    nwn = (1 + 0.1 * torch.randn(T, N, device="cuda", generator=g)).to(dtype)     # the norm after it (the producer's pre-multiplied copy)
    pk = pack_decode_masks(mask)
    weights = {"row": w}
    if N % 16 == 0:
        weights["tile"] = tile_weight(w)
    else:
        with pytest.raises(AssertionError):
            tile_weight(w)
    a8 = alpha.repeat(1, N // 16).contiguous() if N % 16 == 0 else None            # the same scales as N/8 groups of 8 columns
    # strided activations: row stride K + 128, the gap filled with values that would blow up any result that read them
    xs_buf = torch.full((T, 1, K + 128), 1.0e4, device="cuda").to(dtype)
    xs_buf[..., :K] = x
    xs = xs_buf[..., :K]
    # hand-off consumer inputs: what a producer hands over for the rows x and the norm weight nw
    xw_in = (x.float() * nw.float()[:, None, :]).to(dtype)
    ssq_in = torch.zeros(K // 16, 16, device="cuda")
    ssq_in[:, :T] = (x.float()[:, 0].reshape(T, K // 16, 16) ** 2).sum(-1).T

    def lin(xin, al, tiled, **kw):
        return binary_linear_decode(xin, weights["tile" if tiled else "row"], pk, al, layout="packed", weight_tiled=tiled, **kw)

    def into(n, call, dt=dtype, fill=None):
        """run `call(out)` with `out` a CanaryOut view of [T, 1, n]"""
        c = CanaryOut(T, 1, n, dt, row_margin=4, col_margin=64)
        if fill is not None:
            c.view.copy_(fill)
        call(c.view)
        return {"y": c}

    def producer(tiled, *, resid=True, scale=1.0, nrm=None):
        out = {"ssq": torch.full((N // 16, 16), float("nan"), device="cuda")}
        if nrm is not None:
            out["xw"] = CanaryOut(T, 1, N, dtype, row_margin=4, col_margin=64)    # the output's geometry: the same strides
        xw = out["xw"].view if nrm is not None else None
        if resid:
            out.update(into(N, lambda o: lin(x, a1, tiled, residual=o, ssq_out=out["ssq"], ssq_scale=scale, norm_weight=nrm, xw_out=xw),
                            fill=res))
        else:
            out.update(into(N, lambda o: lin(x, a1, tiled, out=o, ssq_out=out["ssq"], ssq_scale=scale, norm_weight=nrm, xw_out=xw)))
        return out

    def swiglu_sep(xin, tiled):
        return ops.swiglu_interleaved8(lin(xin, a8, tiled, groups=N // 8))

    base_ok = lambda tl: not tl or N % 16 == 0
    sw_ok = lambda tl: base_ok(tl) and N % 16 == 0
    norm_ok = lambda tl: base_ok(tl) and fused_norm_ok(T, 1, K)
    prod_ok = lambda tl: base_ok(tl) and T <= 8 and N % 16 == 0
    cons_ok = lambda tl: tl and handoff_ok(T, 1, K) and K <= 8192
    # kind: (allowed(tiled), launch(tiled) -> {name: tensor or CanaryOut}, takes part in the form check, is a hand-off consumer)
    kinds = {
        "plain": (base_ok, lambda tl: {"y": lin(x, a1, tl, out=poisoned((T, 1, N), dtype))}, True, False),
        "f32": (base_ok, lambda tl: into(N, lambda o: lin(x, a1, tl, out_dtype=torch.float32, out=o), dt=torch.float32), True, False),
        "resid": (base_ok, lambda tl: into(N, lambda o: lin(x, a1, tl, residual=o), fill=res), True, False),
        "out_strided": (base_ok, lambda tl: into(N, lambda o: lin(x, a1, tl, out=o)), True, False),
        "x_strided": (base_ok, lambda tl: {"y": lin(xs, a1, tl, out=poisoned((T, 1, N), dtype))}, True, False),
        "alpha_bcast": (base_ok, lambda tl: {"y": lin(x, a1[:1], tl, out=poisoned((T, 1, N), dtype))}, True, False),
        "swiglu": (sw_ok, lambda tl: into(N // 2, lambda o: lin(x, alpha, tl, groups=2, swiglu=True, out=o)), True, False),
        "norm": (norm_ok, lambda tl: into(N, lambda o: lin(x, a1, tl, norm_weight=nw, eps=EPS, out=o)), False, False),
        "norm_b": (norm_ok, lambda tl: into(N, lambda o: lin(x, a1, tl, norm_weight=nw[:1], eps=EPS, out=o)), False, False),
        "norm_swiglu": (lambda tl: norm_ok(tl) and sw_ok(tl),
                        lambda tl: into(N // 2, lambda o: lin(x, alpha, tl, groups=2, swiglu=True, norm_weight=nw, eps=EPS, out=o)),
                        False, False),
        "norm_b_swiglu": (lambda tl: norm_ok(tl) and sw_ok(tl),
                          lambda tl: into(N // 2, lambda o: lin(x, alpha, tl, groups=2, swiglu=True, norm_weight=nw[:1], eps=EPS, out=o)),
                          False, False),
        "prod": (prod_ok, lambda tl: producer(tl), True, False),
        "prod_s6": (prod_ok, lambda tl: producer(tl, scale=2.0 ** -6), True, False),
        "prod_s0": (prod_ok, lambda tl: producer(tl, scale=0.0), True, False),
        "prod_plain": (prod_ok, lambda tl: producer(tl, resid=False), True, False),
        "prod_xw": (prod_ok, lambda tl: producer(tl, nrm=nwn), True, False),
        "prod_xw_b": (prod_ok, lambda tl: producer(tl, scale=2.0 ** -6, nrm=nwn[:1]), True, False),
        "cons": (cons_ok, lambda tl: into(N, lambda o: lin(xw_in, a1, tl, ssq_in=ssq_in, eps=EPS, out=o)), True, True),
        "cons_swiglu": (lambda tl: cons_ok(tl) and sw_ok(tl),
                        lambda tl: into(N // 2, lambda o: lin(xw_in, alpha, tl, groups=2, swiglu=True, ssq_in=ssq_in, eps=EPS, out=o)),
                        True, True),
    }
    # the separate launches the fused forms replace (same bits under the same flags)
    seps = {
        "swiglu": lambda tl: swiglu_sep(x, tl),
        "norm": lambda tl: lin(ops.rmsnorm_tenant(x, nw, EPS), a1, tl),
        "norm_b": lambda tl: lin(ops.rmsnorm_tenant(x, nw[:1].expand(T, K).contiguous(), EPS), a1, tl),
        "norm_swiglu": lambda tl: swiglu_sep(ops.rmsnorm_tenant(x, nw, EPS), tl),
        "norm_b_swiglu": lambda tl: swiglu_sep(ops.rmsnorm_tenant(x, nw[:1].expand(T, K).contiguous(), EPS), tl),
    }

    problems = []
    first = {}

    def note(ok, what):
        if not ok:
            problems.append(what)

    try:
        for flags in FLAGS:
            L.bd_set_stream_tuning(flags)
            for layout in weights:
                tiled = layout == "tile"
                eligible = tiled and fine_grid_ok(T, K, N, C)
                for kind, (allowed, launch, form_checked, consumer) in kinds.items():
                    tag = f"flags={flags} {layout} {kind}"
                    if not allowed(tiled):
                        try:
                            launch(tiled)
                            note(False, f"{tag}: outside the envelope but not refused")
                        except (BitDeltaHipError, AssertionError):
                            pass
                        continue
                    got = launch(tiled)
                    if form_checked:
                        form, want = L.bd_last_decode_form(), expected_form(flags, eligible, consumer, tiles, C)
                        note(form == want, f"{tag}: bd_last_decode_form() = {form}, expected {want}")
                    for name, v in list(got.items()):
                        if isinstance(v, CanaryOut):
                            note(v.untouched_outside(), f"{tag}: store outside the {name} output")
                            got[name] = v.result()
                    if "ssq" in got:
                        note(bool(torch.isnan(got["ssq"][:, T:]).all()), f"{tag}: ssq_out rows past T were written")
                        got["ssq"] = got["ssq"][:, :T].clone()
                    if kind in seps:
                        got["sep"] = seps[kind](tiled)
                        note(torch.equal(got["y"], got["sep"]), f"{tag}: fused form differs from the separate launches, "
                             f"{first_difference(got['y'], got['sep'])}")
                    for name, v in got.items():
                        key = f"{layout}/{kind}/{name}"
                        if flags == 0:
                            first[key] = v
                        elif not torch.equal(v, first[key]):
                            note(False, f"{tag}: {name} differs from flag 0, {first_difference(v, first[key])}")
    finally:
        L.bd_set_stream_tuning(0)

    # ---- flag 0 against the fp64 reference (and tile-major against row-major, bit for bit)
    for key in first:
        if key.startswith("tile/") and "row/" + key[5:] in first:
            note(torch.equal(first[key], first["row/" + key[5:]]), f"{key}: tile-major differs from row-major")
    x64 = x.double()[:, 0]
    xn = torch.stack([x64, rmsnorm64(x64, nw), rmsnorm64(x64, nw[:1])])              # [3, T, K]: raw, normed, normed by a broadcast weight
    base, delta = fp64_parts(xn, w, mask)
    lin1 = base + a1.double() * delta                                                # [3, T, N]
    lin2 = base + alpha.double()[:, (torch.arange(N, device="cuda") // 8) % 2] * delta   # per-column (gate, up) scales
    ref = lin1[0]
    tol = NORM_TOL[dtype]
    for layout in weights:
        def f(kind, name="y"):
            v = first.get(f"{layout}/{kind}/{name}")
            return v if v is None or name == "ssq" else v[:, 0]

        def near16(kind, want):
            got = f(kind)
            if got is not None:
                ok, frac = within_one_ulp(got, want.to(dtype), K)
                note(ok and frac >= 0.99, f"{layout} {kind}: not within 1 ulp of the fp64 reference ({frac:.4f} bit-equal, "
                     f"rel {rel(got, want):.2e})")
        near16("plain", ref)
        near16("out_strided", ref)
        near16("x_strided", ref)
        near16("alpha_bcast", base[0] + a1[:1].double() * delta[0])
        near16("resid", res.double()[:, 0] + ref)
        if f("f32") is not None:
            note(rel(f("f32"), ref) <= 1e-5, f"{layout} f32: rel {rel(f('f32'), ref):.2e} > 1e-5")
        for kind, want in (("swiglu", lambda: swiglu64(lin2[0])), ("norm", lambda: lin1[1]), ("norm_b", lambda: lin1[2]),
                           ("norm_swiglu", lambda: swiglu64(lin2[1])), ("norm_b_swiglu", lambda: swiglu64(lin2[2])), ("cons", lambda: lin1[1]),
                           ("cons_swiglu", lambda: swiglu64(lin2[1]))):
            if f(kind) is not None:                 # (a SwiGLU kind ran only if N % 16 == 0)
                e = rel(f(kind), want())
                note(e <= tol, f"{layout} {kind}: rel {e:.2e} > {tol:.1e} against the fp64 reference")
        if f("prod") is not None:
            y = f("prod")
            note(torch.equal(y, f("resid")), f"{layout} prod: output differs from the residual launch")
            note(torch.equal(f("prod_plain"), f("plain")), f"{layout} prod_plain: output differs from the plain launch")
            for kind in ("prod", "prod_plain"):
                want = (f(kind).double().reshape(T, N // 16, 16) ** 2).sum(-1).T       # sums of squares of the STORED values
                note(torch.allclose(f(kind, "ssq").double(), want, rtol=1e-5, atol=1e-6), f"{layout} {kind}: ssq_out wrong")
            s1 = f("prod", "ssq")
            note(torch.equal(f("prod_s6", "ssq"), s1 * 2.0 ** -6), f"{layout} prod_s6: sums are not exactly 2^-6 x the scale-1 sums")
            note(torch.equal(f("prod_s0", "ssq"), s1), f"{layout} prod_s0: ssq_scale 0 is not taken as 1")
            for kind, nrm, sc in (("prod_xw", nwn, 1.0), ("prod_xw_b", nwn[:1], 2.0 ** -6)):
                note(torch.equal(f(kind), y) and torch.equal(f(kind, "ssq"), s1 * sc), f"{layout} {kind}: output / sums differ")
                note(torch.equal(f(kind, "xw"), (y.float() * nrm.float()).to(dtype)), f"{layout} {kind}: xw_out != round(y * nw)")
    return first, problems


def _resolve_n(Nspec):
    """N, or ("C", a, b[, extra]) -> 16 (a C + b) + extra columns, with C the device's CU count"""
    if isinstance(Nspec, tuple):
        _, a, b, *extra = Nspec
        return 16 * (a * num_cus() + b) + sum(extra)
    return Nspec


C1 = ("C", 1, 1)
SHAPES = [
    pytest.param(6, 4096, ("C", 1, 0), id="tiles=C"),
    pytest.param(6, 4096, C1, id="tiles=C+1"),
    pytest.param(6, 4096, ("C", 2, 0), id="tiles=2C"),
    pytest.param(6, 4096, ("C", 2, 1), id="tiles=2C+1"),
    pytest.param(6, 4096, 6144, id="mistral-qkv"),
    pytest.param(6, 4096, 4096, id="mistral-o"),
    pytest.param(2, 1152, C1, id="K1152-empty-wave"),
    pytest.param(2, 1280, C1, id="K1280"),
    pytest.param(4, 1024, C1, id="K1024-smallest-resident"),
    pytest.param(8, 4096, C1, id="BK=32768"),
    pytest.param(8, 4224, C1, id="BK-above-32768-tpad8"),
    pytest.param(6, 5504, C1, id="BK-above-32768-tpad6"),
    pytest.param(3, 8192, C1, id="3x8192-fg-lds-fits"),
    pytest.param(4, 8192, C1, id="4x8192-fg-lds-over"),
    pytest.param(1, 4096, C1, id="1-tenant"),
    pytest.param(5, 2048, ("C", 2, 0), id="5-tenants-tpad6"),
    pytest.param(7, 4096, C1, id="7-tenants-tpad8"),
    pytest.param(9, 2048, C1, id="9-tenants"),
    pytest.param(12, 2048, C1, id="12-tenants"),
    pytest.param(16, 2048, C1, id="16-tenants"),
    pytest.param(2, 2048, ("C", 1, 1, 8), id="ragged-N"),
    pytest.param(6, 14336, 4096, id="mistral-down"),
    pytest.param(6, 4096, 2 * 14336, id="mistral-gate-up"),
]


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], ids=["fp16", "bf16"])
@pytest.mark.parametrize("T,K,Nspec", SHAPES)
def test_decode_forms_match_fp64_and_each_other_under_every_flag(bd, dtype, T, K, Nspec):
    """every launch kind x weight layout x flag set of the decode entry points: the same bits as at flag 0, close to fp64 at flag 0, no store
    outside the output, refused outside the envelope, and bd_last_decode_form() reports what ran"""
    N = _resolve_n(Nspec)
    _, problems = run_matrix(dtype, T, K, N)
    assert not problems, f"{len(problems)} problems (T = {T}, K = {K}, N = {N}, C = {num_cus()}):\n" + "\n".join(problems[:40])


@pytest.mark.parametrize("T,K,N", [(3, 256, 528), (2, 1024, 4096)])
def test_fp64_reference_agrees_with_the_c_oracle(bd, oracle, T, K, N):
    """the fp64 reference of this module states the operation the C oracle (fp32) computes: y = x W^T + alpha (x S), per-tenant and
    broadcast alpha"""
    g = torch.Generator().manual_seed(T + K + N)
    x = torch.randn(T, 1, K, generator=g).to(torch.float16)
    w = (torch.randn(N, K, generator=g) * 0.02).to(torch.float16)
    mask = torch.randint(-2**31, 2**31 - 1, (T, K // 32, N), generator=g, dtype=torch.int64).to(torch.int32)
    alpha = torch.rand(T, 1, generator=g) * 1e-2 + 1e-3
    base, delta = fp64_parts(x.double().cuda()[None, :, 0], w.cuda(), mask.cuda())
    base, delta = base[0].cpu(), delta[0].cpu()
    for al in (alpha, alpha[:1]):
        want = oracle.binary_linear(x, w, mask, al, out_dtype=torch.float32)[:, 0].double()
        assert rel(base + al.double() * delta, want) <= 1e-6
        assert rel(al.double() * delta, want - base) <= 1e-4          # the delta term itself, not only the dominant base
