"""The decode Linear with a 4-BIT GPTQ base weight (bd_binary_linear_decode_q4; gemv_stream_kernel WT = 3) on the device.

    Y[t, n] = round( sum_k X[t,k] Wdq[n,k]  +  alpha[t, g(n)] * sum_k X[t,k] S_t[k,n]  [+ residual] ),   Wdq = quant.dequantize_base_gptq4(...)

Wdq is the weight the reference's own dequantisation leaves in the model (bitdelta/misc.py:76-105; quant.dequantize_base_gptq4 is pinned bit for
bit by the reference-generated tests/golden/gptq4.pt in test_q4_host.py).  The kernel must rebuild exactly that weight in registers: the first
test reads single weights back through one-hot activations, with no tolerance.  Then the matrix of test_gpu_w8_decode.run_matrix: every launch
kind x every product flag set bit-identical to flag 0, fused prologue / epilogue bit-identical to the separate launches, canaries,
bd_last_decode_form(); flag 0 against fp64 of the formula on Wdq (exact in fp64) under the 16-bit path's own gates -- the launch IS a 16-bit
launch on those weights.  Then the envelope, and the decoder level."""
import os
import sys
import types

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from canary import CanaryOut  # noqa: E402
from test_gpu_decode_forms import (EPS, FLAGS, NORM_TOL, expected_form, fine_grid_ok, first_difference, fp64_parts, num_cus,  # noqa: E402
                                   poisoned, rel, rmsnorm64, swiglu64, _resolve_n)
from test_gpu_parity import within_one_ulp  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def bd():
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    import bitdelta_amd
    from bitdelta_amd import _lib
    _lib.lib()
    return bitdelta_amd


def random_checkpoint(N, K, G, gen, device="cuda"):
    """a GPTQ triple with every nibble value in play: random dwords, zero nibbles 0 .. 15 (z = 1 .. 16), scales that differ per (group, column)"""
    qw = torch.randint(-2**31, 2**31 - 1, (K // 8, N), device=device, generator=gen, dtype=torch.int64).to(torch.int32)
    qz = torch.randint(-2**31, 2**31 - 1, (K // G, N // 8), device=device, generator=gen, dtype=torch.int64).to(torch.int32)
    sc = ((torch.rand(K // G, N, device=device, generator=gen) * 1.5 + 0.25) * 0.02 / 8).half()
    return qw, qz, sc


def make_problem(dtype, T, K, N, seed=0, G=128):
    from bitdelta_amd.binary_gemm_kernel import pack_decode_masks
    from bitdelta_amd.quant import dequantize_base_gptq4, pack_gptq4_params, tile_weight_gptq4
    g = torch.Generator(device="cuda").manual_seed(seed + 7 * K + N + T)
    p = types.SimpleNamespace(T=T, K=K, N=N, dtype=dtype, G=G)
    p.x = (torch.randn(T, 1, K, device="cuda", generator=g) * 1.5).to(dtype)
    p.qw, p.qz, p.sc = random_checkpoint(N, K, G, g)
    p.wdq = dequantize_base_gptq4(p.qw, p.qz, p.sc, dtype)            # [N, K], what the reference leaves in the model
    p.w4 = tile_weight_gptq4(p.qw)
    p.gp = pack_gptq4_params(p.qz, p.sc)
    p.mask = torch.randint(-2**31, 2**31 - 1, (T, K // 32, N), device="cuda", generator=g, dtype=torch.int64).to(torch.int32)
    p.alpha = torch.rand(T, 2, device="cuda", generator=g) * 1e-3 + 2e-4
    p.a1 = p.alpha[:, :1].contiguous()
    p.res = torch.randn(T, 1, N, device="cuda", generator=g).to(dtype)
    p.nw = (1 + 0.1 * torch.randn(T, K, device="cuda", generator=g)).to(dtype)
    p.nwn = (1 + 0.1 * torch.randn(T, N, device="cuda", generator=g)).to(dtype)
    p.pk = pack_decode_masks(p.mask)
    return p


# ------------------------------------------------------------------------------------------------------------------ exact weights
@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], ids=["fp16", "bf16"])
@pytest.mark.parametrize("K,N,G", [(1024, 512, 128), (2048, 1024, 256)])
def test_q4_one_hot_rows_read_back_the_reference_weight_exactly(bd, dtype, K, N, G):
    """x[t] = e_k (value 1), alpha = 0, fp32 output: Y[t, :] = Wdq[:, k], every column, bit for bit.  The rows cover every in-dword nibble
    position, every MFMA step and lane group, the first and last k of a group, the last iteration; the columns hold z = 1 and z = 16."""
    from bitdelta_amd.binary_gemm_kernel import binary_linear_decode, pack_decode_masks
    from bitdelta_amd.quant import dequantize_base_gptq4, pack_gptq4_params, tile_weight_gptq4
    g = torch.Generator(device="cuda").manual_seed(K + N + G)
    qw, qz, sc = random_checkpoint(N, K, G, g)
    qz[:, 0] = (qz[:, 0] & ~0xFF) | 0xF0                     # columns 0 / 1 of every group: z = 1 / z = 16
    qz[:, -1] = (qz[:, -1] & 0x0FFFFFF0) | (-2**31 >> 3)      # ... and the last dword: nibble 7 = 15 (sign bits), nibble 0 = 0
    sc[0, 3], sc[-1, 5] = 6.0e-8, 3.0e-5                      # products in fp16's subnormal range, and a scale that is itself subnormal-adjacent
    nib = torch.stack([(qz >> (4 * i)) & 15 for i in range(8)])
    assert bool((nib == 0).any()) and bool((nib == 15).any())
    wdq = dequantize_base_gptq4(qw, qz, sc, dtype)
    w4, gp = tile_weight_gptq4(qw), pack_gptq4_params(qz, sc)
    ks = sorted(set(
        list(range(8)) +                                      # every nibble position of one dword (step 0, lane group 0)
        [32 * s + 8 * gg + ((3 * s + gg) % 8) for s in range(4) for gg in range(4)] +      # every MFMA step x lane group
        [G - 1, G, 2 * G - 1, 2 * G, K - G, K - 128, K - 1, K - 8, K // 2 + 77]))            # group ends, last group / iteration / element
    mask = torch.randint(-2**31, 2**31 - 1, (1, K // 32, N), device="cuda", generator=g, dtype=torch.int64).to(torch.int32)
    alpha0 = torch.zeros(1, 1, device="cuda")
    seen = 0
    for lo in range(0, len(ks), 16):
        rows = ks[lo:lo + 16]
        T = len(rows)
        x = torch.zeros(T, 1, K, device="cuda", dtype=dtype)
        for t, k in enumerate(rows):
            x[t, 0, k] = 1
        pk = pack_decode_masks(mask.expand(T, -1, -1).contiguous())
        y = binary_linear_decode(x, w4, pk, alpha0.expand(T, 1).contiguous(), layout="packed", weight_tiled=True, group_params=gp, group_size=G,
                                 out_dtype=torch.float32)[:, 0]
        want = wdq[:, rows].T.float()
        bad = (y != want).nonzero()
        assert len(bad) == 0, (f"{len(bad)} weights differ; first: k = {rows[int(bad[0, 0])]}, column {int(bad[0, 1])}: got "
                               f"{float(y[bad[0, 0], bad[0, 1]])!r}, reference {float(want[bad[0, 0], bad[0, 1]])!r}")
        seen += T
    assert seen == len(ks) >= 30


# ------------------------------------------------------------------------------------------------------------------ launch-kind matrix
def run_matrix(dtype, T, K, N, seed=0, G=128):
    """Every launch kind of the 4-bit base under every flag set for one shape.  Returns (flag-0 outputs, problems, the problem's tensors)."""
    from bitdelta_amd import _lib
    from bitdelta_amd import serving_ops as ops
    from bitdelta_amd.binary_gemm_kernel import binary_linear_decode, fused_norm_ok, handoff_ok
    L = _lib.lib()
    C = num_cus()
    tiles = N // 16
    p = make_problem(dtype, T, K, N, seed, G)
    x, a1, alpha, res, nw, nwn = p.x, p.a1, p.alpha, p.res, p.nw, p.nwn
    a8 = alpha.repeat(1, N // 16).contiguous()
    xs_buf = torch.full((T, 1, K + 128), 1.0e4, device="cuda").to(dtype)
    xs_buf[..., :K] = x
    xs = xs_buf[..., :K]
    xw_in = (x.float() * nw.float()[:, None, :]).to(dtype)
    ssq_in = torch.zeros(K // 16, 16, device="cuda")
    ssq_in[:, :T] = (x.float()[:, 0].reshape(T, K // 16, 16) ** 2).sum(-1).T

    def lin(xin, al, **kw):
        return binary_linear_decode(xin, p.w4, p.pk, al, layout="packed", weight_tiled=True, group_params=p.gp, group_size=G, **kw)

    def into(n, call, dt=dtype, fill=None):
        c = CanaryOut(T, 1, n, dt, row_margin=4, col_margin=64)
        if fill is not None:
            c.view.copy_(fill)
        call(c.view)
        return {"y": c}

    def producer(*, resid=True, scale=1.0, nrm=None):
        out = {"ssq": torch.full((N // 16, 16), float("nan"), device="cuda")}
        if nrm is not None:
            out["xw"] = CanaryOut(T, 1, N, dtype, row_margin=4, col_margin=64)
        xw = out["xw"].view if nrm is not None else None
        if resid:
            out.update(into(N, lambda o: lin(x, a1, residual=o, ssq_out=out["ssq"], ssq_scale=scale, norm_weight=nrm, xw_out=xw), fill=res))
        else:
            out.update(into(N, lambda o: lin(x, a1, out=o, ssq_out=out["ssq"], ssq_scale=scale, norm_weight=nrm, xw_out=xw)))
        return out

    def swiglu_sep(xin):
        return ops.swiglu_interleaved8(lin(xin, a8, groups=N // 8))

    norm_ok = fused_norm_ok(T, 1, K)
    prod_ok = T <= 8
    cons_ok = handoff_ok(T, 1, K) and K <= 8192
    # kind: (allowed, launch -> {name: tensor or CanaryOut}, takes part in the form check, is a hand-off consumer)
    kinds = {
        "plain": (True, lambda: {"y": lin(x, a1, out=poisoned((T, 1, N), dtype))}, True, False),
        "f32": (True, lambda: into(N, lambda o: lin(x, a1, out_dtype=torch.float32, out=o), dt=torch.float32), True, False),
        "resid": (True, lambda: into(N, lambda o: lin(x, a1, residual=o), fill=res), True, False),
        "resid_f32": (True, lambda: into(N, lambda o: lin(x, a1, out_dtype=torch.float32, residual=o), dt=torch.float32, fill=res.float()),
                      True, False),
        "x_strided": (True, lambda: {"y": lin(xs, a1, out=poisoned((T, 1, N), dtype))}, True, False),
        "alpha_bcast": (True, lambda: {"y": lin(x, a1[:1], out=poisoned((T, 1, N), dtype))}, True, False),
        "swiglu": (True, lambda: into(N // 2, lambda o: lin(x, alpha, groups=2, swiglu=True, out=o)), True, False),
        "norm": (norm_ok, lambda: into(N, lambda o: lin(x, a1, norm_weight=nw, eps=EPS, out=o)), False, False),
        "norm_b": (norm_ok, lambda: into(N, lambda o: lin(x, a1, norm_weight=nw[:1], eps=EPS, out=o)), False, False),
        "norm_swiglu": (norm_ok, lambda: into(N // 2, lambda o: lin(x, alpha, groups=2, swiglu=True, norm_weight=nw, eps=EPS, out=o)),
                        False, False),
        "prod": (prod_ok, lambda: producer(), True, False),
        "prod_plain": (prod_ok, lambda: producer(resid=False), True, False),
        "prod_xw": (prod_ok, lambda: producer(scale=2.0 ** -6, nrm=nwn), True, False),
        "cons": (cons_ok, lambda: into(N, lambda o: lin(xw_in, a1, ssq_in=ssq_in, eps=EPS, out=o)), True, True),
        "cons_swiglu": (cons_ok, lambda: into(N // 2, lambda o: lin(xw_in, alpha, groups=2, swiglu=True, ssq_in=ssq_in, eps=EPS, out=o)),
                        True, True),
    }
    seps = {
        "swiglu": lambda: swiglu_sep(x),
        "norm": lambda: lin(ops.rmsnorm_tenant(x, nw, EPS), a1),
        "norm_b": lambda: lin(ops.rmsnorm_tenant(x, nw[:1].expand(T, K).contiguous(), EPS), a1),
        "norm_swiglu": lambda: swiglu_sep(ops.rmsnorm_tenant(x, nw, EPS)),
    }
    problems, first = [], {}

    def note(ok, what):
        if not ok:
            problems.append(what)

    eligible = fine_grid_ok(T, K, N, C)
    try:
        for flags in FLAGS:
            L.bd_set_stream_tuning(flags)
            for kind, (allowed, launch, form_checked, consumer) in kinds.items():
                tag = f"flags={flags} {kind}"
                if not allowed:
                    try:
                        launch()
                        note(False, f"{tag}: outside the envelope but not refused")
                    except (_lib.BitDeltaHipError, AssertionError, ValueError):
                        pass
                    continue
                got = launch()
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
                    got["sep"] = seps[kind]()
                    note(torch.equal(got["y"], got["sep"]), f"{tag}: fused form differs from the separate launches, "
                         f"{first_difference(got['y'], got['sep'])}")
                for name, v in got.items():
                    key = f"{kind}/{name}"
                    if flags == 0:
                        first[key] = v
                    elif not torch.equal(v, first[key]):
                        note(False, f"{tag}: {name} differs from flag 0, {first_difference(v, first[key])}")
    finally:
        L.bd_set_stream_tuning(0)

    # ---- flag 0 against fp64 of the formula on the dequantised 16-bit weight (exact in fp64)
    x64 = x.double()[:, 0]
    xn = torch.stack([x64, rmsnorm64(x64, nw), rmsnorm64(x64, nw[:1])])
    base, delta = fp64_parts(xn, p.wdq, p.mask)
    lin1 = base + a1.double() * delta
    lin2 = base + alpha.double()[:, (torch.arange(N, device="cuda") // 8) % 2] * delta
    ref = lin1[0]
    tol = NORM_TOL[dtype]

    def f(kind, name="y"):
        v = first.get(f"{kind}/{name}")
        return v if v is None or name == "ssq" else v[:, 0]

    def near16(kind, want):
        ok, frac = within_one_ulp(f(kind), want.to(dtype), K)
        note(ok and frac >= 0.99, f"{kind}: not within 1 ulp of the fp64 reference ({frac:.4f} bit-equal, rel {rel(f(kind), want):.2e})")
    near16("plain", ref)
    near16("x_strided", ref)
    near16("alpha_bcast", base[0] + a1[:1].double() * delta[0])
    near16("resid", res.double()[:, 0] + ref)
    note(rel(f("f32"), ref) <= 1e-5, f"f32: rel {rel(f('f32'), ref):.2e} > 1e-5")
    note(rel(f("resid_f32"), res.double()[:, 0] + ref) <= 1e-5, "resid_f32: rel > 1e-5")
    for kind, want in (("swiglu", lambda: swiglu64(lin2[0])), ("norm", lambda: lin1[1]), ("norm_b", lambda: lin1[2]),
                       ("norm_swiglu", lambda: swiglu64(lin2[1])), ("cons", lambda: lin1[1]), ("cons_swiglu", lambda: swiglu64(lin2[1]))):
        if f(kind) is not None:
            e = rel(f(kind), want())
            note(e <= tol, f"{kind}: rel {e:.2e} > {tol:.1e} against the fp64 reference")
    if f("prod") is not None:
        y = f("prod")
        note(torch.equal(y, f("resid")), "prod: output differs from the residual launch")
        note(torch.equal(f("prod_plain"), f("plain")), "prod_plain: output differs from the plain launch")
        for kind in ("prod", "prod_plain"):
            want = (f(kind).double().reshape(T, N // 16, 16) ** 2).sum(-1).T
            note(torch.allclose(f(kind, "ssq").double(), want, rtol=1e-5, atol=1e-6), f"{kind}: ssq_out wrong")
        note(torch.equal(f("prod_xw"), y) and torch.equal(f("prod_xw", "ssq"), f("prod", "ssq") * 2.0 ** -6), "prod_xw: output / sums differ")
        note(torch.equal(f("prod_xw", "xw"), (y.float() * nwn.float()).to(dtype)), "prod_xw: xw_out != round(y * nw)")
    return first, problems, p, ref


C1 = ("C", 1, 1)
SHAPES = [
    pytest.param(1, 4096, C1, 128, id="T1-tiles=C+1-fine-grid"),
    pytest.param(3, 4096, C1, 128, id="T3-tiles=C+1-fine-grid"),
    pytest.param(6, 4096, C1, 128, id="T6-tiles=C+1-fine-grid"),
    pytest.param(8, 4096, C1, 128, id="T8-tiles=C+1-tpad8-no-fine-grid"),
    pytest.param(6, 4096, ("C", 1, 0), 128, id="T6-tiles=C"),
    pytest.param(3, 4096, ("C", 2, 0), 128, id="T3-tiles=2C"),
    pytest.param(6, 4096, ("C", 2, 1), 128, id="T6-tiles=2C+1-not-eligible"),
    pytest.param(1, 4096, ("C", 2, 1), 128, id="T1-tiles=2C+1-not-eligible"),
    pytest.param(6, 4096, 6144, 128, id="mistral-qkv"),
    pytest.param(6, 14336, 4096, 128, id="mistral-down-per-stage-rows"),
    pytest.param(6, 4096, 2 * 14336, 128, id="mistral-gate-up-7-tiles-per-block"),
    pytest.param(3, 1024, ("C", 9, 0), 128, id="9-tiles-per-block"),
    pytest.param(8, 1152, C1, 128, id="K1152-empty-wave"),
    pytest.param(1, 1024, 512, 128, id="smallest"),
    pytest.param(2, 4096, 6144, 256, id="G256-two-stages-per-group"),
]


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], ids=["fp16", "bf16"])
@pytest.mark.parametrize("T,K,Nspec,G", SHAPES)
def test_q4_decode_forms_match_fp64_and_each_other_under_every_flag(bd, dtype, T, K, Nspec, G):
    N = _resolve_n(Nspec)
    _, problems, _, _ = run_matrix(dtype, T, K, N, G=G)
    assert not problems, f"{len(problems)} problems (T = {T}, K = {K}, N = {N}, G = {G}, C = {num_cus()}):\n" + "\n".join(problems[:40])


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], ids=["fp16", "bf16"])
@pytest.mark.parametrize("T,K,N,G", [(1, 4096, 4096, 128), (6, 4096, 6144, 128), (3, 14336, 4096, 1024), (3, 14336, 4096, 896),
                                     (2, 4096, 1024, 4096), (2, 1920, 1024, 640)])
def test_q4_launch_is_the_16_bit_launch_on_the_dequantised_weight(bd, dtype, T, K, N, G):
    """the accumulators hold what a tile-major 16-bit launch on dequantize_base_gptq4(...) holds: fp32 and 16-bit outputs bit for bit
    (the group sizes include G / 128 = 7 and 5 stages per group -- the multiply-high group index with a reciprocal that is not a power of
    two -- and one group over all of K)"""
    from bitdelta_amd.binary_gemm_kernel import binary_linear_decode, tile_weight
    p = make_problem(dtype, T, K, N, seed=5, G=G)
    wt = tile_weight(p.wdq)
    for kw in (dict(out_dtype=torch.float32), dict(), dict(residual=True)):
        kw4, kw16 = dict(kw), dict(kw)
        if kw.get("residual"):
            kw4["residual"], kw16["residual"] = p.res.clone(), p.res.clone()
        got = binary_linear_decode(p.x, p.w4, p.pk, p.a1, layout="packed", weight_tiled=True, group_params=p.gp, group_size=G, **kw4)
        want = binary_linear_decode(p.x, wt, p.pk, p.a1, layout="packed", weight_tiled=True, **kw16)
        assert torch.equal(got, want), (kw, first_difference(got, want))


def test_q4_envelope_is_refused_never_answered(bd):
    from bitdelta_amd._lib import BitDeltaHipError
    from bitdelta_amd.binary_gemm_kernel import binary_linear_decode
    from bitdelta_amd.quant import pack_gptq4_params
    refused = (BitDeltaHipError, AssertionError, ValueError)
    p = make_problem(torch.float16, 2, 2048, 1024)
    kw = dict(layout="packed")
    with pytest.raises(refused):                    # not tiled
        binary_linear_decode(p.x, p.qw.T.contiguous(), p.pk, p.a1, group_params=p.gp, **kw)
    with pytest.raises(refused):                    # missing parameters
        binary_linear_decode(p.x, p.w4, p.pk, p.a1, weight_tiled=True, **kw)
    with pytest.raises(refused):                    # parameters on a 16-bit weight
        binary_linear_decode(p.x, p.wdq, p.pk, p.a1, group_params=p.gp, **kw)
    x2 = torch.zeros(2, 2, 2048, device="cuda", dtype=torch.float16)
    with pytest.raises(refused):                    # M > 1
        binary_linear_decode(x2, p.w4, p.pk, p.a1, weight_tiled=True, group_params=p.gp, **kw)
    with pytest.raises(refused):                    # G = 64
        g = torch.Generator(device="cuda").manual_seed(1)
        _, qz, sc = random_checkpoint(1024, 2048, 64, g)
        binary_linear_decode(p.x, p.w4, p.pk, p.a1, weight_tiled=True, group_params=pack_gptq4_params(qz, sc), group_size=64, **kw)
    with pytest.raises(refused):                    # fp32 activations
        binary_linear_decode(p.x.float(), p.w4, p.pk, p.a1, weight_tiled=True, group_params=p.gp, **kw)
    with pytest.raises(refused):                    # N below the streaming kernel's minimum
        q = make_problem(torch.float16, 2, 2048, 256)
        binary_linear_decode(q.x, q.w4, q.pk, q.a1, weight_tiled=True, group_params=q.gp, **kw)
    with pytest.raises(refused):                    # the norm prologue outside its envelope (K not a power of two)
        q = make_problem(torch.float16, 2, 3072, 1024)
        binary_linear_decode(q.x, q.w4, q.pk, q.a1, weight_tiled=True, group_params=q.gp, norm_weight=q.nw, **kw)


# ------------------------------------------------------------------------------------------------------------------ decoder level
def untile_q4(t):
    """decode copy [N, K/8] -> qweight [K/8, N] (nibbles back in GPTQ's order)"""
    N, K8 = t.shape
    K = K8 * 8
    dw = t.view(N // 16, K // 128, 16, 4, 4).permute(1, 4, 3, 0, 2).reshape(K // 8, N)          # [it, s, g | tile, c]
    out = torch.zeros_like(dw)
    for pos, e in enumerate((0, 2, 4, 6, 1, 3, 5, 7)):
        out |= ((dw >> (4 * pos)) & 15) << (4 * e)
    return out


def test_q4_decoder_module_state(bd):
    from bitdelta_amd.quant import dequantize_base_gptq4, pack_gptq4_params, quantize_base_gptq4
    from bitdelta_amd.serving_loop import FusedDeltaLinear, TenantDecoder
    d16 = TenantDecoder.synthetic("tiny4096", 2, "cuda", dtype=torch.float16, seed=3, layers=1, shared_heads=True)
    d4 = TenantDecoder.synthetic("tiny4096", 2, "cuda", dtype=torch.float16, seed=3, layers=1, shared_heads=True, base_gptq4=True)
    assert d4.base_gptq4 and not d4.base_int8 and not d16.base_gptq4
    for name in ("qkv", "o", "gate_up", "down"):
        a, b = getattr(d16.layers[0], name), getattr(d4.layers[0], name)
        qw, qz, sc = quantize_base_gptq4(a.weight, 128)
        N, K = a.weight.shape
        assert b.base_gptq4 and not a.base_gptq4 and a.group_params is None and b.wscale is None
        assert torch.equal(b.weight, dequantize_base_gptq4(qw, qz, sc, torch.float16)), "the 16-bit buffer is the reference-dequantised weight"
        assert b.weight_tiled.dtype == torch.int32 and torch.equal(untile_q4(b.weight_tiled), qw)
        assert torch.equal(b.group_params, pack_gptq4_params(qz, sc))
        assert torch.equal(a.mask, b.mask)
        assert b.linear_bytes() == N * K // 2 + (K // 128) * N * 4 + a.mask.numel() * 4
    assert d4.lm_head.dtype == torch.float16
    # a checkpoint-supplied triple gives the same module as quantising the dequantised weight's source
    fl = d16.layers[0].qkv
    parts = list(fl.weight.split(fl.widths, 0))
    masks = list(fl.mask.split(fl.widths, 2))
    coeffs = [fl.alpha[:, :1].reshape(-1).clone() for _ in parts]
    quantised = FusedDeltaLinear(parts, masks, coeffs, base_gptq4=True)
    triples = [quantize_base_gptq4(w, 128) for w in parts]
    supplied = FusedDeltaLinear.from_gptq4(triples, masks, coeffs, dtype=torch.float16)
    for buf in ("weight", "weight_tiled", "group_params", "mask_packed", "alpha"):
        assert torch.equal(getattr(quantised, buf), getattr(supplied, buf)), buf
    x = torch.randn(2, 1, parts[0].shape[1], device="cuda").half()
    assert torch.equal(quantised(x), supplied(x))


def test_q4_decoder_logits_match_the_dense_twin_and_prefill_continues(bd):
    """prefill (16-bit kernels on the dequantised weight) then one 4-bit decode step from the same cache, against the dense fp32 twin of
    test_gpu_serving on the module's own `weight` -- which IS what the 4-bit launches compute on -- at the existing bound"""
    from test_gpu_serving import _dense_reference_logits, relerr
    from bitdelta_amd.serving_loop import TenantDecoder
    T = 6
    dec = TenantDecoder.synthetic("mistral-1layer", T, "cuda", dtype=torch.float16, seed=21, max_len=128, base_gptq4=True)
    g = torch.Generator().manual_seed(2)
    prompts = [torch.randint(1, 512, (n,), generator=g).tolist() for n in (9, 64, 33, 50, 17, 60)]
    ids, am = dec.prepare(prompts)
    cache = dec.new_cache()
    lg = dec.prefill(ids, am, cache)
    tok = torch.argmax(lg, dim=-1)
    pos = torch.tensor([ids.shape[1]], device="cuda")
    cache["valid"].index_fill_(1, pos, True)
    step = dec.forward(tok[:, None], pos, cache, cache["valid"][:, None, None, :]).float()
    assert step.shape[0] == T and bool(torch.isfinite(step).all())
    for t in range(T):
        seq = torch.cat([ids[t], tok[t:t + 1]])
        msk = torch.cat([am[t], torch.tensor([True], device="cuda")])
        ref = _dense_reference_logits(bd, dec, t, seq, msk)
        assert relerr(step[t], ref) <= 3e-3, (t, relerr(step[t], ref))


def test_q4_decoder_graph_replay_equals_eager_over_33_steps(bd):
    from bitdelta_amd.serving_loop import TenantDecoder
    for T, dtype in ((6, torch.float16), (1, torch.bfloat16)):
        dec = TenantDecoder.synthetic("tiny4096", T, "cuda", dtype=dtype, seed=11, max_len=128, shared_heads=True, base_gptq4=True)
        prompts = [[(7 * t + 3 * i) % 500 + 1 for i in range(5 + t)] for t in range(T)]
        tg, n = dec.generate(prompts, max_new_tokens=33, use_graph=True)
        te, ne = dec.generate(prompts, max_new_tokens=33, use_graph=False)
        assert n == ne == 33 and torch.equal(tg, te)


def test_q4_norm_handoff_token_level_agreement_over_33_greedy_steps(bd):
    """the int8 test of the same name (test_gpu_w8_decode.py), on the 4-bit base: the hand-off decoder teacher-forced on the separate-launch
    decoder's tokens; same bounds"""
    from test_gpu_serving import relerr
    from bitdelta_amd.serving_loop import TenantDecoder
    T, steps = 6, 33
    dec = TenantDecoder.synthetic((4096, 14336, 2, 32, 8, 512), T, "cuda", dtype=torch.float16, seed=31, max_len=128, base_gptq4=True)
    g = torch.Generator().manual_seed(3)
    prompts = [torch.randint(1, 512, (n,), generator=g).tolist() for n in (9, 64, 33, 50, 17, 60)]
    ids, am = dec.prepare(prompts)
    L = ids.shape[1]

    def run(flag, forced=None):
        dec.norm_handoff = flag
        cache = dec.new_cache()
        lg = dec.prefill(ids, am, cache)
        logits, toks = [lg.float()], []
        for s_ in range(steps):
            tok = forced[s_] if forced is not None else torch.argmax(logits[-1], dim=-1)
            toks.append(tok)
            pos = torch.tensor([L + s_], device="cuda")
            cache["valid"].index_fill_(1, pos, True)
            logits.append(dec.forward(tok[:, None], pos, cache, cache["valid"][:, None, None, :]).float())
        return logits, toks
    l_off, t_off = run(False)
    l_on, _ = run(True, forced=t_off)
    n_tie = 0
    for s_ in range(1, steps + 1):
        a, b = l_off[s_], l_on[s_]
        assert relerr(b, a) <= 4e-3, (s_, relerr(b, a))
        top2 = a.topk(2, dim=-1).values
        margin = top2[:, 0] - top2[:, 1]
        same = a.argmax(-1) == b.argmax(-1)
        near_tie = margin <= 4e-3 * top2[:, 0].abs().clamp_min(1.0)
        assert bool((same | near_tie).all()), (s_, margin.tolist(), same.tolist())
        n_tie += int((~same).sum())
    assert n_tie <= 2
    assert torch.equal(l_off[0], l_on[0])
