"""The decode Linear with an INT8 base weight (bd_binary_linear_decode_w8; gemv_stream_kernel WT = 2) on the device.

    Y[t, n] = round( wscale[n] * sum_k X[t,k] CB[n,k]  +  alpha[t, g(n)] * sum_k X[t,k] S_t[k,n]  [+ residual] ),   wscale = SCB / 127

The format is the one the reference dequantises in bitdelta/misc.py:72-73; its `dequantize_8bit` is a closure of a function that imports
bitsandbytes, so no reference-generated fixture exists: the checkers are that one line restated (quant.dequantize_base_int8, pinned in
test_w8_host.py) and an fp64 evaluation of the formula above that uses no kernel under test (test_gpu_decode_forms.fp64_parts).
Mirrors test_gpu_decode_forms.run_matrix: every launch kind x every product flag set, each bit-identical to its flag-0 result, the fused
prologue / epilogue bit-identical to the separate launches, canaries, bd_last_decode_form(); then flag 0 against fp64 under the 16-bit path's
own gates, and against the reference route (dequantise to 16 bits, run the 16-bit kernel)."""
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


@pytest.fixture(scope="module")
def bd():
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    import bitdelta_amd
    from bitdelta_amd import _lib
    _lib.lib()
    return bitdelta_amd


def make_problem(dtype, T, K, N, seed=0):
    from bitdelta_amd.binary_gemm_kernel import pack_decode_masks
    from bitdelta_amd.quant import quantize_base_int8, tile_weight_int8, weight_scale
    g = torch.Generator(device="cuda").manual_seed(seed + 7 * K + N + T)
    p = types.SimpleNamespace(T=T, K=K, N=N, dtype=dtype)
    p.x = (torch.randn(T, 1, K, device="cuda", generator=g) * 1.5).to(dtype)
    w = (torch.randn(N, K, device="cuda", generator=g) * 0.02).to(dtype)
    w *= (0.25 + 1.5 * torch.rand(N, 1, device="cuda", generator=g)).to(dtype)           # row scales that differ: a misplaced wscale[n] shows
    p.cb, p.scb = quantize_base_int8(w)
    p.ws = weight_scale(p.scb)
    p.w8 = tile_weight_int8(p.cb)
    p.mask = torch.randint(-2**31, 2**31 - 1, (T, K // 32, N), device="cuda", generator=g, dtype=torch.int64).to(torch.int32)
    p.alpha = torch.rand(T, 2, device="cuda", generator=g) * 1e-3 + 2e-4
    p.a1 = p.alpha[:, :1].contiguous()
    p.res = torch.randn(T, 1, N, device="cuda", generator=g).to(dtype)
    p.nw = (1 + 0.1 * torch.randn(T, K, device="cuda", generator=g)).to(dtype)
    p.nwn = (1 + 0.1 * torch.randn(T, N, device="cuda", generator=g)).to(dtype)
    p.pk = pack_decode_masks(p.mask)
    return p


def run_matrix(dtype, T, K, N, seed=0):
    """Every launch kind of the int8 base under every flag set for one shape.  Returns (flag-0 outputs, problems, the problem's tensors)."""
    from bitdelta_amd import _lib
    from bitdelta_amd import serving_ops as ops
    from bitdelta_amd.binary_gemm_kernel import binary_linear_decode, fused_norm_ok, handoff_ok
    L = _lib.lib()
    C = num_cus()
    tiles = N // 16
    p = make_problem(dtype, T, K, N, seed)
    x, a1, alpha, res, nw, nwn = p.x, p.a1, p.alpha, p.res, p.nw, p.nwn
    a8 = alpha.repeat(1, N // 16).contiguous()
    xs_buf = torch.full((T, 1, K + 128), 1.0e4, device="cuda").to(dtype)
    xs_buf[..., :K] = x
    xs = xs_buf[..., :K]
    xw_in = (x.float() * nw.float()[:, None, :]).to(dtype)
    ssq_in = torch.zeros(K // 16, 16, device="cuda")
    ssq_in[:, :T] = (x.float()[:, 0].reshape(T, K // 16, 16) ** 2).sum(-1).T

    def lin(xin, al, **kw):
        return binary_linear_decode(xin, p.w8, p.pk, al, layout="packed", weight_tiled=True, weight_scale=p.ws, **kw)

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

    # ---- flag 0 against fp64 of the formula: exact CB (integers), exact wscale as fp32, fp64 everywhere else
    x64 = x.double()[:, 0]
    xn = torch.stack([x64, rmsnorm64(x64, nw), rmsnorm64(x64, nw[:1])])
    base, delta = fp64_parts(xn, p.cb, p.mask)                        # base = xs . CB^T (CB.double(): exact)
    base = base * p.ws.double()
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
    pytest.param(1, 4096, C1, id="T1-tiles=C+1-fine-grid"),
    pytest.param(3, 4096, C1, id="T3-tiles=C+1-fine-grid"),
    pytest.param(6, 4096, C1, id="T6-tiles=C+1-fine-grid"),
    pytest.param(8, 4096, C1, id="T8-tiles=C+1-tpad8-no-fine-grid"),
    pytest.param(6, 4096, ("C", 1, 0), id="T6-tiles=C"),
    pytest.param(3, 4096, ("C", 2, 0), id="T3-tiles=2C"),
    pytest.param(6, 4096, ("C", 2, 1), id="T6-tiles=2C+1-not-eligible"),
    pytest.param(1, 4096, ("C", 2, 1), id="T1-tiles=2C+1-not-eligible"),
    pytest.param(6, 4096, 6144, id="mistral-qkv"),
    pytest.param(6, 14336, 4096, id="mistral-down-per-stage-rows"),
    pytest.param(6, 4096, 2 * 14336, id="mistral-gate-up-7-tiles-per-block"),
    pytest.param(3, 1024, ("C", 9, 0), id="9-tiles-per-block-scale-load-in-epilogue"),
    pytest.param(8, 1152, C1, id="K1152-empty-wave"),
    pytest.param(1, 1024, 512, id="smallest"),
]


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], ids=["fp16", "bf16"])
@pytest.mark.parametrize("T,K,Nspec", SHAPES)
def test_w8_decode_forms_match_fp64_and_each_other_under_every_flag(bd, dtype, T, K, Nspec):
    N = _resolve_n(Nspec)
    _, problems, _, _ = run_matrix(dtype, T, K, N)
    assert not problems, f"{len(problems)} problems (T = {T}, K = {K}, N = {N}, C = {num_cus()}):\n" + "\n".join(problems[:40])


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], ids=["fp16", "bf16"])
@pytest.mark.parametrize("T,K,N", [(1, 4096, 4096), (6, 4096, 6144), (3, 14336, 4096), (8, 2048, 1024)])
def test_w8_is_no_further_from_fp64_than_the_reference_route(bd, dtype, T, K, N):
    """fp32 outputs: the int8 launch rounds no weight, the reference route (dequantise to 16 bits -- misc.py:72-73 -- then the 16-bit kernel)
    rounds every one, so the new path's error to the fp64 value of the formula is no larger.  Derived; no margin."""
    from bitdelta_amd.binary_gemm_kernel import binary_linear_decode, tile_weight
    from bitdelta_amd.quant import dequantize_base_int8
    p = make_problem(dtype, T, K, N, seed=5)
    base, delta = fp64_parts(p.x.double()[None, :, 0], p.cb, p.mask)
    ref = (base * p.ws.double() + p.a1.double() * delta)[0]
    got = binary_linear_decode(p.x, p.w8, p.pk, p.a1, layout="packed", weight_tiled=True, weight_scale=p.ws, out_dtype=torch.float32)[:, 0]
    wd = dequantize_base_int8(p.cb, p.scb, dtype)
    route = binary_linear_decode(p.x, tile_weight(wd), p.pk, p.a1, layout="packed", weight_tiled=True, out_dtype=torch.float32)[:, 0]
    e_new, e_route = rel(got, ref), rel(route, ref)
    assert e_new <= e_route, f"int8 path rel {e_new:.3e} > reference route rel {e_route:.3e}"
    assert e_new <= 1e-5, e_new


def test_w8_envelope_is_refused_never_answered(bd):
    from bitdelta_amd._lib import BitDeltaHipError
    from bitdelta_amd.binary_gemm_kernel import binary_linear_decode
    refused = (BitDeltaHipError, AssertionError, ValueError)
    p = make_problem(torch.float16, 2, 2048, 1024)
    kw = dict(layout="packed")
    with pytest.raises(refused):                    # row-major int8
        binary_linear_decode(p.x, p.cb, p.pk, p.a1, weight_scale=p.ws, **kw)
    with pytest.raises(refused):                    # missing scale
        binary_linear_decode(p.x, p.w8, p.pk, p.a1, weight_tiled=True, **kw)
    with pytest.raises(refused):                    # a scale on a 16-bit weight
        binary_linear_decode(p.x, p.cb.half(), p.pk, p.a1, weight_scale=p.ws, **kw)
    x2 = torch.zeros(2, 2, 2048, device="cuda", dtype=torch.float16)
    with pytest.raises(refused):                    # M > 1
        binary_linear_decode(x2, p.w8, p.pk, p.a1, weight_tiled=True, weight_scale=p.ws, **kw)
    with pytest.raises(refused):                    # N below the streaming kernel's minimum
        q = make_problem(torch.float16, 2, 2048, 256)
        binary_linear_decode(q.x, q.w8, q.pk, q.a1, weight_tiled=True, weight_scale=q.ws, **kw)


# ------------------------------------------------------------------------------------------------------------------ decoder level
def untile_int8(t):
    N, K = t.shape
    return t.view(N // 16, K // 128, 2, 16, 4, 2, 8).permute(0, 3, 1, 2, 5, 4, 6).reshape(N, K)


def unrounded_twin(dec):
    """a view of `dec` whose delta Linears expose weight = CB * SCB / 127 in fp32 (NOT the fp16-rounded dequantised buffer): what the int8
    decode launches compute on"""
    def shim(fl):
        w = untile_int8(fl.weight_tiled).float() * fl.wscale[:, None]
        return types.SimpleNamespace(weight=w, mask=fl.mask, column_alpha=fl.column_alpha, split=fl.split)
    layers = [types.SimpleNamespace(qkv=shim(l.qkv), o=shim(l.o), gate_up=shim(l.gate_up), down=shim(l.down), norm1=l.norm1, norm2=l.norm2)
              for l in dec.layers]
    return types.SimpleNamespace(cfg=dec.cfg, hd=dec.hd, eps=dec.eps, cos=dec.cos, sin=dec.sin, embed=dec.embed, final_norm=dec.final_norm,
                                 lm_head=dec.lm_head, layers=layers)


def test_w8_decoder_module_state(bd):
    from bitdelta_amd.quant import dequantize_base_int8, quantize_base_int8
    from bitdelta_amd.serving_loop import TenantDecoder
    d16 = TenantDecoder.synthetic("tiny4096", 2, "cuda", dtype=torch.float16, seed=3, layers=1, shared_heads=True)
    d8 = TenantDecoder.synthetic("tiny4096", 2, "cuda", dtype=torch.float16, seed=3, layers=1, shared_heads=True, base_int8=True)
    for name in ("qkv", "o", "gate_up", "down"):
        a, b = getattr(d16.layers[0], name), getattr(d8.layers[0], name)
        cb, scb = quantize_base_int8(a.weight)
        assert b.base_int8 and not a.base_int8 and a.wscale is None
        assert torch.equal(b.weight, dequantize_base_int8(cb, scb, torch.float16)), "the 16-bit buffer is the reference-dequantised weight"
        assert b.weight_tiled.dtype == torch.int8 and torch.equal(untile_int8(b.weight_tiled), cb) and torch.equal(b.wscale, scb / 127)
        assert torch.equal(a.mask, b.mask)
        assert b.linear_bytes() == a.linear_bytes() - a.weight.numel()
    assert d8.lm_head.dtype == torch.float16


def test_w8_decoder_logits_match_the_unrounded_dense_twin_and_prefill_continues(bd):
    from test_gpu_serving import _dense_reference_logits, relerr
    from bitdelta_amd.serving_loop import TenantDecoder
    T = 6
    dec = TenantDecoder.synthetic("mistral-1layer", T, "cuda", dtype=torch.float16, seed=21, max_len=128, base_int8=True)
    g = torch.Generator().manual_seed(2)
    prompts = [torch.randint(1, 512, (n,), generator=g).tolist() for n in (9, 64, 33, 50, 17, 60)]
    ids, am = dec.prepare(prompts)
    cache = dec.new_cache()
    lg = dec.prefill(ids, am, cache)                     # 16-bit kernels on the dequantised weight
    tok = torch.argmax(lg, dim=-1)
    pos = torch.tensor([ids.shape[1]], device="cuda")
    cache["valid"].index_fill_(1, pos, True)
    step = dec.forward(tok[:, None], pos, cache, cache["valid"][:, None, None, :]).float()      # int8 decode from the same cache
    assert step.shape[0] == T and bool(torch.isfinite(step).all())
    twin = unrounded_twin(dec)
    for t in range(T):
        seq = torch.cat([ids[t], tok[t:t + 1]])
        msk = torch.cat([am[t], torch.tensor([True], device="cuda")])
        ref = _dense_reference_logits(bd, twin, t, seq, msk)
        assert relerr(step[t], ref) <= 3e-3, (t, relerr(step[t], ref))


def test_w8_decoder_graph_replay_equals_eager_over_33_steps(bd):
    from bitdelta_amd.serving_loop import TenantDecoder
    for T, dtype in ((6, torch.float16), (1, torch.bfloat16)):
        dec = TenantDecoder.synthetic("tiny4096", T, "cuda", dtype=dtype, seed=11, max_len=128, shared_heads=True, base_int8=True)
        prompts = [[(7 * t + 3 * i) % 500 + 1 for i in range(5 + t)] for t in range(T)]
        tg, n = dec.generate(prompts, max_new_tokens=33, use_graph=True)
        te, ne = dec.generate(prompts, max_new_tokens=33, use_graph=False)
        assert n == ne == 33 and torch.equal(tg, te)


def test_w8_norm_handoff_token_level_agreement_over_33_greedy_steps(bd):
    """the 16-bit test of the same name (test_gpu_serving.py), on the int8 base: the hand-off decoder teacher-forced on the separate-launch
    decoder's tokens; same bounds"""
    from test_gpu_serving import relerr
    from bitdelta_amd.serving_loop import TenantDecoder
    T, steps = 6, 33
    dec = TenantDecoder.synthetic((4096, 14336, 2, 32, 8, 512), T, "cuda", dtype=torch.float16, seed=31, max_len=128, base_int8=True)
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
