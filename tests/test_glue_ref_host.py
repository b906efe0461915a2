"""CPU-only checks of tests/glue_ref.py, the fp64 models and the acceptance rule tests/test_gpu_glue_exact.py holds the RMSNorm / SwiGLU / RoPE
kernels to: round16 on every 16-bit pattern, on every exact midpoint and one float64 step either side of it; the models against torch's CPU ops in
HF's order and against serving_loop._rope / _rope_tables; and the rule's power to discriminate -- an fp32 emulation of the kernels' arithmetic
passes accept(), the same emulation with eps dropped, the intermediate rounding skipped, the weight multiplied before the rounding, or the mean
taken over H rounded up to 2048 fails it, on the very inputs the GPU test uses.  The last test is what keeps the rule from being loosened
unnoticed."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import glue_ref as ref

DTYPES = [torch.float16, torch.bfloat16]


def _all_patterns(dtype):
    bits = np.arange(65536)
    return bits, ref.to64(ref.from_bits(bits, dtype))


# ------------------------------------------------------------------------------------------------------------------------ round16 / ulp16
@pytest.mark.parametrize("dtype", DTYPES)
def test_round16_round_trips_every_pattern(dtype):
    bits, v = _all_patterns(dtype)
    r = ref.round16(v, dtype)
    finite = np.isfinite(v)
    assert np.array_equal(np.isnan(r), np.isnan(v)) and np.array_equal(r[~np.isnan(v)], v[~np.isnan(v)])
    assert np.array_equal(np.signbit(r[finite]), np.signbit(v[finite]))                  # -0 stays -0
    assert np.array_equal(ref.bits16(v, dtype)[~np.isnan(v)], bits[~np.isnan(v)])        # ... and every value maps back to its own pattern


@pytest.mark.parametrize("dtype", DTYPES)
def test_round16_midpoints_go_to_even_and_their_float64_neighbours_to_the_nearer_value(dtype):
    """every pair of neighbouring non-negative values (subnormals, the subnormal / normal seam and the largest finite value | 2^(emax+1) pair
    included), both signs: the exact midpoint goes to the even pattern; the float64 next below it to the lower value, the next above to the upper.
    In float32 those two neighbours ARE the midpoint (it has at most 12 significant bits), so a rounding that passes through float32 fails here."""
    mbits, emin, emax = ref._FORMAT[dtype]
    inf_bits = (emax - emin + 2) << mbits
    lo_bits = np.arange(inf_bits)
    lo = ref.to64(ref.from_bits(lo_bits, dtype))
    hi = np.append(lo[1:], np.ldexp(1.0, emax + 1))                                      # past the largest finite value: where inf begins
    mid = (lo + hi) / 2                                                                  # exact: both have <= 11 significant bits
    below, above = np.nextafter(mid, -np.inf), np.nextafter(mid, np.inf)
    assert (below > lo).all() and (above < hi).all() and (below < mid).all() and (above > mid).all()
    f32_ok = mid >= 2.0 ** -126                                                          # (float32 normal range: where the collapse is certain)
    assert f32_ok.sum() > 0.9 * len(mid) or dtype == torch.bfloat16
    assert np.array_equal(below[f32_ok].astype(np.float32), mid[f32_ok].astype(np.float32))
    assert np.array_equal(above[f32_ok].astype(np.float32), mid[f32_ok].astype(np.float32))
    hi_v = np.append(lo[1:], np.inf)
    even = np.where(lo_bits % 2 == 0, lo, hi_v)
    for s in (1.0, -1.0):
        assert np.array_equal(ref.round16(s * mid, dtype), s * even)
        assert np.array_equal(ref.round16(s * below, dtype), s * lo)
        assert np.array_equal(ref.round16(s * above, dtype), s * hi_v)
    # overflow and the far ends
    assert ref.round16(np.array(1e300), dtype) == np.inf and ref.round16(np.array(-1e300), dtype) == -np.inf
    tiny = ref.round16(np.array([1e-300, -1e-300, 5e-324]), dtype)
    assert np.array_equal(tiny, [0.0, -0.0, 0.0]) and np.array_equal(np.signbit(tiny), [False, True, False])
    assert np.isnan(ref.round16(np.array(np.nan), dtype)) and ref.round16(np.array(-np.inf), dtype) == -np.inf


def test_round16_does_not_round_twice():
    """1 + 2^-8 + 2^-30 lies above the midpoint of the bf16 neighbours 1 and 1 + 2^-7: it rounds up.  Through float32 it first becomes the midpoint
    and then goes to the even side, 1."""
    v = 1 + 2.0 ** -8 + 2.0 ** -30
    assert ref.round16(np.array(v), torch.bfloat16) == 1 + 2.0 ** -7
    assert float(np.float32(v)) == 1 + 2.0 ** -8


@pytest.mark.parametrize("dtype", DTYPES)
def test_ulp16_is_the_gap_to_the_next_value(dtype):
    mbits, emin, emax = ref._FORMAT[dtype]
    lo = ref.to64(ref.from_bits(np.arange(((emax - emin + 2) << mbits)), dtype))         # 0 .. the largest finite value
    gap = np.diff(lo)
    assert np.array_equal(ref.ulp16(lo[:-1], dtype), gap) and np.array_equal(ref.ulp16(-lo[:-1], dtype), gap)
    assert ref.ulp16(np.array(0.0), dtype) == np.ldexp(1.0, emin - mbits)                # the subnormal quantum
    assert ref.ulp16(np.array(1.0), dtype) == 2.0 ** -mbits and ref.ulp16(np.array(1.5), dtype) == 2.0 ** -mbits
    assert np.isnan(ref.ulp16(np.array(np.nan), dtype)) and ref.ulp16(np.array(np.inf), dtype) == np.ldexp(1.0, emax - mbits)


def test_accept_semantics():
    dt = torch.float16
    model = np.array([1.0, -0.0, np.nan, 2.0, 1e-7, np.inf])
    one = np.ones(6)
    same = torch.tensor([1.0, 0.0, float("nan"), 2.0, 1e-7, float("inf")], dtype=dt)
    model[4] = float(same[4])
    v = ref.accept(same, model, model, one, dt, 1, 1.0)
    assert v.ok and v.worst_ulp == 0 and v.equal_share == 1.0 and v.first_bad == -1           # NaN matches NaN, -0 equals +0
    for i, val in ((2, 1.0), (0, float("nan"))):                                             # NaN against a number, either way round: never
        t = same.clone()
        t[i] = val
        v = ref.accept(t, model, model, one, dt, 10 ** 6, 0.0)
        assert not v.ok and v.first_bad == i and v.n_bad == 1
    t = same.clone()
    t[3] = 2.0 + 2 * 2.0 ** -9                                                              # two ulps of 2.0
    assert ref.accept(t, model, model, one, dt, 2, 0.8).ok and ref.accept(t, model, model, one, dt, 2, 0.8).worst_ulp == 2
    assert not ref.accept(t, model, model, one, dt, 2, 0.9).ok                              # the share: 5 of 6 are equal
    # one ulp is no longer within the derived band of an ordinary value (band = ulp(inter) |mult| + ulp(model) = 2 ulps there) ...
    v = ref.accept(t, model, np.full(6, 2.0), one, dt, 1, 0.0)
    assert v.ok
    t[3] = 2.0 + 3 * 2.0 ** -9
    assert not ref.accept(t, model, np.full(6, 2.0), one, dt, 1, 0.0).ok
    # ... the band matters where the intermediate is subnormal: inter = 3 * 2^-24 times mult = 1000 is 1.79e-4; inter one quantum away moves the
    # product by 1000 * 2^-24 = 6e-5, hundreds of ulps of the result
    inter, mult = np.array([3 * 2.0 ** -24]), np.array([1000.0])
    m = ref.round16(inter * mult, dt)
    got = torch.tensor(ref.round16(4 * 2.0 ** -24 * mult, dt), dtype=dt)
    v = ref.accept(got, m, inter, mult, dt, 2, 0.0)
    assert v.ok and v.worst_ulp > 100
    assert not ref.accept(torch.tensor(ref.round16(6 * 2.0 ** -24 * mult, dt), dtype=dt), m, inter, mult, dt, 2, 0.0).ok


# ------------------------------------------------------------------------------------------------------------------------ the models against torch
def _hf_norm(x, w, eps, rows_per_tenant):
    v = x.float()
    wr = w[torch.arange(x.shape[0]) // rows_per_tenant]
    return (v * torch.rsqrt(v.pow(2).mean(-1, True) + eps)).to(x.dtype) * wr


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("H", [264, 2056, 4096])
def test_norm_model_against_torch_in_hf_order(dtype, H):
    x, w, classes = ref.norm_inputs(dtype, H, ref.NORM_BLOCK_ROWS)
    for eps in ref.NORM_EPS:
        want, a = ref.rmsnorm(ref.to64(x), ref.to64(w), eps, 7, dtype)
        v = ref.accept(_hf_norm(x, w, eps, 7), want, a, ref.to64(w)[np.arange(len(classes)) // 7], dtype, *ref.NORM_LIMITS)
        assert v.ok, (H, eps, v)
        # what the model says about the special rows: zeros stay exact zeros, a NaN takes its whole row, an inf leaves NaN in its place and zeros
        for r, c in enumerate(classes):
            if c == ref.ZERO_ROW:
                assert not want[r].any()
            elif c == ref.NAN_ROW:
                assert np.isnan(want[r]).all()
            elif c == ref.INF_ROW:
                assert np.isnan(want[r]).sum() == 1 and not np.nan_to_num(want[r]).any()
            else:
                assert np.isfinite(want[r]).all() and want[r].any()


@pytest.mark.parametrize("dtype", DTYPES)
def test_add_norm_model_against_torch(dtype):
    H = 264
    resid, w, classes = ref.norm_inputs(dtype, H, ref.NORM_BLOCK_ROWS)
    y32 = ref.add_norm_y32(resid, classes)
    x_t = resid + y32.to(dtype)
    x, h, a = ref.add_rmsnorm(ref.to64(resid), ref.to64(y32), ref.to64(w), 1e-5, 7, dtype)
    v = ref.accept(x_t, x, x, np.ones(1), dtype, 1, 0.999)
    assert v.ok, v
    v = ref.accept(_hf_norm(x_t, w, 1e-5, 7), ref.rmsnorm(ref.to64(x_t), ref.to64(w), 1e-5, 7, dtype)[0], a, ref.to64(w)[np.arange(len(classes)) // 7],
                   dtype, *ref.NORM_LIMITS)
    assert v.ok, v


@pytest.mark.parametrize("dtype", DTYPES)
def test_swiglu_model_against_torch(dtype):
    g, u = ref.swiglu_exhaustive_inputs(dtype)
    assert g.shape[1] % 8 == 0 and g.shape[1] >= (43522 if dtype == torch.float16 else 34114)
    want, a = ref.swiglu(ref.to64(g), ref.to64(u), dtype)
    v = ref.accept(F.silu(g) * u, want, a, ref.to64(u), dtype, *ref.SWIGLU_LIMITS)
    assert v.ok, v


@pytest.mark.parametrize("dtype", DTYPES)
def test_rope_model_and_tables_against_serving_loop(dtype):
    from bitdelta_amd.serving_loop import _rope, _rope_tables
    L = 256
    cos16, sin16 = _rope_tables(L, 128, "cpu", dtype)
    cos, sin, ang = ref.rope_tables(L)
    pos = np.arange(L)[:, None]
    for table, model in ((cos16, cos), (sin16, sin)):
        # _rope_tables forms the angle as a float32 product, as HF does: its error is at most 3 * 2^-24 * angle <= pos * 2^-22
        assert (np.abs(ref.to64(table) - model) <= 0.5 * ref.ulp16(model, dtype) + pos * 2.0 ** -22).all()
    clear = np.abs(np.sin(ang)) > 2.0 ** -6
    assert clear.mean() > 0.4
    s16 = ref.to64(sin16)
    assert (np.sign(s16[:, :64])[clear[:, :64]] == -np.sign(np.sin(ang[:, :64]))[clear[:, :64]]).all()
    assert (np.sign(s16[:, 64:])[clear[:, 64:]] == np.sign(np.sin(ang[:, 64:]))[clear[:, 64:]]).all()
    # the rotation: x [T, heads, S, 128] in serving_loop's layout, positions 0 .. S - 1
    g = torch.Generator().manual_seed(11)
    x = torch.randn(2, 5, L, 128, generator=g).to(dtype)
    got = _rope(x, cos16, sin16)
    rows = ref.to64(x).transpose(0, 2, 1, 3).reshape(2 * L, 5, 128)                       # [T * S, heads, 128]
    want, inter = ref.rope(rows, ref.to64(cos16), ref.to64(sin16), np.tile(np.arange(L), 2), dtype)
    v = ref.accept(got.permute(0, 2, 1, 3).reshape(2 * L, 5, 128), want, inter, np.ones(1), dtype, *ref.ROPE_LIMITS)
    assert v.ok, v


@pytest.mark.parametrize("dtype", DTYPES)
def test_rotation_invariant_holds_for_the_model_and_breaks_for_a_wrong_sign_or_pairing(dtype):
    from bitdelta_amd.serving_loop import _rope_tables
    cos16, sin16 = (ref.to64(t) for t in _rope_tables(256, 128, "cpu", dtype))
    vec = ref.to64(torch.randn(128, generator=torch.Generator().manual_seed(5)).to(dtype))
    rows = np.broadcast_to(vec, (256, 1, 128))
    out, _ = ref.rope(rows, cos16, sin16, np.arange(256), dtype)
    spread, tol = ref.rotation_spread(out[:, 0], ref.ROTATION_PAIRS, dtype)
    assert spread <= tol, (spread, tol)
    flipped, _ = ref.rope(rows, cos16, np.abs(sin16), np.arange(256), dtype)               # the rotate-half sign lost
    spread, tol = ref.rotation_spread(flipped[:, 0], ref.ROTATION_PAIRS, dtype)
    assert spread > 10 * tol, (spread, tol)
    with np.errstate(all="ignore"):                                                        # partners 32 apart instead of 64
        wrong = ref.round16(ref.round16(rows * cos16[:, None], dtype) + np.roll(rows, 32, -1) * sin16[:, None], dtype)
    spread, tol = ref.rotation_spread(wrong[:, 0], ref.ROTATION_PAIRS, dtype)
    assert spread > 10 * tol, (spread, tol)


# ------------------------------------------------------------------------------------------------------------------------ the rule discriminates
def _f32(a):
    return np.asarray(a, dtype=np.float32)


def emulate_norm(x16, w16, eps, rows_per_tenant, dtype, mutant=None):
    """the kernels' RMSNorm arithmetic in float32 numpy (the order of the sum is numpy's); mutant: None, "no_eps", "no_round", "w_first", "h2048" """
    x = x16.float().numpy()
    rows, H = x.shape
    w = w16.float().numpy()[np.arange(rows) // rows_per_tenant]
    with np.errstate(all="ignore"):
        ss = (x * x).sum(-1, keepdims=True, dtype=np.float32)
        Hd = np.float32(-(-H // 2048) * 2048 if mutant == "h2048" else H)
        rs = _f32(np.float32(1) / np.sqrt(_f32(ss / Hd) + np.float32(0 if mutant == "no_eps" else eps)))
        if mutant == "no_round":
            y = _f32(x * rs) * w
        elif mutant == "w_first":
            y = _f32(ref.round16(np.float64(_f32(x * w)), dtype)) * rs
        else:
            y = _f32(ref.round16(np.float64(_f32(x * rs)), dtype)) * w
        return ref.from_bits(ref.bits16(np.float64(_f32(y)), dtype), dtype)


def emulate_swiglu(g16, u16, dtype, mutant=None):
    g, u = g16.float().numpy(), u16.float().numpy()
    with np.errstate(all="ignore"):
        a = _f32(g / _f32(np.float32(1) + np.exp(-g, dtype=np.float32)))
        if mutant != "no_round":
            a = _f32(ref.round16(np.float64(a), dtype))
        return ref.from_bits(ref.bits16(np.float64(_f32(a * u)), dtype), dtype)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("H,rows", [(H, ref.NORM_BLOCK_ROWS) for H in ref.NORM_BLOCK_H] + [(4096, ref.NORM_WAVE_ROWS)])
def test_accept_passes_the_fp32_norm_and_fails_each_mutant(dtype, H, rows):
    x, w, classes = ref.norm_inputs(dtype, H, rows)
    rpt = rows // ref.NORM_TENANTS
    wr = ref.to64(w)[np.arange(rows) // rpt]
    for eps in ref.NORM_EPS:
        want, a = ref.rmsnorm(ref.to64(x), ref.to64(w), eps, rpt, dtype)
        v = ref.accept(emulate_norm(x, w, eps, rpt, dtype), want, a, wr, dtype, *ref.NORM_LIMITS)
        assert v.ok, (H, eps, v)
        for mutant in ("no_eps", "no_round", "w_first", "h2048"):
            if mutant == "h2048" and H % 2048 == 0:
                continue                                        # (H is its own multiple of 2048: not a mutant there)
            v = ref.accept(emulate_norm(x, w, eps, rpt, dtype, mutant), want, a, wr, dtype, *ref.NORM_LIMITS)
            assert not v.ok, (mutant, H, eps, v)


@pytest.mark.parametrize("dtype", DTYPES)
def test_accept_passes_the_fp32_swiglu_and_fails_the_unrounded_one(dtype):
    g, u = ref.swiglu_exhaustive_inputs(dtype)
    want, a = ref.swiglu(ref.to64(g), ref.to64(u), dtype)
    v = ref.accept(emulate_swiglu(g, u, dtype), want, a, ref.to64(u), dtype, *ref.SWIGLU_LIMITS)
    assert v.ok, v
    v = ref.accept(emulate_swiglu(g, u, dtype, "no_round"), want, a, ref.to64(u), dtype, *ref.SWIGLU_LIMITS)
    assert not v.ok, v
