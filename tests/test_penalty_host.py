"""CPU-only checks of the penalty path: penalty_params accepts and refuses exactly what the session documents and is neutral by default; the
extend fold of a history row; the restatement (penalty_ref) on hand-made rows and its neutral case on +-0, +-inf, subnormals and the largest
finite values in both dtypes; the two C-ABI symbols in the header, the library, the ctypes table and INTEGRATION.md, with the argument checks
they answer before any device call."""
import ctypes
import math
import os
import re

import numpy as np
import pytest
import torch

import penalty_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
inf, nan = math.inf, math.nan
DTYPES = [torch.float16, torch.bfloat16]


# ------------------------------------------------------------------------------------------------ 1. penalty_params
def test_penalty_params_is_neutral_by_default_and_canonical():
    from bitdelta_amd.serving_loop import NEUTRAL, penalty_params, penalty_row
    assert penalty_params() == NEUTRAL == (1.0, 0.0, 0.0, ())
    assert penalty_params(1, 0, 0, {}) == NEUTRAL and penalty_params(np.float32(1.0), 0.0, -0.0, None) == NEUTRAL
    assert penalty_row(NEUTRAL) == [1.0, 1.0, 0.0, 0.0]
    got = penalty_params(1.1, -0.5, 2, {7: 1.5, np.int64(3): -inf, 500: -100, 0: 100.0}, vocab=512)
    assert got == (1.1, -0.5, 2.0, ((0, 100.0), (3, -inf), (7, 1.5), (500, -100.0)))                 # sorted by id, plain floats and ints
    assert all(type(i) is int and type(v) is float for i, v in got[3])
    assert penalty_params(logit_bias={5: 1, 2: 2}) == penalty_params(logit_bias={2: 2.0, 5: 1.0})
    assert penalty_row(got) == [1.1, 1.0 / 1.1, -0.5, 2.0]
    assert penalty_params(logit_bias={511: 0.0}, vocab=512)[3] == ((511, 0.0),)
    assert len(penalty_params(logit_bias={i: 1.0 for i in range(64)})[3]) == 64
    assert len(penalty_params(logit_bias={i: 1.0 for i in range(16)}, max_logit_bias=16)[3]) == 16


@pytest.mark.parametrize("kw", [
    dict(repetition_penalty=0.0), dict(repetition_penalty=-1.0), dict(repetition_penalty=inf), dict(repetition_penalty=nan),
    dict(repetition_penalty="x"), dict(repetition_penalty=None), dict(repetition_penalty=True),
    dict(presence_penalty=inf), dict(presence_penalty=nan), dict(presence_penalty=[1]), dict(frequency_penalty=-inf), dict(frequency_penalty=nan),
    dict(frequency_penalty=False),
    dict(logit_bias=[(1, 2.0)]), dict(logit_bias="12"), dict(logit_bias={1.5: 1.0}), dict(logit_bias={"1": 1.0}), dict(logit_bias={True: 1.0}),
    dict(logit_bias={-1: 1.0}), dict(logit_bias={512: 1.0}, vocab=512), dict(logit_bias={1: 100.5}), dict(logit_bias={1: -101}),
    dict(logit_bias={1: inf}), dict(logit_bias={1: nan}), dict(logit_bias={1: "a"}), dict(logit_bias={1: None}), dict(logit_bias={1: True}),
    dict(logit_bias={i: 1.0 for i in range(65)}), dict(logit_bias={i: 1.0 for i in range(17)}, max_logit_bias=16),
])
def test_penalty_params_refuses(kw):
    from bitdelta_amd.serving_loop import penalty_params
    with pytest.raises(ValueError):
        penalty_params(**kw)


# ------------------------------------------------------------------------------------------------ 2. the extend fold
def test_the_extend_fold_turns_everything_seen_into_context():
    from bitdelta_amd.serving_loop import fold_history
    h = ref.bits16(torch.tensor([0, 0x8000, 1, 0x8001, 32767, 0xffff, 0, 5]))
    before = h.clone()
    f = fold_history(h)
    assert f.dtype == torch.int16 and f.tolist() == [0, -32768, -32768, -32768, -32768, -32768, 0, -32768]
    assert torch.equal(h, before) and torch.equal(fold_history(f), f)                               # a new tensor; folding twice is folding once
    # what a submit of the whole conversation would have written: bit 15 at every token of prompt + generated
    prompt, generated = [3, 9, 9, 200], [9, 17, 17, 17]
    turn1 = ref.history(prompt, {9: 1, 17: 3}, V=256)
    assert torch.equal(fold_history(turn1), ref.history(prompt + generated, V=256))
    assert fold_history(torch.zeros(2, 8, dtype=torch.int16)).shape == (2, 8)


# ------------------------------------------------------------------------------------------------ 3. the restatement
def _pen(r=1.0, presence=0.0, frequency=0.0, r_inv=None):
    return torch.tensor([[r, 1.0 / r if r_inv is None else r_inv, presence, frequency]], dtype=torch.float32)


def test_restatement_on_a_hand_made_row():
    l = torch.tensor([[2.0, -2.0, 2.0, -2.0, 4.0, 4.0, 0.0, 1.0]], dtype=torch.float16)
    h = ref.bits16(torch.tensor([[0, 0, 0x8000, 0x8000, 2, 0x8003, 1, 0]]))
    out, h2 = ref.penalize(l, h, _pen(2.0, 0.25, 0.5))
    # unseen: untouched; context: / 2 or * 2; count 2: 4 / 2 - 0.5 * 2 - 0.25; bit 15 + count 3: 4 / 2 - 1.5 - 0.25; count 1 at 0: -0.5 - 0.25
    assert out[0].tolist() == [2.0, -2.0, 1.0, -4.0, 0.75, 0.25, -0.75, 1.0] and torch.equal(h2, h)
    # the step form counts the fed token first: element 7 (never seen) becomes count 1 and is seen; element 5 goes from 3 to 4
    out, h2 = ref.penalize(l, h, _pen(2.0, 0.25, 0.5), tok=torch.tensor([7]), active=torch.tensor([True]))
    assert out[0].tolist() == [2.0, -2.0, 1.0, -4.0, 0.75, 0.25, -0.75, 0.5 - 0.5 - 0.25] and (h2[0].int() & 0xffff).tolist() == [0, 0, 0x8000, 0x8000, 2, 0x8003, 1, 1]
    out, h2 = ref.penalize(l, h, _pen(2.0, 0.25, 0.5), tok=torch.tensor([5]), active=torch.tensor([True]))
    assert float(out[0, 5]) == 2.0 - 2.0 - 0.25 and (h2[0].int() & 0xffff).tolist() == [0, 0, 0x8000, 0x8000, 2, 0x8004, 1, 0]
    # saturation, with and without bit 15; an inactive row keeps hist and its previous output; a token out of range counts nothing
    hs = ref.bits16(torch.tensor([[32767, 0xffff, 32766, 0, 0, 0, 0, 0]]))
    for y, want in ((0, 32767), (1, 0xffff), (2, 32767)):
        assert int(ref.penalize(l, hs, _pen(), tok=torch.tensor([y]), active=torch.tensor([True]))[1][0, y]) & 0xffff == want
    prev = torch.full_like(l, 9.0)
    out, h2 = ref.penalize(l, hs, _pen(2.0), tok=torch.tensor([3]), active=torch.tensor([False]), out=prev)
    assert torch.equal(out, prev) and torch.equal(h2, hs)
    for y in (-1, 8, 2 ** 40):
        out, h2 = ref.penalize(l, hs, _pen(), tok=torch.tensor([y]), active=torch.tensor([True]))
        assert torch.equal(h2, hs) and ref.same_bits(out, l)
    # the bias list: list order, a repeated id twice, -1 and ids past V match nothing, -inf bans
    ids = torch.tensor([[1, 7, 1, -1, 8, 4]], dtype=torch.int32)
    vals = torch.tensor([[0.5, -inf, 0.25, 50.0, 50.0, 100.0]], dtype=torch.float32)
    out, _ = ref.penalize(l, torch.zeros_like(h), _pen(), ids, vals)
    assert out[0].tolist() == [2.0, -1.25, 2.0, -2.0, 104.0, 4.0, 0.0, -inf]
    # values the host could not have written: r not in (0, inf) turns the repetition step off, a NaN penalty counts as 0
    for r in (0.0, -2.0, inf, nan):
        out, _ = ref.penalize(l, h, torch.tensor([[r, 0.5, nan, nan]]))
        assert ref.same_bits(out, l), r
    # fp16 overflow by r: the rounding gives -inf (the product is finite in fp32)
    big = torch.tensor([[-60000.0] * 8], dtype=torch.float16)
    assert ref.penalize(big, torch.full((1, 8), ref.BIT15, dtype=torch.int16), _pen(2.0))[0].tolist() == [[-inf] * 8]
    # each operation is rounded on its own: x * r_inv with the host's float32 reciprocal, not a division
    x = torch.tensor([[3.0] * 8], dtype=torch.bfloat16)
    out, _ = ref.penalize(x, torch.full((1, 8), ref.BIT15, dtype=torch.int16), _pen(1.1))
    assert float(out[0, 0]) == float((torch.tensor(3.0) * torch.tensor(1.0 / 1.1, dtype=torch.float32)).to(torch.bfloat16))


@pytest.mark.parametrize("dtype", DTYPES, ids=["f16", "bf16"])
def test_neutral_parameters_return_the_input_bits(dtype):
    """every finite pattern next to 0 and next to the largest value, both signs, +-0, +-inf, the subnormals: bits in = bits out, whatever the
    history holds (x * 1, x - 0 * c and x - 0 are exact)"""
    top = 0x7c00 if dtype == torch.float16 else 0x7f80                                              # +inf; below it the finite patterns
    mags = list(range(0, 0x0410)) + list(range(top - 64, top + 1))
    pats = torch.tensor(mags + [m | 0x8000 for m in mags], dtype=torch.int32)
    pats = torch.cat([pats, pats.new_zeros((-pats.numel()) % 8)]).reshape(1, -1)
    l = ref.bits16(pats).view(dtype)
    V = l.shape[1]
    assert bool(torch.isinf(l).any()) and not bool(torch.isnan(l).any())
    g = torch.Generator().manual_seed(1)
    h = ref.bits16(torch.randint(0, 0x10000, (1, V), generator=g))
    from bitdelta_amd.serving_loop import NEUTRAL, penalty_row
    pen = torch.tensor([penalty_row(NEUTRAL)], dtype=torch.float32)
    for hist in (torch.zeros_like(h), h):
        out, h2 = ref.penalize(l, hist, pen)
        assert torch.equal(out.view(torch.int16), l.view(torch.int16)) and torch.equal(h2, hist)
        out, h2 = ref.penalize(l, hist, pen, torch.full((1, 4), -1, dtype=torch.int32), torch.ones(1, 4), tok=torch.tensor([5]),
                               active=torch.tensor([True]))
        assert torch.equal(out.view(torch.int16), l.view(torch.int16))
        assert int((h2 != hist).sum()) == (0 if int(hist[0, 5]) & 0x7fff == 0x7fff else 1)


# ------------------------------------------------------------------------------------------------ 4. symbols and argument checks
NAMES = {"bd_srv_penalize_rows": 14, "bd_srv_step_penalize": 16}


def test_symbols_in_header_library_ctypes_table_and_integration_notes():
    from bitdelta_amd import _lib
    src = open(os.path.join(ROOT, "include", "bitdelta_hip.h")).read()
    assert re.search(r"#define\s+BD_LOGIT_BIAS_MAX\s+64\b", src)
    txt = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    for name, nargs in NAMES.items():
        decl = re.search(r"\bint\s+%s\s*\(([^;]*)\)\s*;" % name, txt)
        assert decl, name + " is not declared in include/bitdelta_hip.h"
        assert name in _lib.SIGNATURES and len(_lib.SIGNATURES[name][1]) == len(decl.group(1).split(",")) == nargs
        assert name in open(os.path.join(ROOT, "INTEGRATION.md")).read()
        assert hasattr(_lib.lib(), name)
    from bitdelta_amd import serving_loop, serving_ops
    assert callable(serving_ops.penalize_rows) and callable(serving_ops.step_penalize) and serving_ops.LOGIT_BIAS_MAX == 64
    assert callable(serving_loop.penalty_params) and callable(serving_loop.fold_history)
    import inspect
    for fn in (serving_loop.TenantSession.submit, serving_loop.TenantSession.extend, serving_loop.TenantSession.submit_all):
        assert {"repetition_penalty", "presence_penalty", "frequency_penalty", "logit_bias"} <= set(inspect.signature(fn).parameters)
    assert {"penalties", "max_logit_bias"} <= set(inspect.signature(serving_loop.TenantDecoder.session).parameters)


def test_entry_points_validate_before_any_device_call():
    from bitdelta_amd import _lib
    L = _lib.lib()
    buf = ctypes.create_string_buffer(1 << 12)
    base = (ctypes.addressof(buf) + 255) & ~255            # an aligned, non-null host address: never dereferenced by the checks
    BAD_SHAPE, BAD_DTYPE, NULL = (L.bd_srv_rope(None, None, None, -1, 1, 128, 0, 1, 0, 0, None),
                                  L.bd_srv_rope(None, None, None, 1, 1, 128, 0, 1, 0, 7, None), L.bd_srv_rope(None, None, None, 1, 1, 128, 0, 1, 0, 0, None))
    assert len({BAD_SHAPE, BAD_DTYPE, NULL, 0}) == 4
    good = dict(logits=base, sl=72, V=64, out=base, so=80, hist=base, sh=64, tok=base, active=base, pen=base, bias_id=base, bias_val=base, nb=5,
                R=2, dtype=0)

    def rows(**kw):
        a = dict(good, **kw)
        return L.bd_srv_penalize_rows(a["logits"], a["sl"], a["V"], a["out"], a["so"], a["hist"], a["sh"], a["pen"], a["bias_id"], a["bias_val"],
                                      a["nb"], a["R"], a["dtype"], None)

    def step(**kw):
        a = dict(good, **kw)
        return L.bd_srv_step_penalize(a["logits"], a["sl"], a["V"], a["out"], a["so"], a["hist"], a["sh"], a["tok"], a["active"], a["pen"],
                                      a["bias_id"], a["bias_val"], a["nb"], a["R"], a["dtype"], None)
    ptrs = ("logits", "out", "hist", "pen", "bias_id", "bias_val")
    for call in (rows, step):
        assert call(R=0) == 0 and call(R=0, tok=None, active=None, **{q: None for q in ptrs}) == 0                  # launches nothing
        assert call(R=-1) == BAD_SHAPE
        assert call(V=60) == BAD_SHAPE and call(V=0) == BAD_SHAPE and call(V=-8) == BAD_SHAPE                       # V % 8, V < 1
        assert call(V=(1 << 22) + 8, sl=(1 << 22) + 8, so=(1 << 22) + 8, sh=(1 << 22) + 8) == BAD_SHAPE              # V > 2^22
        for q in ("sl", "so", "sh"):
            assert call(**{q: 68}) == BAD_SHAPE and call(**{q: 56}) == BAD_SHAPE, q                                   # stride % 8, stride < V
        for q in ("logits", "out", "hist", "pen"):
            assert call(**{q: base + 8}) == BAD_SHAPE, q                                                              # 16-byte alignment
        assert call(bias_id=base + 2) == BAD_SHAPE and call(bias_val=base + 2) == BAD_SHAPE
        assert call(nb=-1) == BAD_SHAPE and call(nb=65) == BAD_SHAPE                                                  # 0 .. 64
        for q in ptrs:
            assert call(**{q: None}) == NULL, q
        # null lists are fine at nb = 0, and a list of 64 is: the call gets past the NULL and length checks to the layout check behind them
        assert call(nb=0, bias_id=None, bias_val=None, sl=68) == BAD_SHAPE and call(nb=64, sl=68) == BAD_SHAPE
        assert call(nb=1, bias_id=None, bias_val=None, sl=68) == NULL
        assert call(dtype=2) == BAD_DTYPE and call(dtype=7) == BAD_DTYPE and call(dtype=-1) == BAD_DTYPE
        # the order of bd_srv_token_logprobs: shape of R / V, dtype, R == 0, the list's length, null pointers, layout
        assert call(R=-1, dtype=7) == BAD_SHAPE and call(R=0, dtype=7) == BAD_DTYPE and call(R=0, nb=99, V=60) == 0
        assert call(nb=65, logits=None) == BAD_SHAPE and call(logits=None, V=60) == NULL
    assert step(tok=None) == NULL and step(active=None) == NULL and step(tok=base + 4) == BAD_SHAPE
