"""GPU tests of bd_srv_step_penalize / bd_srv_penalize_rows (serving_ops.step_penalize / penalize_rows): EXACT bits against the restatement of
the definition (tests/penalty_ref.py; NaN elements compared as NaN), in both dtypes, at six vocabulary sizes -- one vector, part of a block, a
quarter block, one vector past a block, the served vocabulary (its last block is masked), one vector past a multiple of 8 blocks... -- with row
strides larger than V, eight tenants of which two are inactive, and every output inside poisoned canary buffers."""
import pytest
import torch

import penalty_ref as ref
from canary import POISON, CanaryOut

pytestmark = pytest.mark.gpu

DTYPES = [torch.float16, torch.bfloat16]
VS = [8, 64, 512, 2056, 32000, 32008]
T = 8
INACTIVE = (2, 5)
NB = 64
HIST_VALUES = [0, 0x8000, 1, 0x8001, 32766, 32767, 0xfffe, 0xffff, 7, 0x8123]       # unseen, context, counts 1 / 32766 / 32767 with and without bit 15
H_POISON = POISON * 0x0101
inf, nan = float("inf"), float("nan")


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    from bitdelta_amd import _lib, serving_ops
    _lib.lib()
    return serving_ops


_CASES = {}


def _case(dtype, V):
    """the eight tenants of one launch and the restatement's answers for both forms -- made once per (dtype, V) and never modified"""
    key = (dtype, V)
    if key in _CASES:
        return _CASES[key]
    g = torch.Generator().manual_seed(9000 * V + (1 if dtype == torch.bfloat16 else 0))
    pick = lambda: int(torch.randint(0, V, (1,), generator=g))
    logits = (torch.randn(T, V, generator=g) * 4).to(dtype)
    hv = torch.tensor(HIST_VALUES, dtype=torch.int32)
    hist = hv[torch.randint(0, len(HIST_VALUES), (T, V), generator=g)]
    hist[:, 0::5] = 0                                                        # (most of a real history is unseen)
    pen = torch.zeros(T, 4)
    bias_id = torch.full((T, NB), -1, dtype=torch.int32)
    bias_val = torch.zeros(T, NB)
    tok = torch.zeros(T, dtype=torch.long)
    rinv = lambda r: float(torch.tensor(1.0 / r, dtype=torch.float32))
    # 0: ordinary parameters; the token at element 0, where a bias sits too; biases at both ends of the row, a ban
    pen[0] = torch.tensor([1.3, rinv(1.3), 0.5, 0.25])
    tok[0] = 0
    hist[0, 0] = 0x8002
    bias_id[0, :4] = torch.tensor([V - 1, 0, pick(), V // 2])
    bias_val[0, :4] = torch.tensor([-3.5, 7.25, -inf, 100.0])
    # 1: special values (-inf, NaN, +-0, +inf, magnitudes that overflow fp16 once multiplied by r or 1 / r); the token at V - 1; a FULL list of
    #    64 with repeated ids (added twice, in list order: a finite value then -inf, and the other way round)
    sp = torch.tensor([-inf, nan, 0.0, -0.0, inf, -60000.0, 60000.0, -3.0e4, 3.0e4, 65504.0, -65504.0, 6.0e-8, -6.0e-8, 1.0e-40])
    logits[1] = sp[torch.randint(0, len(sp), (V,), generator=g)].to(dtype)
    hist[1, 1::2] = 0x8000
    pen[1] = torch.tensor([0.5, 2.0, -1.5, 3.0]) if V % 16 else torch.tensor([2.0, 0.5, 1.5, -3.0])
    tok[1] = V - 1
    bias_id[1] = torch.randint(0, V, (NB,), generator=g).to(torch.int32)
    bias_val[1] = torch.randn(NB, generator=g) * 30
    bias_id[1, 10], bias_id[1, 50] = bias_id[1, 3], bias_id[1, 3]
    bias_val[1, 50] = -inf
    bias_id[1, 20] = bias_id[1, 4]
    bias_val[1, 4] = -inf
    # 2, 5: inactive -- with parameters that would change everything
    for t in INACTIVE:
        pen[t] = torch.tensor([2.0, 0.5, 1.0, 1.0])
        tok[t] = pick()
        bias_id[t, 0], bias_val[t, 0] = pick(), 9.0
    # 3: neutral parameters, an empty list; the token inside the masked tail block
    pen[3] = torch.tensor([1.0, 1.0, 0.0, 0.0])
    tok[3] = V - 3
    # 4: NaN parameters written straight to the device (neutralised), ids that match nothing, one real id twice
    pen[4] = torch.tensor([nan, nan, nan, nan])
    tok[4] = pick()
    p = pick()
    bias_id[4, :7] = torch.tensor([-1, V, p, V + 5, -7, p, 2 ** 31 - 1])
    bias_val[4, :7] = torch.tensor([50.0, 50.0, 1.5, 50.0, 50.0, 2.25, 50.0])
    # 6: r = 0 or negative (off), a negative presence, frequency 2; the token on a saturated count (bit 15 set)
    pen[6] = torch.tensor([-2.0 if V % 16 else 0.0, 5.0, -1.0, 2.0])
    tok[6] = pick()
    hist[6, tok[6]] = 0xffff
    # 7: r = +inf (off), a NaN frequency; the token on count 32766 -> 32767, at the block's first vector
    pen[7] = torch.tensor([inf, 0.0, 0.75, nan])
    tok[7] = min(2048, V - 8) + 1
    hist[7, tok[7]] = 32766
    active = torch.tensor([t not in INACTIVE for t in range(T)])
    hist = ref.bits16(hist)
    prev = torch.full((T, V), H_POISON, dtype=torch.int16).view(dtype)       # what the canary output holds before the launch
    step_out, step_hist = ref.penalize(logits, hist, pen, bias_id, bias_val, tok=tok, active=active, out=prev)
    rows_out, rows_hist = ref.penalize(logits, hist, pen, bias_id, bias_val)
    assert torch.equal(rows_hist, hist)
    c = dict(logits=logits, hist=hist, pen=pen, bias_id=bias_id, bias_val=bias_val, tok=tok, active=active, step_out=step_out,
             step_hist=step_hist, rows_out=rows_out)
    _CASES[key] = c
    return c


def _padded(x, pad, fill):
    """x [T, V] on the device as a view of a [T, V + pad] buffer whose padding holds `fill` bits (int16); returns (view, buffer)"""
    buf = torch.full((x.shape[0], x.shape[1] + pad), fill, dtype=torch.int16, device="cuda")
    view = buf.view(x.dtype)[:, :x.shape[1]]
    view.copy_(x)
    return view, buf


def _dev(c):
    return {k: c[k].cuda() for k in ("pen", "bias_id", "bias_val", "tok", "active")}


NAN16 = {torch.float16: 0x7e00, torch.bfloat16: 0x7fc0}


@pytest.mark.parametrize("dtype", DTYPES, ids=["f16", "bf16"])
@pytest.mark.parametrize("V", VS)
def test_step_form_against_the_restatement(ops, dtype, V):
    c, d = _case(dtype, V), _dev(_case(dtype, V))
    lg, _ = _padded(c["logits"], 8, NAN16[dtype])                            # sl = V + 8, the padding holds NaN
    hist, hbuf = _padded(c["hist"], 16, H_POISON)                            # sh = V + 16
    out = CanaryOut(1, T, V, dtype, row_margin=2)                            # so = V + 512
    ops.step_penalize(lg, out.view[0], hist, d["tok"], d["active"], d["pen"], d["bias_id"], d["bias_val"])
    got, got_h = out.view[0].cpu(), hist.cpu()
    assert ref.same_bits(got, c["step_out"])
    assert torch.equal(got_h, c["step_hist"])
    # the inactive tenants' rows still hold the canary; nothing outside the output or past V in hist was written
    for t in INACTIVE:
        assert bool((got[t].view(torch.int16) == H_POISON).all()) and torch.equal(got_h[t], c["hist"][t]), t
    assert out.untouched_outside() and bool((hbuf[:, V:] == H_POISON).all())
    # hist differs from before only at [t, tok[t]] of the active tenants, by the saturating +1 with bit 15 kept
    diff = (got_h != c["hist"]).nonzero().tolist()
    want = []
    for t in range(T):
        y = int(c["tok"][t])
        old = int(c["hist"][t, y]) & 0xffff
        if t not in INACTIVE and old & 0x7fff != 0x7fff:
            want.append([t, y])
            assert int(got_h[t, y]) & 0xffff == old + 1, t
    assert diff == sorted(want) and [6, int(c["tok"][6])] not in diff and {0, 1, 7} <= {t for t, _ in diff}


@pytest.mark.parametrize("dtype", DTYPES, ids=["f16", "bf16"])
@pytest.mark.parametrize("V", VS)
def test_rows_form_is_the_step_form_without_the_count(ops, dtype, V):
    c, d = _case(dtype, V), _dev(_case(dtype, V))
    lg, _ = _padded(c["logits"], 24, NAN16[dtype])
    hist, hbuf = _padded(c["hist"], 8, H_POISON)
    out = CanaryOut(1, T, V, dtype, row_margin=2)
    res = ops.penalize_rows(lg, hist, d["pen"], d["bias_id"], d["bias_val"], out=out.view[0])
    assert res.data_ptr() == out.view[0].data_ptr()
    got = out.view[0].cpu()
    assert ref.same_bits(got, c["rows_out"])                                 # every row is live
    assert out.untouched_outside() and torch.equal(hbuf.cpu(), _padded(c["hist"], 8, H_POISON)[1].cpu())      # hist is only read
    # the step form with tokens that count nothing (outside the vocabulary) and every tenant active: the same bits, hist unchanged
    out2 = torch.zeros(T, V, dtype=dtype, device="cuda")
    nowhere = torch.tensor([-1, V, V + 3, 2 ** 40, -2 ** 40, V + 2047, 2 ** 31, 2 ** 32 + 5], device="cuda")
    ops.step_penalize(lg, out2, hist, nowhere, torch.ones(T, dtype=torch.bool, device="cuda"), d["pen"], d["bias_id"], d["bias_val"])
    assert torch.equal(out2.cpu().view(torch.int16), got.view(torch.int16)) and torch.equal(hist.cpu(), c["hist"])
    # and where the step form does count, it differs from the rows form at most at the counted elements
    step = c["step_out"].view(torch.int16) != c["rows_out"].view(torch.int16)
    for t in range(T):
        if t not in INACTIVE:
            assert step[t].nonzero().flatten().tolist() in ([], [int(c["tok"][t])]), t


@pytest.mark.parametrize("dtype", DTYPES, ids=["f16", "bf16"])
@pytest.mark.parametrize("V", VS)
def test_neutral_parameters_return_the_input_bits(ops, dtype, V):
    """r = 1, presence = frequency = 0 and an empty list -- null pointers, and a list of -1 ids -- whatever the history holds; +-0, +-inf and
    subnormals included (row 1).  NaN elements stay NaN."""
    c = _case(dtype, V)
    lg, hist = c["logits"].cuda(), c["hist"].cuda()
    pen = torch.tensor([[1.0, 1.0, 0.0, 0.0]] * T, device="cuda")
    act = torch.ones(T, dtype=torch.bool, device="cuda")
    a = ops.penalize_rows(lg, hist, pen)
    b = ops.penalize_rows(lg, hist, pen, torch.full((T, 3), -1, dtype=torch.int32, device="cuda"), torch.ones(T, 3, device="cuda"))
    h2 = hist.clone()
    s = ops.step_penalize(lg, torch.zeros_like(lg), h2, c["tok"].cuda(), act, pen)
    for got in (a, b, s):
        assert ref.same_bits(got.cpu(), c["logits"])
        keep = ~torch.isnan(c["logits"])
        assert torch.equal(got.cpu().view(torch.int16)[keep], c["logits"].view(torch.int16)[keep])
    assert torch.equal(h2.cpu(), ref.penalize(c["logits"], c["hist"], pen.cpu(), tok=c["tok"], active=act.cpu())[1])


@pytest.mark.parametrize("dtype", DTYPES, ids=["f16", "bf16"])
@pytest.mark.parametrize("V", [2056, 32000])
def test_same_bits_alone_at_another_stride_and_from_a_graph(ops, dtype, V):
    """an element is a pure function of its own inputs: a tenant launched alone, contiguous rows instead of padded ones, and a replayed capture
    of the launch give the bits of the eight-tenant launch"""
    from bitdelta_amd._lib import DTYPE_CODE, lib, ptr, stream_ptr
    c, d = _case(dtype, V), _dev(_case(dtype, V))
    want, want_h = c["step_out"], c["step_hist"]
    for t in range(T):
        if t in INACTIVE:
            continue
        h = c["hist"][t:t + 1].cuda()
        got = ops.step_penalize(c["logits"][t:t + 1].cuda(), torch.zeros(1, V, dtype=dtype, device="cuda"), h, d["tok"][t:t + 1],
                                d["active"][t:t + 1], d["pen"][t:t + 1], d["bias_id"][t:t + 1], d["bias_val"][t:t + 1])
        assert ref.same_bits(got.cpu(), want[t:t + 1]) and torch.equal(h.cpu(), want_h[t:t + 1]), t
        rows = ops.penalize_rows(c["logits"][t:t + 1].cuda(), c["hist"][t:t + 1].cuda(), d["pen"][t:t + 1], d["bias_id"][t:t + 1], d["bias_val"][t:t + 1])
        assert ref.same_bits(rows.cpu(), c["rows_out"][t:t + 1]), t
    # contiguous rows (stride V), the launch captured once and replayed twice: the history counts once per replay
    lg, hist = c["logits"].cuda(), c["hist"].cuda()
    out = torch.full((T, V), H_POISON, dtype=torch.int16, device="cuda").view(dtype)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        rc = lib().bd_srv_step_penalize(ptr(lg), V, V, ptr(out), V, ptr(hist), V, ptr(d["tok"]), ptr(d["active"]), ptr(d["pen"]), ptr(d["bias_id"]),
                                        ptr(d["bias_val"]), NB, T, DTYPE_CODE[dtype], stream_ptr())
    assert rc == 0
    graph.replay()
    torch.cuda.synchronize()
    assert ref.same_bits(out.cpu(), want) and torch.equal(hist.cpu(), want_h)
    graph.replay()
    torch.cuda.synchronize()
    prev = torch.full((T, V), H_POISON, dtype=torch.int16).view(dtype)
    out2, hist2 = ref.penalize(c["logits"], want_h, c["pen"], c["bias_id"], c["bias_val"], tok=c["tok"], active=c["active"], out=prev)
    assert ref.same_bits(out.cpu(), out2) and torch.equal(hist.cpu(), hist2)


def test_wrapper_refuses_what_the_entry_points_do_not_take(ops):
    V = 64
    lg = torch.zeros(2, V, dtype=torch.float16, device="cuda")
    hist = torch.zeros(2, V, dtype=torch.int16, device="cuda")
    pen = torch.tensor([[1.0, 1.0, 0.0, 0.0]] * 2, device="cuda")
    with pytest.raises(AssertionError):
        ops.penalize_rows(lg, hist.int(), pen)
    with pytest.raises(AssertionError):
        ops.penalize_rows(lg, hist, pen[:, :3])
    with pytest.raises(AssertionError):
        ops.penalize_rows(lg, hist, pen, torch.zeros(2, 65, dtype=torch.int32, device="cuda"), torch.zeros(2, 65, device="cuda"))
    with pytest.raises(Exception):
        ops.penalize_rows(lg.cpu(), hist, pen)
    assert ops.penalize_rows(lg[:0], hist[:0], pen[:0]).shape == (0, V)      # no rows: nothing is launched
