"""GPU tests of bd_srv_truncate_rows / bd_srv_step_truncate (serving_ops.truncate_rows / step_truncate) against the fp64 restatement of the
definition and its acceptance rule (tests/truncation_ref.py: E = 1e-4 on masses, delta = 1e-4 * max(1, max |x|) on x and on keys, derived
there).  Both entry points and both dtypes; V = 8 (one vector), 2048 (exactly one trip of 256 threads), 2056 (one vector past it), 32000 (the
real row) and 32776 (past the register-resident form); 1, 6 and 16 rows; logits N(0, sd) with sd in {0.5, 2, 6} and a tenth of the row at -inf;
tau in {0.3, 1, 1.7}; each filter alone at three settings, all four together, and every row of a launch with parameters of its own.  Every
random row is one on which the reference keeps more than one and fewer than all finite elements (asserted), every test reports how many rows
came out EXACTLY equal to the reference's set, and the always-exact properties -- kept bits unchanged, dropped elements the dtype's -inf, -inf
stays -inf, copied rows bit-identical, an inactive tenant's row untouched, nothing outside the output written -- are checked on the whole row
inside a poisoned canary buffer.  The reference of a row is computed once and shared."""
import math

import numpy as np
import pytest
import torch

import truncation_ref as ref
from canary import POISON, CanaryOut

pytestmark = pytest.mark.gpu

DTYPES = [torch.float16, torch.bfloat16]
NAME = {torch.float16: "float16", torch.bfloat16: "bfloat16"}
VS = [8, 2048, 2056, 32000]
POISON16 = POISON * 0x0101
inf, nan = float("inf"), float("nan")

# (sd, tau, (min_p, typical_p, epsilon_cutoff, eta_cutoff)) of row r % 13 of a launch: each filter alone at three settings -- with every
# sd, and every tau among them -- and all four together.  The parameters are chosen so that the REFERENCE keeps more than one and fewer than all
# finite elements on every row the tests make at these sizes (asserted per row): V = 8 needs coarser ones than a long row.
SETTINGS = {
    "long": [(2.0, 1.0, (0.05, 1.0, 0.0, 0.0)), (0.5, 0.3, (0.2, 1.0, 0.0, 0.0)), (6.0, 1.7, (0.01, 1.0, 0.0, 0.0)),
             (2.0, 1.0, (0.0, 0.9, 0.0, 0.0)), (0.5, 0.3, (0.0, 0.5, 0.0, 0.0)), (6.0, 1.7, (0.0, 0.2, 0.0, 0.0)),
             (2.0, 1.0, (0.0, 1.0, 3e-4, 0.0)), (0.5, 0.3, (0.0, 1.0, 1e-4, 0.0)), (6.0, 1.7, (0.0, 1.0, 1e-3, 0.0)),
             (2.0, 0.3, (0.0, 1.0, 0.0, 3e-4)), (0.5, 1.0, (0.0, 1.0, 0.0, 0.9)), (6.0, 1.7, (0.0, 1.0, 0.0, 0.05)),
             (2.0, 1.0, (0.02, 0.95, 1e-4, 3e-4))],
    "short": [(2.0, 1.0, (0.1, 1.0, 0.0, 0.0)), (0.5, 0.3, (0.1, 1.0, 0.0, 0.0)), (6.0, 1.7, (0.02, 1.0, 0.0, 0.0)),
              (2.0, 1.0, (0.0, 0.9, 0.0, 0.0)), (0.5, 1.7, (0.0, 0.5, 0.0, 0.0)), (6.0, 1.7, (0.0, 0.9, 0.0, 0.0)),
              (6.0, 1.7, (0.0, 1.0, 0.01, 0.0)), (0.5, 1.0, (0.0, 1.0, 0.1, 0.0)), (2.0, 1.7, (0.0, 1.0, 0.05, 0.0)),
              (2.0, 0.3, (0.0, 1.0, 0.0, 0.05)), (0.5, 1.0, (0.0, 1.0, 0.0, 0.3)), (6.0, 1.7, (0.0, 1.0, 0.0, 0.05)),
              (2.0, 1.0, (0.05, 0.95, 0.02, 0.05))],
}


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    from bitdelta_amd import _lib, serving_ops
    _lib.lib()
    return serving_ops


def _bits(t):
    """the 16-bit patterns of a 16-bit tensor, as numpy uint16"""
    return t.contiguous().view(torch.int16).cpu().numpy().view(np.uint16)


def setting(V, r):
    return SETTINGS["short" if V < 64 else "long"][r % 13]


def random_row(dtype, V, r):
    """row r of the (dtype, V) launches, on the CPU: N(0, sd) with a tenth of the row at -inf; the same whatever the launch's row count is"""
    sd = setting(V, r)[0]
    g = torch.Generator().manual_seed(1000003 * V + 17 * r + (1 if dtype == torch.bfloat16 else 0))
    x = torch.randn(V, generator=g) * sd
    x[torch.rand(V, generator=g) < 0.1] = -inf
    return x.to(dtype)


_ROWS = {}


def _row(dtype, V, r):
    """(logits row, its bits, tau, params, the reference) -- made once per (dtype, V, r), never modified"""
    key = (dtype, V, r)
    if key not in _ROWS:
        _, tau, prm = setting(V, r)
        row = random_row(dtype, V, r)
        b = _bits(row)
        _ROWS[key] = (row, b, tau, prm, ref.reference(b, NAME[dtype], tau, prm))
    return _ROWS[key]


def _launch(ops, form, logits, tau, params, active=None):
    """the launch into a poisoned canary buffer; returns (out bits [R, V], canary).  form "rows" / "step"; active: the step form's flags"""
    R, V = logits.shape
    can = CanaryOut(1, R, V, logits.dtype, row_margin=8, col_margin=256)
    out = can.view[0]
    tau_d = torch.tensor(tau, dtype=torch.float32).cuda()
    prm_d = torch.tensor(params, dtype=torch.float32).reshape(R, 4).cuda()
    if form == "rows":
        got = ops.truncate_rows(logits, tau_d, prm_d, out=out)
    else:
        act = torch.ones(R, dtype=torch.bool) if active is None else torch.tensor(active, dtype=torch.bool)
        got = ops.step_truncate(logits, out, tau_d, prm_d, act.cuda())
    assert got.data_ptr() == out.data_ptr()
    torch.cuda.synchronize()
    return _bits(out), can


def _judge(dtype, in_bits, taus, prms, out_bits, refs=None):
    """check_row on every row; returns the number of rows that are exactly the reference's"""
    exact = 0
    for r in range(in_bits.shape[0]):
        exact += ref.check_row(in_bits[r], NAME[dtype], taus[r], prms[r], out_bits[r], r=None if refs is None else refs[r])
    return exact


# ------------------------------------------------------------------------------------------------ 1. random rows, every size, both forms
@pytest.mark.parametrize("form", ["rows", "step"])
@pytest.mark.parametrize("V", VS)
@pytest.mark.parametrize("dtype", DTYPES, ids=["f16", "bf16"])
def test_random_rows_every_filter_and_every_row_with_its_own_parameters(ops, dtype, V, form):
    total = exact = 0
    for R in (1, 6, 16):
        rows = [_row(dtype, V, r) for r in range(R)]
        for r, (_, b, tau, prm, rf) in enumerate(rows):                  # the power of the case: the reference cuts the row, and not to one token
            assert not rf["copied"] and 1 < int(rf["mask"].sum()) < int(rf["st"]["fin"].sum()), (V, r, int(rf["mask"].sum()))
        logits = torch.stack([q[0] for q in rows]).cuda()
        out, can = _launch(ops, form, logits, [q[2] for q in rows], [q[3] for q in rows])
        exact += _judge(dtype, np.stack([q[1] for q in rows]), [q[2] for q in rows], [q[3] for q in rows], out, [q[4] for q in rows])
        total += R
        assert can.untouched_outside()
    print("%s V=%d %s: %d of %d rows exactly the reference's set" % (NAME[dtype], V, form, exact, total))
    assert exact >= 1


@pytest.mark.parametrize("dtype", DTYPES, ids=["f16", "bf16"])
def test_the_two_forms_agree_bit_for_bit_and_a_launch_repeats_itself(ops, dtype):
    for V in VS:
        rows = [_row(dtype, V, r) for r in range(16)]
        logits = torch.stack([q[0] for q in rows]).cuda()
        taus, prms = [q[2] for q in rows], [q[3] for q in rows]
        a, _ = _launch(ops, "rows", logits, taus, prms)
        b, _ = _launch(ops, "step", logits, taus, prms)
        c, _ = _launch(ops, "step", logits, taus, prms)
        d, _ = _launch(ops, "rows", logits[3:9], taus[3:9], prms[3:9])   # other neighbours, another row index: the same bits
        assert np.array_equal(a, b) and np.array_equal(b, c) and np.array_equal(a[3:9], d)


# ------------------------------------------------------------------------------------------------ 2. edge rows
def _known(dtype, V):
    row = torch.full((V,), -inf)
    row[:4] = torch.log(torch.tensor([0.5, 0.25, 0.125, 0.125]))
    return row.to(dtype)


def _edge_rows(dtype, V):
    """(name, row, tau, params, the kept indices or None = judged by the rule / "copy") -- the margins of the crafted rows are wide"""
    g = torch.Generator().manual_seed(77 + V)
    base = (torch.randn(V, generator=g) * 2).to(dtype)
    all4 = (0.05, 0.9, 1e-4, 3e-4)
    rows = []
    one = torch.full((V,), -inf)
    one[V - 3] = -7.25
    rows.append(("one finite element", one.to(dtype), 1.0, all4, [V - 3]))
    rows.append(("all finite elements equal", torch.where(torch.arange(V) % 5 == 0, torch.tensor(-inf), torch.tensor(1.5)).to(dtype), 0.7, all4,
                 [i for i in range(V) if i % 5]))
    tie = base.clone().float()
    tie[1], tie[V - 1] = 9.0, 9.0
    rows.append(("a tie at the maximum, min_p = 1", tie.to(dtype), 1.0, (1.0, 1.0, 0.0, 0.0), [1, V - 1]))
    rows.append(("min_p past 1 (a device value): the maximum only", tie.to(dtype), 1.0, (2.0, 1.0, 0.0, 0.0), [1, V - 1]))
    wide = ((torch.rand(V, generator=g) * 2 - 1) * 60000.0)
    wide[V // 2] = 65000.0
    rows.append(("tau = 0.01 on a wide row: the masses underflow", wide.to(dtype), 0.01, (0.1, 0.9, 1e-4, 3e-4), [V // 2]))
    rows.append(("tau = 0.01, typical_p alone", wide.to(dtype), 0.01, (0.0, 0.9, 0.0, 0.0), [V // 2]))
    for name, val in (("a NaN", nan), ("a +inf", inf)):
        sp = base.clone().float()
        sp[V // 3] = val
        rows.append((name + ": copied", sp.to(dtype), 1.0, all4, "copy"))
    rows.append(("nothing finite: copied", torch.full((V,), -inf).to(dtype), 1.0, all4, "copy"))
    for tau in (0.0, -1.0, inf, nan):
        rows.append(("tau = %r (greedy): copied" % tau, base, tau, all4, "copy"))
    nz = base.clone().float()
    nz[0], nz[5] = nan, -0.0
    rows.append(("neutral parameters: copied, NaN and -0 included", nz.to(dtype), 1.0, ref.NEUTRAL, "copy"))
    rows.append(("parameters off by device values: copied", base, 1.0, (-0.5, 1.5, nan, -1.0), "copy"))
    rows.append(("typical_p = 0 is off (a device value)", base, 1.0, (0.0, 0.0, 0.0, 0.0), "copy"))
    rows.append(("the known row: min_p 0.3", _known(dtype, V), 1.0, (0.3, 1.0, 0.0, 0.0), [0, 1]))
    rows.append(("the known row: typical_p 0.2 drops the maximum", _known(dtype, V), 1.0, (0.0, 0.2, 0.0, 0.0), [1]))
    rows.append(("the known row: eta 0.2", _known(dtype, V), 1.0, (0.0, 1.0, 0.0, 0.2), [0, 1]))
    rows.append(("the known row: the intersection", _known(dtype, V), 1.0, (0.3, 0.2, 0.0, 0.0), [1]))
    rows.append(("the crafted fallback row: typical_p ignored", _known(dtype, V), 1.0, (0.6, 0.2, 0.0, 0.0), [0]))
    return rows


@pytest.mark.parametrize("form", ["rows", "step"])
@pytest.mark.parametrize("V", [8, 2056])
@pytest.mark.parametrize("dtype", DTYPES, ids=["f16", "bf16"])
def test_edge_rows_an_inactive_tenant_and_a_strided_input(ops, dtype, V, form):
    rows = _edge_rows(dtype, V)
    R = len(rows)
    wide = torch.full((R, V + 24), 3.0, dtype=dtype)                     # a non-contiguous row stride: the columns past V are never read
    for r, q in enumerate(rows):
        wide[r, :V] = q[1]
    logits = wide.cuda()[:, :V]
    assert logits.stride(0) == V + 24 and not logits.is_contiguous()
    taus, prms = [q[2] for q in rows], [q[3] for q in rows]
    active = [r % 7 != 3 for r in range(R)] if form == "step" else None
    out, can = _launch(ops, form, logits, taus, prms, active=active)
    in_bits = _bits(logits)
    exact = 0
    for r, (name, _, tau, prm, want) in enumerate(rows):
        if active is not None and not active[r]:
            assert bool((out[r] == POISON16).all()), name + ": an inactive tenant's row was written"
            continue
        e = ref.check_row(in_bits[r], NAME[dtype], tau, prm, out[r])
        exact += e
        if want == "copy":
            assert np.array_equal(out[r], in_bits[r]), name
        else:
            kept = np.nonzero(out[r] != ref.NINF[NAME[dtype]])[0].tolist()
            assert kept == want and e, (name, kept[:8], want[:8])
    assert can.untouched_outside()
    print("%s V=%d %s: %d of %d edge rows exactly the reference's set" % (NAME[dtype], V, form, exact, R))


# ------------------------------------------------------------------------------------------------ 3. past the register-resident form
@pytest.mark.parametrize("dtype", DTYPES, ids=["f16", "bf16"])
def test_a_row_longer_than_the_registers_hold(ops, dtype):
    V = 32776
    rows = [_row(dtype, V, r) for r in (0, 3, 6, 9, 12)]
    for _, _, _, _, rf in rows:
        assert 1 < int(rf["mask"].sum()) < int(rf["st"]["fin"].sum())
    logits = torch.stack([q[0] for q in rows]).cuda()
    taus, prms = [q[2] for q in rows], [q[3] for q in rows]
    a, can = _launch(ops, "rows", logits, taus, prms)
    b, _ = _launch(ops, "step", logits, taus, prms, active=[True, False, True, True, True])
    exact = _judge(dtype, np.stack([q[1] for q in rows]), taus, prms, a, [q[4] for q in rows])
    assert can.untouched_outside() and np.array_equal(np.delete(a, 1, 0), np.delete(b, 1, 0)) and bool((b[1] == POISON16).all())
    print("%s V=%d: %d of %d rows exactly the reference's set" % (NAME[dtype], V, exact, len(rows)))
    assert exact >= 1


def test_layout_asserts(ops):
    x = torch.zeros(2, 16, dtype=torch.float16).cuda()
    tau = torch.ones(2).cuda()
    prm = torch.tensor([ref.NEUTRAL] * 2, dtype=torch.float32).cuda()
    for bad in (dict(tau=tau.double()), dict(params=prm[:, :3].contiguous()), dict(params=prm.t().contiguous().t()), dict(tau=tau[:1]),
                dict(out=torch.zeros(2, 16, dtype=torch.bfloat16).cuda()), dict(out=torch.zeros(2, 24, dtype=torch.float16).cuda())):
        kw = dict(dict(tau=tau, params=prm, out=None), **bad)
        with pytest.raises(AssertionError):
            ops.truncate_rows(x, kw["tau"], kw["params"], out=kw["out"])
    with pytest.raises(AssertionError):
        ops.step_truncate(x, torch.zeros_like(x), tau, prm, torch.ones(2, dtype=torch.int32).cuda())
    with pytest.raises(AssertionError):
        ops.truncate_rows(torch.zeros(2, 12, dtype=torch.float16).cuda(), tau, prm)
    assert torch.equal(ops.truncate_rows(x, tau, prm), x) and math.isfinite(float(x.sum()))
