"""GPU tests of bd_srv_sample_rows (serving_ops.sample_rows): the sampling kernel against the fp64 / integer restatement of its definition
(tests/sampling_ref.py).  The kept set is seen through the kernel's dbg words.  Decisive cases must match exactly; the rest may land on the
adjacent answer, and their share is capped and asserted."""
import ctypes
import math

import numpy as np
import pytest
import torch

import sampling_ref as ref

pytestmark = pytest.mark.gpu

DTYPES = [torch.float16, torch.bfloat16]
NAME = {torch.float16: "float16", torch.bfloat16: "bfloat16"}
GREEDY_FLAG, TOPK_FLAG, TOPP_FLAG, SPECIAL_FLAG = 1, 2, 4, 8


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    from bitdelta_amd import _lib, serving_ops
    _lib.lib()
    return serving_ops


def _logits(R, V, dtype, seed, std=3.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(R, V, generator=g) * std).to(dtype)


def _bits(l_cpu):
    return l_cpu.view(torch.int16).numpy().view(np.uint16)


def _run(ops, l_cpu, tau, k, p, seed, d, pad=0):
    """sample_rows on the CPU tensor's rows (optionally inside wider rows: a row stride > V); returns (tokens, dbg) as numpy"""
    R, V = l_cpu.shape
    dev = "cuda"
    full = torch.full((R, V + pad), float("nan"), dtype=l_cpu.dtype)
    full[:, :V] = l_cpu
    lg = full.to(dev)[:, :V]
    per = lambda v, dt: torch.tensor(v if isinstance(v, (list, tuple)) else [v] * R, dtype=dt).to(dev)
    wrap = lambda s: [x - (1 << 64) if x >= 1 << 63 else x for x in (s if isinstance(s, (list, tuple)) else [s] * R)]
    dbg = torch.full((R, 4), -77, dtype=torch.int32, device=dev)
    tok = ops.sample_rows(lg, per(tau, torch.float32), per(k, torch.int32), per(p, torch.float32), per(wrap(seed), torch.long),
                          per(wrap(d), torch.long), dbg)
    torch.cuda.synchronize()
    return tok.cpu().numpy(), dbg.cpu().numpy()


def _list(v, R):
    return list(v) if isinstance(v, (list, tuple)) else [v] * R


def _check_rows(l_cpu, dtype, tok, dbg, tau, k, p, seed, d, what):
    """every row against the restatement; returns (rows, rows with an indecisive filter, rows with an indecisive draw)"""
    R, V = l_cpu.shape
    bits = _bits(l_cpu)
    tau, k, p, seed, d = (_list(v, R) for v in (tau, k, p, seed, d))
    soft_f = soft_d = 0
    for r in range(R):
        s = ref.sample(bits[r], NAME[dtype], tau[r], k[r], p[r], seed[r], d[r])
        ctx = (what, r, tau[r], k[r], p[r], seed[r], d[r])
        assert 0 <= tok[r] < V, ctx
        filt = (TOPK_FLAG if 1 <= k[r] < V else 0) | (TOPP_FLAG if 0 < np.float32(p[r]) < 1 else 0)
        if s["greedy"]:
            assert tok[r] == s["token"] and dbg[r, 3] & GREEDY_FLAG and list(dbg[r, :3]) == [0, 0, 0], ctx
            continue
        assert dbg[r, 3] == filt, ctx + (dbg[r].tolist(),)
        got = (int(dbg[r, 0]), int(dbg[r, 1]) & 0xffff)
        want = (s["count"], ref.pattern(s["thr"], NAME[dtype]))
        exact = got == want
        if s["filters_decisive"]:
            assert exact, ctx + (got, want)
        elif not exact:
            assert got in [(c, ref.pattern(v, NAME[dtype])) for v, c in s["near"]], ctx + (got, want, s["near"])
        if not s["filters_decisive"]:
            soft_f += 1
        if not exact:
            continue                                                  # (another kept set: the draw is over other tokens)
        word = int(dbg[r, 2]) & 0xffffffff
        if s["gap"] > s["delta"]:
            assert tok[r] == s["token"] and word == s["r"], ctx + (int(tok[r]), s["token"], s["gap"], s["delta"])
        else:
            soft_d += 1
            assert (tok[r], word) in ((s["token"], s["r"]), (s["second"], s["r_second"])), ctx + (int(tok[r]), s["token"], s["second"])
    return R, soft_f, soft_d


SHAPES = [(1, 8), (3, 8), (3, 2048), (16, 2056), (3, 32000), (1, 2056)]
BIG = [2 ** 32 + 12345, 2 ** 64 - 3, 7, 2 ** 63 + 11]                 # seeds / draw indices that exercise both high words


# ------------------------------------------------------------------------------------------------ greedy
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("R,V", SHAPES)
def test_greedy_is_argmax_and_step_end_ragged(ops, dtype, R, V):
    """tau = 0 == torch.argmax == step_end_ragged's token, with NaN, +-inf, a tied maximum and all -inf rows; any tau on a NaN / +inf row too"""
    rows = []
    base = _logits(8, V, dtype, 100 + V)
    base[1, [V - 1, V // 2, 3]] = float("nan")
    base[2, [V - 2, 5]] = float("inf")
    base[3, ::2] = float("-inf")
    base[4, [V - 1, 1, V // 3]] = base[4].max() + 1                    # a tied maximum: the lowest index wins
    base[5, :] = float("-inf")
    base[6, :] = float("-inf"); base[6, V - 1] = -3.0                  # one finite value
    base[7, 0] = float("inf"); base[7, 4] = float("nan")
    for i in range(max(R, 8)):
        rows.append(base[i % 8])
    l = torch.stack(rows)
    Rr = l.shape[0]
    want = torch.argmax(l.to("cuda"), dim=-1).cpu().numpy()
    # step_end_ragged on the same rows
    dev = "cuda"
    st = dict(tok=torch.zeros(Rr, 1, dtype=torch.long, device=dev), out=torch.zeros(Rr, 4, dtype=torch.long, device=dev),
              n=torch.zeros(Rr, dtype=torch.long, device=dev), pos=torch.zeros(Rr, dtype=torch.long, device=dev),
              limit=torch.full((Rr,), 99, dtype=torch.long, device=dev), stop=torch.full((Rr, 1), -1, dtype=torch.long, device=dev),
              act=torch.ones(Rr, dtype=torch.bool, device=dev), done=torch.zeros(Rr, dtype=torch.uint8, device=dev))
    ops.step_end_ragged(l.to(dev), st["tok"], st["out"], st["n"], st["pos"], st["limit"], st["stop"], st["act"], st["done"], 64)
    assert np.array_equal(st["tok"][:, 0].cpu().numpy(), want)
    for tau, k, p in ((0.0, 0, 1.0), (0.0, 5, 0.5)):
        tok, dbg = _run(ops, l, tau, k, p, BIG[0], BIG[1], pad=8)
        assert np.array_equal(tok, want), (tau, tok, want)
        assert (dbg[:, 3] & GREEDY_FLAG).all()
    tok, dbg = _run(ops, l, 1.0, 4, 0.9, 3, 4)
    for i in range(Rr):
        if i % 8 in (1, 2, 5, 7):                                      # NaN / +inf / nothing finite: greedy whatever tau is
            assert tok[i] == want[i] and dbg[i, 3] & SPECIAL_FLAG and dbg[i, 3] & GREEDY_FLAG, i
        else:
            assert not dbg[i, 3] & GREEDY_FLAG and 0 <= tok[i] < V and math.isfinite(float(l[i, tok[i]])), i
    assert tok[6] == V - 1                                             # the one finite value is the only token that can be drawn
    _check_rows(l, dtype, tok, dbg, 1.0, 4, 0.9, 3, 4, "special rows")


# ------------------------------------------------------------------------------------------------ top-k
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("R,V", SHAPES)
def test_top_k_is_exact(ops, dtype, R, V):
    """dbg's kept count and threshold == the restatement for top_k in {1, 2, V - 1, V, V + 5}, on random rows and on rows with ties across the
    threshold (coarse values: many equal logits; -0 next to +0; -inf entries)"""
    fine = _logits(R, V, dtype, 200 + V)
    coarse = (_logits(R, V, dtype, 300 + V).float() * 2).round().div(4).to(dtype)      # steps of 0.25: ties everywhere
    coarse[:, 1::5] = -0.0
    coarse[:, 2::7] = float("-inf")
    for name, l in (("fine", fine), ("coarse", coarse)):
        for k in (1, 2, V - 1, V, V + 5) + ((7, 50) if V > 64 else ()):
            tok, dbg = _run(ops, l, 1.0, k, 1.0, 11, 5)
            n, sf, sd = _check_rows(l, dtype, tok, dbg, 1.0, k, 1.0, 11, 5, name)
            assert sf == 0                                              # top-k alone is always decisive: it is exact


# ------------------------------------------------------------------------------------------------ top-p
def _decisive_rows(R, V, dtype, tau, k, p, start):
    """R random rows that are decisive for (tau, k, p), chosen on the CPU with the restatement alone: seeds start, start + 1, ... are tried in order"""
    rows, seed = [], start
    while len(rows) < R:
        assert seed < start + 80, "no decisive rows: (V, tau, k, p) = %r" % ((V, tau, k, p),)
        l = _logits(1, V, dtype, seed)
        seed += 1
        if ref.kept_set(ref.values(_bits(l)[0], NAME[dtype]), tau, k, p)["decisive"]:
            rows.append(l[0])
    return torch.stack(rows)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("R,V,tau", [(1, 8, 1.0), (3, 2048, 1.0), (16, 2056, 0.25), (3, 2056, 4.0), (3, 32000, 1.0), (3, 32000, 0.25)])
def test_top_p_matches_the_restatement(ops, dtype, R, V, tau):
    """dbg == the restatement for top_p in {1e-6, 0.5, 0.9, 1.0}, alone and after top-k = 40, on rows chosen decisive on the CPU (no cumulative
    ratio within 1e-4 of top_p).  (At V = 32000 and tau = 4 consecutive values are less than 1e-4 of the mass apart -- no row is decisive without
    a top-k in front -- so tau = 4 runs at V = 2056.)  Plus coarse rows (steps of 0.5: large ties at the boundary) taken as they come: a decisive
    one must match, an indecisive one must report one of the two adjacent thresholds.  Indecisive share <= 5 %, asserted."""
    rows = soft = 0
    for k in (0, 40):
        if k >= V:
            continue
        for p in (1e-6, 0.5, 0.9, 1.0):
            l = _decisive_rows(R, V, dtype, tau, k, p, 400 + V)
            tok, dbg = _run(ops, l, tau, k, p, 21, 9)
            n, sf, sd = _check_rows(l, dtype, tok, dbg, tau, k, p, 21, 9, "decisive")
            assert sf == 0
            rows, soft = rows + n, soft + sf
    coarse = (_logits(R, V, dtype, 500 + V).float() * 2).round().div(2).to(dtype)
    for p in (0.5, 0.9):
        tok, dbg = _run(ops, coarse, tau, 0, p, 22, 10)
        n, sf, sd = _check_rows(coarse, dtype, tok, dbg, tau, 0, p, 22, 10, "coarse")
        rows, soft = rows + n, soft + sf
    assert soft <= 0.05 * rows, (soft, rows)


# ------------------------------------------------------------------------------------------------ the draw
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("V,tau,R", [(64, 1.0, 256), (2056, 0.25, 48), (32000, 1.0, 12), (32000, 4.0, 12), (8, 1.0, 64), (2048, 4.0, 48)])
def test_draw_matches_the_restatement(ops, dtype, V, tau, R):
    """token and Philox word == the restatement on every decisive draw (fp64 top-two gap > 1e-3 * max(1, max|l| / tau)), one of the fp64 top two
    otherwise; indecisive share <= 5 %.  Seeds and draw indices beyond 2^32 exercise both high words; no filter, then top-k + top-p."""
    l = _logits(R, V, dtype, 600 + V)
    seeds = [BIG[r % 4] + r for r in range(R)]
    ds = [BIG[(r + 1) % 4] - r if BIG[(r + 1) % 4] > 2 ** 32 else r for r in range(R)]
    rows = soft = 0
    for k, p in ((0, 1.0), (min(50, V - 1), 0.9)):
        tok, dbg = _run(ops, l, tau, k, p, seeds, ds)
        n, sf, sd = _check_rows(l, dtype, tok, dbg, tau, k, p, seeds, ds, "draw")
        rows, soft = rows + n, soft + sd
    assert soft <= 0.05 * rows, (soft, rows)


def test_distribution_chi_square(ops):
    """4096 draws (d = 0 .. 4095) of ONE V = 64 row: the chi-square of the token counts against softmax(l / tau) over the kept set has p > 1e-4 --
    first on the restatement (so the committed seed is known good: the kernel's counts are then a deterministic function of it), then on the
    kernel.  Tokens with an expected count below 5 are pooled into one cell, the usual condition of the chi-square approximation."""
    V, N, tau, seed = 64, 4096, 1.0, 2 ** 40 + 5
    row = _logits(1, V, torch.float16, 77, std=1.5)
    bits = _bits(row)[0]
    l = ref.values(bits, "float16")
    for k, p in ((0, 1.0), (20, 0.95)):
        mask = ref.kept_set(l, tau, k, p)["mask"]
        prob = np.where(mask, np.exp((l - l.max()) / tau), 0.0)
        prob /= prob.sum()
        tok, dbg = _run(ops, row.expand(N, V).contiguous(), tau, k, p, seed, list(range(N)))
        u = ((ref.words_rows(V, seed, range(N)) >> np.uint64(8)).astype(np.float64) + 0.5) * 2.0 ** -24
        want = np.argmax(np.where(mask, l / tau - np.log(-np.log(u)), -np.inf), axis=1)       # (the first maximum: ties to the lower index)
        assert want[5] == ref.sample(bits, "float16", tau, k, p, seed, 5)["token"]
        for name, t in (("restatement", want), ("kernel", tok)):
            cnt = np.bincount(t, minlength=V).astype(np.float64)
            assert cnt[~mask].sum() == 0, name
            exp = prob * N
            big = exp >= 5
            o = np.append(cnt[big], cnt[~big].sum())
            e = np.append(exp[big], exp[~big].sum())
            o, e = o[e > 0], e[e > 0]
            chi2 = float(((o - e) ** 2 / e).sum())
            pv = ref.chi2_sf(chi2, len(e) - 1)
            print(name, "k", k, "p", p, "chi2 %.2f dof %d p-value %.4f" % (chi2, len(e) - 1, pv))
            assert pv > 1e-4, (name, chi2, len(e) - 1, pv)
        assert (tok != want).mean() <= 0.05


# ------------------------------------------------------------------------------------------------ determinism, independence of the launch
@pytest.mark.parametrize("dtype", DTYPES)
def test_determinism_and_row_independence(ops, dtype):
    """the same launch twice: equal; a row's token and dbg do not change with R or with its row index; 4096 rows in one launch"""
    V = 2056
    l = _logits(16, V, dtype, 700)
    par = dict(tau=[0.25, 1.0, 4.0, 1.0] * 4, k=[0, 50, 0, 7] * 4, p=[1.0, 0.9, 0.5, 1.0] * 4, seed=[BIG[i % 4] + i for i in range(16)],
               d=[BIG[(i + 2) % 4] - i for i in range(16)])
    a = _run(ops, l, **par)
    b = _run(ops, l, **par)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    perm = [5, 0, 15, 9, 3]
    c = _run(ops, l[perm], **{k_: [v[i] for i in perm] for k_, v in par.items()})
    assert np.array_equal(c[0], a[0][perm]) and np.array_equal(c[1], a[1][perm])
    one = _run(ops, l[9:10], **{k_: [v[9]] for k_, v in par.items()}, pad=24)
    assert one[0][0] == a[0][9] and np.array_equal(one[1][0], a[1][9])
    # R = 4096 rows of V = 64 in one launch, every row with its own parameters; a sample of them against the restatement, all of them twice
    R, V = 4096, 64
    l = _logits(R, V, dtype, 701)
    par = dict(tau=[(0.25, 1.0, 4.0)[i % 3] for i in range(R)], k=[(0, 5, 63, 70)[i % 4] for i in range(R)], p=[(1.0, 0.9, 0.5)[i % 3] for i in range(R)],
               seed=[BIG[i % 4] + i for i in range(R)], d=[BIG[(i + 1) % 4] - i for i in range(R)])
    a = _run(ops, l, **par)
    b = _run(ops, l, **par)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    idx = list(range(0, R, 16))
    n, sf, sd = _check_rows(l[idx], dtype, a[0][idx], a[1][idx], *[[par[q][i] for i in idx] for q in ("tau", "k", "p", "seed", "d")], "4096 rows")
    assert sf + sd <= 0.05 * n * 2


# ------------------------------------------------------------------------------------------------ device values the host cannot see
@pytest.mark.parametrize("dtype", DTYPES)
def test_bad_device_values_are_neutral(ops, dtype):
    """top_k < 0, top_p = NaN, top_p = 0, top_p > 1: the filter is off (the token and dbg of the call without it); tau = NaN, tau < 0, tau = inf:
    the greedy token.  Always in range."""
    V = 2056
    l = _logits(4, V, dtype, 800)
    good = _run(ops, l, 1.0, 0, 1.0, 5, 6)
    for k, p in ((-1, 1.0), (-2 ** 31, 1.0), (0, float("nan")), (0, 0.0), (0, -0.5), (0, 1.5), (V, float("inf"))):
        tok, dbg = _run(ops, l, 1.0, k, p, 5, 6)
        assert np.array_equal(tok, good[0]) and np.array_equal(dbg, good[1]), (k, p)
        assert (dbg[:, 3] == 0).all() and (dbg[:, 0] == V).all()
    only_k = _run(ops, l, 1.0, 9, 1.0, 5, 6)
    tok, dbg = _run(ops, l, 1.0, 9, float("nan"), 5, 6)
    assert np.array_equal(tok, only_k[0]) and np.array_equal(dbg, only_k[1]) and (dbg[:, 3] == TOPK_FLAG).all()
    _check_rows(l, dtype, tok, dbg, 1.0, 9, 1.0, 5, 6, "top-k alone")   # (9 tokens, or more where the 9th value is tied)
    want = torch.argmax(l.to("cuda"), dim=-1).cpu().numpy()
    for tau in (float("nan"), -1.0, float("inf"), float("-inf")):
        tok, dbg = _run(ops, l, tau, 9, 0.5, 5, 6)
        assert np.array_equal(tok, want) and (dbg[:, 3] & GREEDY_FLAG).all(), tau


# ------------------------------------------------------------------------------------------------ host refusals launch nothing
def test_abi_refusals_launch_nothing(ops):
    """null, V % 8, a misaligned row, a bad dtype: the error code comes back and tok / dbg keep their fill (nothing was launched)"""
    from bitdelta_amd._lib import lib, ptr, stream_ptr
    L = lib()
    dev = "cuda"
    R, V = 3, 64
    buf = torch.randn(R, V + 8, device=dev).half()
    tau, k, p = torch.ones(R, device=dev), torch.zeros(R, dtype=torch.int32, device=dev), torch.ones(R, device=dev)
    seed, d = torch.zeros(R, dtype=torch.long, device=dev), torch.zeros(R, dtype=torch.long, device=dev)
    tok = torch.full((R,), -5, dtype=torch.long, device=dev)
    dbg = torch.full((R, 4), -5, dtype=torch.int32, device=dev)

    def call(logits=buf.data_ptr(), sl=V + 8, V_=V, tau_=ptr(tau), tok_=ptr(tok), R_=R, dtype=0):
        return L.bd_srv_sample_rows(ctypes.c_void_p(logits), sl, V_, tau_, ptr(k), ptr(p), ptr(seed), ptr(d), tok_, ptr(dbg), R_, dtype, stream_ptr())
    codes = [call(logits=0), call(tau_=None), call(tok_=None), call(V_=60), call(sl=V + 4), call(sl=V - 8), call(logits=buf.data_ptr() + 2),
             call(dtype=2), call(dtype=9), call(R_=-1)]
    torch.cuda.synchronize()
    assert all(c != 0 for c in codes), codes
    assert len(set(codes)) == 3                                          # BD_E_NULL, BD_E_BAD_SHAPE, BD_E_BAD_DTYPE
    assert int(tok.max()) == -5 and int(dbg.max()) == -5 and int(dbg.min()) == -5
    assert call(R_=0) == 0
    torch.cuda.synchronize()
    assert int(tok.max()) == -5
    assert call() == 0
    torch.cuda.synchronize()
    assert int(tok.min()) >= 0 and int(tok.max()) < V
