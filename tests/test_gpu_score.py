"""TenantDecoder.score and eval_ppl.perplexity on the GPU: the teacher-forced token losses of three fine-tunes of one base in one pass.

The yardsticks: the stock tail (log_softmax + gather on the same 16-bit logits) for the HIP token-NLL launch, and tenant t's dense fp32 twin
(the delta merged into the weights, every row's logits) for the whole path.  The band against the twin is measured inside the test from code
that predates score: e = the largest |prefill's last-row logits - the twin's| over the tenants; a logit error of e moves a log-probability by
at most 2 e, and rows other than the last are not in e, so the band is 4 e + the kernel's own bound."""
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

KERNEL = 2.0 ** -19          # include/bitdelta_hip.h (bd_srv_token_nll): |got - exact| <= 2^-19 (1 + |exact|)
ARMS = 2.0 ** -18            # HIP arm against stock arm: the kernel's bound plus the same again for fp32 log_softmax
LENGTHS = (33, 70, 128)      # pad to 128


@pytest.fixture(scope="module")
def bd():
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    import bitdelta_amd
    from bitdelta_amd import _lib
    _lib.lib()
    return bitdelta_amd


@pytest.fixture(scope="module")
def dec(bd):
    from bitdelta_amd.serving_loop import TenantDecoder
    return TenantDecoder.synthetic("tiny128", 3, "cuda", dtype=torch.float16, seed=41, max_len=256)


def _toks(n, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(1, 500, (n,), generator=g).tolist()


@pytest.fixture(scope="module")
def seqs():
    return [_toks(n, 70 + i) for i, n in enumerate(LENGTHS)]


def _dense_all_rows(bd, dec, t, ids, am):
    """test_gpu_serving._dense_reference_logits restated to return EVERY row: tenant t's model as one dense fp32 network (W + alpha * S^T), no KV
    cache, raw positions, causal mask, left pads masked as keys.  ids / am: 1-D tensors (the padded sequence).  Returns [L, vocab] fp32."""
    import torch.nn.functional as F
    from bitdelta_amd.serving_loop import _rope
    hid, inter, nl, heads, kvh, vocab = dec.cfg
    hd = dec.hd
    L = ids.shape[0]

    def merged(fl):
        S = (bd.unpack(fl.mask[t]).float() * 2 - 1).T
        return fl.weight.float() + fl.column_alpha(t)[:, None] * S

    def rms(x, w):
        return x * torch.rsqrt(x.pow(2).mean(-1, keepdim=True) + dec.eps) * w.float()

    cos, sin = dec.cos[:L].float(), dec.sin[:L].float()
    x = dec.embed[t][ids].float()
    keymask = am[None, :] & torch.ones(L, L, dtype=torch.bool, device=ids.device).tril()
    keymask = keymask | torch.eye(L, dtype=torch.bool, device=ids.device)
    for layer in dec.layers:
        q, k, v = layer.qkv.split(rms(x, layer.norm1[t]) @ merged(layer.qkv).T)
        q = _rope(q.view(L, heads, hd).transpose(0, 1)[None], cos, sin)[0]
        k = _rope(k.view(L, kvh, hd).transpose(0, 1)[None], cos, sin)[0]
        v = v.view(L, kvh, hd).transpose(0, 1)
        k, v = k.repeat_interleave(heads // kvh, 0), v.repeat_interleave(heads // kvh, 0)
        s = ((q @ k.transpose(1, 2)) / hd ** 0.5).masked_fill(~keymask[None], float("-inf"))
        x = x + (s.softmax(-1) @ v).transpose(0, 1).reshape(L, heads * hd) @ merged(layer.o).T
        g, u = layer.gate_up.split(rms(x, layer.norm2[t]) @ merged(layer.gate_up).T)
        x = x + (F.silu(g) * u) @ merged(layer.down).T
    return rms(x, dec.final_norm[t]) @ dec.lm_head[t].float().T


@pytest.fixture(scope="module")
def twin(bd, dec, seqs):
    """computed once, never modified: per tenant the dense twin's fp64 log-probabilities of every row [L, vocab], and e"""
    ids, am = dec.prepare(seqs)
    assert ids.shape == (3, 128)
    last = dec.prefill(ids, am, dec.new_cache(128))
    logp, e = [], 0.0
    for t in range(3):
        dense = _dense_all_rows(bd, dec, t, ids[t], am[t])
        e = max(e, float((last[t].float() - dense[-1]).abs().max()))
        logp.append(torch.log_softmax(dense.double(), dim=-1))
    print("e = largest |prefill last-row logit - dense fp32 twin| over the tenants: %.3e" % e)
    return {"ids": ids, "logp": logp, "e": e}


def _twin_nll(twin, seqs, t, first=1, shift=0):
    """tenant t's losses by the twin, in score's layout: entry i = -log p(seq[i + shift] | seq[:i]) for i >= first (shift = 1: wrong labels)"""
    s, L = seqs[t], 128
    pad = L - len(s)
    out = torch.zeros(len(s), dtype=torch.float64, device="cuda")
    for i in range(max(1, first), len(s) - shift):
        out[i] = -twin["logp"][t][pad + i - 1, s[i + shift]]
    return out


def _within(a, b_ref, bound, extra=0.0):
    a, b_ref = a.double(), b_ref.double()
    return bool(((a - b_ref).abs() <= extra + bound * (1.0 + b_ref.abs())).all())


@pytest.fixture(scope="module")
def scored(dec, seqs):
    return dec.score(seqs)


def test_hip_arm_against_stock_arm(dec, seqs, scored):
    stock = dec.score(seqs, hip_nll=False)
    for t in range(3):
        assert scored[t].dtype == torch.float32 and scored[t].shape == (LENGTHS[t],) and scored[t].is_cuda
        worst = float(((scored[t].double() - stock[t].double()).abs() / (1.0 + stock[t].double().abs())).max())
        print("tenant %d: HIP against stock, largest |d| / (1 + |ref|) = %.3e (bound %.3e)" % (t, worst, ARMS))
        assert _within(scored[t], stock[t], ARMS), (t, worst)
        assert bool((scored[t][1:] > 0).all())


def test_against_the_dense_fp32_twin_and_shifted_labels_fail(twin, seqs, scored):
    e = twin["e"]
    for t in range(3):
        ref = _twin_nll(twin, seqs, t)
        worst = float((scored[t].double() - ref).abs().max())
        print("tenant %d: score against the twin, largest |d| = %.3e (band 4 e = %.3e)" % (t, worst, 4 * e))
        assert _within(scored[t], ref, KERNEL, extra=4 * e), (t, worst, e)
        wrong = _twin_nll(twin, seqs, t, shift=1)                       # labels one position late: the same band must refuse them
        got = scored[t].clone()
        got[-1] = 0.0
        assert not _within(got, wrong, KERNEL, extra=4 * e), t
        bad = ((got.double() - wrong).abs() > 4 * e + KERNEL * (1.0 + wrong.abs())).float().mean().item()
        print("tenant %d: shifted labels leave the band at %.0f %% of the positions" % (t, 100 * bad))


def test_bookkeeping(dec, twin, seqs, scored):
    # positions before max(1, targets_from) are exactly 0; per-tenant targets_from; the scored entries do not move
    for tf in (0, 1):
        again = dec.score(seqs, targets_from=tf)
        assert all(torch.equal(a, b) for a, b in zip(again, scored))
    assert all(float(s[0]) == 0.0 for s in scored)
    per = [5, 69, 100]
    part = dec.score(seqs, targets_from=per)
    for t, f in enumerate(per):
        assert part[t].shape == (LENGTHS[t],) and not bool(part[t][:f].any()) and bool((part[t][f:] > 0).all())
        # (fewer rows per tenant: another GEMM shape, whose 16-bit logits may round differently -- the twin's band covers that, ARMS does not)
        assert _within(part[t][f:], scored[t][f:], KERNEL, extra=4 * twin["e"]), t
    beyond = dec.score(seqs, targets_from=[33, 200, 127])              # nothing / nothing / one token
    assert not bool(beyond[0].any()) and not bool(beyond[1].any()) and int((beyond[2] != 0).sum()) == 1 and float(beyond[2][127]) > 0
    # the left pads never show: the list holds each sequence's own length (asserted above), and a window of the padded batch has no entry for them
    # row_chunk: the lm_head in chunks of 16 / 40 / 512 rows per tenant
    for rc in (16, 40, 512):
        c = dec.score(seqs, row_chunk=rc)
        for t in range(3):
            assert _within(c[t], scored[t], ARMS), (rc, t, float((c[t] - scored[t]).abs().max()))
    # a [T, n] LongTensor equals the list input
    same = [s[:33] for s in seqs]
    a, b = dec.score(same), dec.score(torch.tensor(same, dtype=torch.long))
    c = dec.score(torch.tensor(same, dtype=torch.long).cuda())
    assert all(torch.equal(x, y) and torch.equal(x, z) for x, y, z in zip(a, b, c))


def test_tenants_are_independent(dec, seqs, scored):
    other = [seqs[0], _toks(70, 999), _toks(128, 998)]
    again = dec.score(other)
    assert torch.equal(again[0], scored[0])
    assert not torch.equal(again[1], scored[1])
    other = [_toks(33, 997), seqs[1], _toks(128, 996)]
    assert torch.equal(dec.score(other)[1], scored[1])


def test_a_live_session_is_untouched(dec, seqs, scored):
    prompt = _toks(9, 5)
    ctl = dec.session()
    ctl.submit(1, prompt, max_new_tokens=8)
    ctl.run()
    want = ctl.result(1)[0]
    sess = dec.session()
    sess.submit(1, prompt, max_new_tokens=8)
    sess.step(3)
    assert sess.active()[1]
    snap = [v.clone() for v in sess._state()] + [c.clone() for c in sess.cache["k"] + sess.cache["v"]]
    graphs = dict(sess._graphs)
    got = dec.score(seqs)
    now = sess._state() + sess.cache["k"] + sess.cache["v"]
    assert all(torch.equal(a, b) for a, b in zip(snap, now))
    assert dict(sess._graphs) == graphs and dec._kv_cache is sess.cache
    assert all(torch.equal(a, b) for a, b in zip(got, scored))
    sess.run()
    toks, reason = sess.result(1)
    assert reason == 2 and torch.equal(toks, want)


def test_tenant_view_scores_one_fine_tune_alone(dec, twin, seqs, scored):
    for t in range(3):
        alone = dec.tenant_view(t).score([seqs[t]])
        assert len(alone) == 1 and alone[0].shape == (LENGTHS[t],)
        assert _within(alone[0], scored[t], KERNEL, extra=4 * twin["e"]), t
        assert _within(alone[0], _twin_nll(twin, seqs, t), KERNEL, extra=4 * twin["e"]), t


def test_perplexity_is_the_reference_s_rule_over_score(dec):
    from bitdelta_amd.eval_ppl import perplexity, ppl_windows
    toks = _toks(300, 123)
    got = perplexity(dec, toks, context_size=128, window_size=64)
    wins = ppl_windows(300, 128, 64)
    assert wins == [(0, 192, 64), (64, 256, 64)]
    means = np.zeros((len(wins), 3))
    for w, (b, e_, n) in enumerate(wins):
        nll = dec.score([toks[b:e_]] * 3, targets_from=e_ - b - n)
        for t in range(3):
            v = nll[t].cpu().numpy().astype(np.float64)
            assert not v[:e_ - b - n].any() and (v[e_ - b - n:] > 0).all()
            means[w, t] = v[e_ - b - n:].sum() / n
    for t in range(3):
        want = math.exp(means[:, t].sum() / len(wins))
        assert math.isfinite(got[t]) and got[t] > 1.0
        assert abs(got[t] - want) <= 1e-12 * want, (t, got[t], want)
    rows = torch.tensor([toks, _toks(300, 124), toks])                                   # [T, n]: a row per tenant
    per = perplexity(dec, rows, context_size=128, window_size=64, hip_nll=False, row_chunk=40)
    # the other arm and another chunking: a window's mean moves by at most one rounding of a 16-bit logit of order 1 (2^-11) plus ARMS
    assert abs(per[0] - got[0]) <= 2e-3 * got[0] and abs(per[2] - got[2]) <= 2e-3 * got[2] and per[1] != got[1]


def test_refusals_come_before_any_launch(dec, seqs, monkeypatch):
    def never(*a, **kw):
        raise AssertionError("a refused call reached the device path")
    monkeypatch.setattr(dec, "new_cache", never)
    monkeypatch.setattr(dec, "prefill", never)
    with pytest.raises(ValueError):
        dec.score([seqs[0], [7], seqs[2]])                                               # a sequence of length 1
    with pytest.raises(ValueError):
        dec.score(seqs[:2])                                                              # a wrong number of sequences
    with pytest.raises(ValueError):
        dec.score([seqs[0], seqs[1], _toks(257, 1)])                                     # pads to 320 > max_len = 256
    with pytest.raises(ValueError):
        dec.score(seqs, targets_from=[1, 2])
    with pytest.raises(ValueError):
        dec.score(seqs, targets_from=-1)
    with pytest.raises(ValueError):
        dec.score([seqs[0], seqs[1], [1, 2, 512]])                                       # a token outside the vocabulary
    with pytest.raises(ValueError):
        dec.score(seqs, row_chunk=0)
