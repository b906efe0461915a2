"""CPU-only checks of the hard bans (no_repeat_ngram_size / bad_words / min_new_tokens): ban_params accepts and refuses what it documents and
returns a canonical form; the table builder pads; the restatement (ban_ref) answers the hand cases of the definition and agrees with the three
Hugging Face processors on random small cases wherever the history is at least as long as the longest bad word; a session made without
bans=True refuses the arguments; the BD_BAN_* limits of the header are the serving_ops constants; both C-ABI symbols are in the header, the
library, the ctypes table and INTEGRATION.md and answer their argument checks, in the documented order, before any device call."""
import ctypes
import inspect
import os
import random
import re

import pytest

import ban_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------------------------ 1. ban_params and the table
def test_ban_params_accepts_and_normalises():
    import numpy as np
    from bitdelta_amd.serving_loop import NO_BANS, ban_params
    assert ban_params() == NO_BANS == (0, (), 0)
    assert ban_params(0, None, 0) == NO_BANS and ban_params(0, [], 0) == NO_BANS
    got = ban_params(3, [[7, 8], (9,)], 5, vocab=16)
    assert got == (3, ((7, 8), (9,)), 5) and all(type(v) is int for w in got[1] for v in w) and type(got[0]) is int and type(got[2]) is int
    assert ban_params(np.int64(2), [[np.int32(4), np.int64(5)]], np.int32(1), vocab=8) == (2, ((4, 5),), 1)
    assert ban_params(8)[0] == 8 and ban_params(1)[0] == 1
    assert ban_params(bad_words=[[0, 511]], vocab=512)[1] == ((0, 511),)
    assert ban_params(bad_words=[[1], [1]])[1] == ((1,), (1,))                           # the caller's order, nothing merged
    assert ban_params(min_new_tokens=2 ** 40)[2] == 2 ** 31 - 1                           # past int32: the same as "never before the end"
    full = [[(q + j) % 512 for j in range(32)] for q in range(64)]
    assert ban_params(bad_words=full, vocab=512)[1] == tuple(tuple(w) for w in full)      # the ABI maxima
    assert ban_params(bad_words=[[1] * 8] * 16, max_bad_words=16, max_bad_word_len=8)[1] == ((1,) * 8,) * 16


@pytest.mark.parametrize("kw", [
    dict(no_repeat_ngram_size=-1), dict(no_repeat_ngram_size=9), dict(no_repeat_ngram_size=True), dict(no_repeat_ngram_size=2.0),
    dict(no_repeat_ngram_size="2"), dict(no_repeat_ngram_size=None),
    dict(min_new_tokens=-1), dict(min_new_tokens=False), dict(min_new_tokens=1.5), dict(min_new_tokens=None),
    dict(bad_words=[[]]), dict(bad_words=[[1, 2], []]), dict(bad_words=[[1.0]]), dict(bad_words=[[True]]), dict(bad_words=[["a"]]),
    dict(bad_words=[[None]]), dict(bad_words=[[512]], vocab=512), dict(bad_words=[[3, -1]]), dict(bad_words=[[2 ** 31]]),
    dict(bad_words=[1, 2]), dict(bad_words="ab"), dict(bad_words=5), dict(bad_words={1: 2}),
    dict(bad_words=[[1]] * 65), dict(bad_words=[[1] * 33]),
    dict(bad_words=[[1]] * 17, max_bad_words=16), dict(bad_words=[[1] * 9], max_bad_word_len=8),
])
def test_ban_params_refuses(kw):
    from bitdelta_amd.serving_loop import ban_params
    with pytest.raises(ValueError):
        ban_params(**kw)


def test_table_builder_pads_and_refuses():
    from bitdelta_amd.serving_loop import ban_params, ban_word_table
    tok, lens = ban_word_table(ban_params(bad_words=[[7, 8, 9], (3,)])[1], 4, 5)
    assert tok == [[7, 8, 9, -1, -1], [3, -1, -1, -1, -1], [-1] * 5, [-1] * 5] and lens == [3, 1, 0, 0]
    assert ban_word_table((), 2, 3) == ([[-1] * 3] * 2, [0, 0])
    assert ban_word_table(((1, 2),), 1, 2) == ([[1, 2]], [2])
    for words, Q, W in ((((1,), (2,)), 1, 4), (((1, 2, 3),), 4, 2)):
        with pytest.raises(ValueError):
            ban_word_table(words, Q, W)


# ------------------------------------------------------------------------------------------------ 2. the restatement
def test_hand_cases_of_the_definition():
    b = ref.banned
    # n-gram: the last g - 1 tokens occurred before -> what followed them is banned
    assert b([1, 2, 3, 1, 2], g=3) == {3} and b([1, 2, 3, 1], g=3) == set() and b([1, 2, 3, 1, 2], g=2) == {3}
    assert b([5, 6, 7], g=1) == {5, 6, 7} and b([], g=1) == set()                         # g = 1: every token of the history
    assert b([4, 4, 4, 4], g=2) == {4} and b([4, 4, 4, 4], g=3) == {4} and b([4, 4], g=3) == set()      # overlapping matches; m = g - 1: no i
    assert b([4, 4, 4], g=3) == {4}                                                         # m = g: i = 0 only
    assert b([1], g=3) == set() and b([], g=2) == set()                                    # m < g - 1 (m = 0 with g = 2: the empty tail, no i)
    assert b([1, 2, 1, 3, 1], g=2) == {2, 3}
    # bad words
    assert b([], words=[[9]]) == {9} and b([1], words=[[1, 2]]) == {2} and b([], words=[[1, 2]]) == set()
    assert b([1], words=[[5, 1, 2]]) == set() and b([5, 1], words=[[5, 1, 2]]) == {2} and b([3, 5, 1], words=[[5, 1, 2], [1, 7], [4, 8]]) == {2, 7}
    # early stop: stop ids only, while n < min_new
    assert b([1], n=2, min_new=3, stops=[7, -1, 9]) == {7, 9} and b([1], n=3, min_new=3, stops=[7]) == set()
    assert b([1, 2, 1], g=2, words=[[1, 4]], n=0, min_new=1, stops=[6]) == {2, 4, 6}     # the union
    assert ref.repeats_ngram([1, 2, 3, 1, 2], 2) and not ref.repeats_ngram([1, 2, 3, 2, 1], 2)
    assert ref.completes_word([1], [2, 3], [[1, 2]]) and not ref.completes_word([1], [3, 2], [[1, 2]])
    # device values the clamps neutralise
    h, nn, g, words = ref.clamp_row([1, 2, 3], 7, [4, 5], 9, 12, [[6, 7], [8, -1]], [5, 1], 2)
    assert (h, nn, g, words) == ([1, 2, 3, 4, 5], 2, 0, [[8]])
    assert ref.clamp_row([1, 2, 3], -4, [4, 5], -1, -2, [[6, 7]], [-1], 2) == ([], 0, 0, [])


def test_restatement_against_transformers_processors():
    """HF's three processors on one row: wherever the history is at least as long as the longest bad word the banned sets are equal (below that
    length the definition deviates on purpose: see the header)"""
    try:
        import torch
        from transformers.generation.logits_process import (MinNewTokensLengthLogitsProcessor, NoBadWordsLogitsProcessor,
                                                            NoRepeatNGramLogitsProcessor)
    except Exception as e:                                                                  # noqa: BLE001
        pytest.skip("transformers cannot be imported: %r" % (e,))
    rng = random.Random(20241021)
    V, EOS = 6, [4, 5]
    seen_ngram = seen_word = seen_min = 0
    for _ in range(300):
        g = rng.randint(1, 4)
        words = [[rng.randrange(V) for _ in range(rng.randint(1, 3))] for _ in range(rng.randint(1, 3))]
        words = [list(w) for w in dict.fromkeys(tuple(w) for w in words)]
        prompt_len, min_new = rng.randint(1, 4), rng.randint(0, 3)
        h = [rng.randrange(V) for _ in range(rng.randint(max(prompt_len, max(len(w) for w in words)), 10))]
        n = len(h) - prompt_len
        if n < 0:
            continue
        ids, scores = torch.tensor([h]), torch.zeros(1, V)
        hf = set()
        hf |= set((NoRepeatNGramLogitsProcessor(g)(ids, scores.clone())[0] == -float("inf")).nonzero().flatten().tolist())
        a = set((NoBadWordsLogitsProcessor(words, eos_token_id=None)(ids, scores.clone())[0] == -float("inf")).nonzero().flatten().tolist())
        if min_new > 0:
            c = set((MinNewTokensLengthLogitsProcessor(prompt_len, min_new, EOS)(ids, scores.clone())[0] == -float("inf")).nonzero().flatten().tolist())
        else:
            c = set()
        assert ref.banned_ngram(h, g) == hf, (h, g)
        assert ref.banned_words(h, words) == a, (h, words)
        assert ref.banned(h, 0, (), n, min_new, EOS) == c, (h, n, min_new)
        assert ref.banned(h, g, words, n, min_new, EOS) == hf | a | c
        seen_ngram += bool(hf)
        seen_word += bool(a)
        seen_min += bool(c)
    assert seen_ngram > 50 and seen_word > 50 and seen_min > 20


# ------------------------------------------------------------------------------------------------ 3. the session's arguments
def _bare(flag, T=4, Q=16, W=8, vocab=512):
    import torch
    from bitdelta_amd.serving_loop import TenantSession
    s = object.__new__(TenantSession)
    s.bans, s.T = flag, T

    class _Dec:
        lm_head = torch.zeros(1, vocab, 8)
    s.dec = _Dec()
    if flag:
        s.ban_tok = torch.zeros(T, Q, W, dtype=torch.int32)
    return s


def test_a_session_without_the_feature_refuses_the_arguments():
    from bitdelta_amd.serving_loop import NO_BANS, TenantDecoder, TenantSession
    plain = _bare(False)
    assert plain._ban_params(0, (), 0) == NO_BANS and plain._ban_params(0, None, 0) == NO_BANS and plain._ban_params(0, [], 0) == NO_BANS
    for a in ((2, (), 0), (0, [[1]], 0), (0, (), 1)):
        with pytest.raises(ValueError, match="bans=True"):
            plain._ban_params(*a)
    for a in ((True, (), 0), (0, [[]], 0), (0, (), -1)):                                   # invalid values are refused as such everywhere
        with pytest.raises(ValueError):
            plain._ban_params(*a)
    on = _bare(True)
    assert on._ban_params(2, [[3, 4], (5,)], 7) == (2, ((3, 4), (5,)), 7)
    for a in ((0, [[512]], 0), (0, [[1]] * 17, 0), (0, [[1] * 9], 0), (9, (), 0)):         # the session's vocabulary and sizes
        with pytest.raises(ValueError):
            on._ban_params(*a)
    for fn in (TenantSession.submit, TenantSession.extend, TenantSession.submit_all):
        p = inspect.signature(fn).parameters
        assert (p["no_repeat_ngram_size"].default, p["bad_words"].default, p["min_new_tokens"].default) == (0, (), 0)
    p = inspect.signature(TenantDecoder.session).parameters
    assert (p["bans"].default, p["max_bad_words"].default, p["max_bad_word_len"].default) == (False, 16, 8)
    assert "bans=True" in TenantSession.__doc__


def test_submit_all_takes_one_value_or_one_per_tenant():
    s = _bare(True, T=2)
    one = [[5, 6], [7]]
    assert s._per_tenant_bad_words(one) == [one, one] and s._per_tenant_bad_words(()) == [(), ()]
    per = [[[5, 6]], [[7], [8, 9]]]
    assert s._per_tenant_bad_words(per) == per and s._per_tenant_bad_words([[[5]], []]) == [[[5]], []]
    with pytest.raises(ValueError, match="for 2 tenants"):
        s._per_tenant_bad_words([[[5]], [[6]], [[7]]])
    assert s._per_tenant(3) == [3, 3] and s._per_tenant([2, 0]) == [2, 0]
    with pytest.raises(ValueError, match="for 2 tenants"):
        s._per_tenant([1, 2, 3])


def test_session_sizes_are_validated_against_the_abi_maxima():
    from bitdelta_amd.serving_loop import TenantSession
    for kw in (dict(max_bad_words=0), dict(max_bad_words=65), dict(max_bad_word_len=0), dict(max_bad_word_len=33), dict(max_bad_words=True),
               dict(max_bad_word_len=2.0)):
        with pytest.raises(ValueError, match="max_bad_word"):
            TenantSession(None, bans=True, **kw)                                            # refused before the decoder is looked at
    with pytest.raises(ValueError, match="stop ids"):
        TenantSession(None, max_stop_ids=65, bans=True)


# ------------------------------------------------------------------------------------------------ 4. the symbols and their argument checks
NAMES = {"bd_srv_ban_rows": 23, "bd_srv_step_ban": 24}


def test_limits_and_symbols_in_header_library_ctypes_table_and_integration_notes():
    from bitdelta_amd import _lib, serving_ops
    src = open(os.path.join(ROOT, "include", "bitdelta_hip.h")).read()
    for macro, value in (("BD_BAN_NGRAM_MAX", serving_ops.BAN_NGRAM_MAX), ("BD_BAN_WORDS_MAX", serving_ops.BAN_WORDS_MAX),
                         ("BD_BAN_WORD_LEN_MAX", serving_ops.BAN_WORD_LEN_MAX), ("BD_BAN_STOP_MAX", serving_ops.BAN_STOP_MAX)):
        assert re.search(r"#define\s+%s\s+%d\b" % (macro, value), src), macro
    assert (serving_ops.BAN_NGRAM_MAX, serving_ops.BAN_WORDS_MAX, serving_ops.BAN_WORD_LEN_MAX) == (8, 64, 32) and ref.NGRAM_MAX == 8
    txt = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    notes = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name, arity in NAMES.items():
        decl = re.search(r"\bint\s+%s\s*\(([^;]*)\)\s*;" % name, txt)
        assert decl, name + " is not declared in include/bitdelta_hip.h"
        assert name in _lib.SIGNATURES and len(_lib.SIGNATURES[name][1]) == len(decl.group(1).split(",")) == arity
        assert name in notes and hasattr(_lib.lib(), name)
    assert callable(serving_ops.ban_rows) and callable(serving_ops.step_ban)


@pytest.mark.parametrize("step", [False, True], ids=["rows", "step"])
def test_entry_points_validate_before_any_device_call(step):
    """every call below is one the entry point refuses, or answers with R == 0, before any device call: none passes a complete valid argument
    list"""
    from bitdelta_amd import _lib
    L = _lib.lib()
    buf = ctypes.create_string_buffer(1 << 12)
    base = (ctypes.addressof(buf) + 255) & ~255            # an aligned, non-null host address: never dereferenced by the checks
    BAD_SHAPE, BAD_DTYPE, NULL = (L.bd_srv_rope(None, None, None, -1, 1, 128, 0, 1, 0, 0, None), L.bd_srv_rope(None, None, None, 1, 1, 128, 0, 1, 0, 7, None),
                                  L.bd_srv_rope(None, None, None, 1, 1, 128, 0, 1, 0, 0, None))
    assert len({BAD_SHAPE, BAD_DTYPE, NULL, 0}) == 4
    good = dict(logits=base, sl=72, V=64, out=base, so=64, ctx=base, Lc=40, ctx_len=base, toks=base, s_tok=48, tok_cap=40, n=base, ban_ngram=base,
                ban_tok=base, ban_len=base, Q=16, W=8, ban_min=base, stop_ids=base, ns=2, active=base, R=3, dtype=0)
    order = ["logits", "sl", "V", "out", "so", "ctx", "Lc", "ctx_len", "toks", "s_tok", "tok_cap", "n", "ban_ngram", "ban_tok", "ban_len", "Q", "W",
             "ban_min", "stop_ids", "ns"] + (["active"] if step else []) + ["R", "dtype"]
    fn = L.bd_srv_step_ban if step else L.bd_srv_ban_rows
    ptrs = ["logits", "out", "ctx", "ctx_len", "toks", "n", "ban_ngram", "ban_tok", "ban_len", "ban_min", "stop_ids"] + (["active"] if step else [])
    nulls = {q: None for q in ptrs}

    def call(**kw):
        a = dict(good, **kw)
        assert len(kw) >= 1                                # never the complete valid list
        return fn(*[a[k] for k in order], None)
    # 1. R and V
    assert call(R=-1) == BAD_SHAPE and call(V=0) == BAD_SHAPE and call(V=(1 << 22) + 8, sl=(1 << 22) + 8, so=(1 << 22) + 8) == BAD_SHAPE
    assert call(R=-1, dtype=7, **nulls) == BAD_SHAPE                                       # ... before anything else
    # 2. the dtype, in front of the sizes and the pointers
    assert call(dtype=2) == BAD_DTYPE and call(dtype=7, Q=0, **nulls) == BAD_DTYPE
    # 3. R == 0: nothing is launched, whatever the rest is
    assert call(R=0) == 0 and call(R=0, Q=0, **nulls) == 0 and call(R=0, logits=base + 2) == 0
    # 4. the sizes
    for kw in (dict(Q=0), dict(Q=65), dict(W=0), dict(W=33), dict(ns=-1), dict(ns=65), dict(Lc=-1), dict(tok_cap=-1), dict(s_tok=39),
               dict(Lc=2 ** 31 - 1, tok_cap=1, s_tok=1), dict(R=65536)):
        assert call(**kw) == BAD_SHAPE, kw
        assert call(**dict(kw, **nulls)) == BAD_SHAPE, kw                                  # ... in front of the pointers
    # 5. null pointers, in front of the alignment
    need = [q for q in ptrs if q not in ("toks", "n")] + (["n", "toks"] if step else ["toks"])
    for q in need:
        assert call(**{q: None}) == NULL, q
        assert call(**{q: None, "V": 60}) == NULL, q
    assert call(logits=None, out=base + 2) == NULL
    if not step:
        assert call(n=None, toks=None, logits=None) == NULL                                # n absent: toks is not needed, the rest still is
        assert call(n=None, toks=None, V=60) == BAD_SHAPE                                  # ... and the call gets past the pointer checks
    assert call(Lc=0, ctx=None, V=60) == BAD_SHAPE and call(ns=0, stop_ids=None, V=60) == BAD_SHAPE      # not needed: past the pointer checks
    assert call(tok_cap=0, s_tok=0, toks=None, V=60) == BAD_SHAPE
    # 6. shape of the rows and alignment
    for kw in (dict(V=60), dict(sl=60), dict(so=60), dict(sl=76), dict(so=68), dict(logits=base + 8), dict(out=base + 8)):
        assert call(**kw) == BAD_SHAPE, kw
    for q in ("toks", "n", "stop_ids"):
        assert call(**{q: base + 4}) == BAD_SHAPE, q
    for q in ("ctx", "ctx_len", "ban_ngram", "ban_tok", "ban_len", "ban_min"):
        assert call(**{q: base + 2}) == BAD_SHAPE, q
    # the largest sizes get past the range checks to the ones behind them
    assert call(Q=64, W=32, ns=64, R=65535, logits=None) == NULL
