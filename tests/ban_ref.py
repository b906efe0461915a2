"""The definition of bd_srv_ban_rows / bd_srv_step_ban (include/bitdelta_hip.h) restated in plain Python on host integers, and helpers for the
tests that hold the kernel and the session to it.  Nothing here imports the package."""
import torch

NEG_INF_BITS = {torch.float16: -1024, torch.bfloat16: -128}      # 0xFC00 / 0xFF80 as int16
NGRAM_MAX = 8


def banned_ngram(h, g):
    """the tokens a no-repeat n-gram size g bans after the history h"""
    h, m = list(h), len(h)
    if g < 1 or m < g - 1:
        return set()
    tail = h[m - g + 1:]                                                 # g - 1 tokens
    return {h[i + g - 1] for i in range(0, m - g + 1) if h[i:i + g - 1] == tail}


def banned_words(h, words):
    """the tokens the bad words ban after the history h: a word's last token, when the word has one token or the history ends with the rest"""
    h, m = list(h), len(h)
    out = set()
    for q in words:
        q, L = list(q), len(q)
        if L == 1 or (L > 1 and m >= L - 1 and h[m - L + 1:] == q[:L - 1]):
            out.add(q[L - 1])
    return out


def banned(h, g=0, words=(), n=0, min_new=0, stops=()):
    """the banned set after the history h (the conversation's real tokens, then the n tokens this turn has emitted): the union of the three parts"""
    out = banned_ngram(h, g) | banned_words(h, words)
    if n < min_new:
        out |= {s for s in stops if s >= 0}
    return out


def clamp_row(ctx_row, ctx_len, toks_row, n, g, tok_rows, lens, W):
    """what the kernel makes of a row's device values: (history, g, words) with ctx_len clamped into [0, Lc], n into [0, cap], a g outside 0 .. 8
    switched off and a length outside 0 .. W an unused slot"""
    cl = min(max(int(ctx_len), 0), len(ctx_row))
    nn = 0 if n is None else min(max(int(n), 0), len(toks_row))
    h = [int(v) for v in ctx_row[:cl]] + [int(v) for v in toks_row[:nn]]
    g = int(g) if 1 <= int(g) <= NGRAM_MAX else 0
    words = [[int(v) for v in row[:L]] for row, L in zip(tok_rows, lens) if 1 <= int(L) <= W]
    return h, nn, g, words


def mask(logits, ctx, ctx_len, toks, n, ngram, ban_tok, ban_len, ban_min, stops, active=None, out=None):
    """bd_srv_ban_rows (active None) / bd_srv_step_ban on CPU tensors and lists: logits [R, V] 16-bit; ctx [R][Lc], ctx_len [R]; toks [R][cap] and
    n [R], or n None; ngram [R]; ban_tok [R][Q][W], ban_len [R][Q]; ban_min [R]; stops [R][ns].  Returns the output rows, bits exact; an
    inactive row keeps what `out` held."""
    R, V = logits.shape
    res = logits.clone() if out is None else out.clone()
    bits = res.view(torch.int16)
    src = logits.view(torch.int16)
    for r in range(R):
        if active is not None and not active[r]:
            continue
        W = len(ban_tok[r][0])
        h, nn, g, words = clamp_row(ctx[r], ctx_len[r], toks[r] if n is not None else [], None if n is None else n[r], ngram[r], ban_tok[r],
                                    ban_len[r], W)
        b = banned(h, g, words, nn, int(ban_min[r]), [int(s) for s in stops[r]])
        bits[r] = src[r]
        idx = [v for v in b if 0 <= v < V]
        if idx:
            bits[r, torch.tensor(idx)] = NEG_INF_BITS[logits.dtype]
    return res


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.contiguous().view(torch.int16), b.contiguous().view(torch.int16))


def repeats_ngram(seq, g):
    """whether some g-gram occurs twice in seq"""
    seen = set()
    for i in range(len(seq) - g + 1):
        k = tuple(seq[i:i + g])
        if k in seen:
            return True
        seen.add(k)
    return False


def completes_word(conv, turn, words):
    """whether some emitted token of `turn` completes a bad word over conv + turn"""
    h = list(conv)
    for y in turn:
        if y in banned_words(h, words):
            return True
        h.append(y)
    return False
