"""Sliding-window perplexity of T fine-tunes over one base: the reference's bitdelta/eval_ppl.py:34-85 on TenantDecoder.score.

The reference loads one model per diff and, per window, asks HF for the mean cross entropy of the window's last `window_size` tokens given up
to `context_size` tokens before them; its perplexity is exp(mean over the windows of those means).  Here the T fine-tunes score the same
window in one pass over the base weight.  Tokenising text stays with the caller: the functions take token ids."""
import math

import torch


def ppl_windows(n_tokens, context_size=1024, window_size=512):
    """The windows of eval_ppl.py:34-83 over n_tokens tokens: [(begin, end, n_targets)], tokens[begin:end] scored on its last n_targets tokens.
    stride = window_size; windows begin at 0, stride, ... below seq_len = n_tokens - n_tokens % stride; the slice runs to the real end of the
    tokens, not to seq_len; the loop stops after the first window whose nominal end reaches seq_len.  A window's first token has no prediction,
    so n_targets = min(window_size, end - begin - 1).  No window at all (n_tokens < window_size) is a ValueError."""
    n_tokens, context_size, window_size = int(n_tokens), int(context_size), int(window_size)
    if window_size < 1 or context_size < 0:
        raise ValueError("window_size >= 1 and context_size >= 0")
    max_length, stride = context_size + window_size, window_size
    seq_len = n_tokens - n_tokens % stride
    out = []
    for begin in range(0, seq_len, stride):
        end = min(begin + max_length, n_tokens)
        out.append((begin, end, min(window_size, end - begin - 1)))
        if begin + max_length >= seq_len:
            break
    if not out:
        raise ValueError("%d tokens hold no window of %d" % (n_tokens, window_size))
    return out


def perplexity(dec, token_ids, context_size=1024, window_size=512, **score_kw):
    """exp(mean over windows of the window's mean target loss), per tenant of `dec`, in fp64 (eval_ppl.py:85): a list of T floats.
    token_ids: one sequence shared by all tenants, or [T, n] (a row per tenant).  score_kw goes to dec.score (row_chunk, hip_nll)."""
    ids = torch.as_tensor(token_ids, dtype=torch.long)
    if ids.dim() == 1:
        ids = ids[None, :].expand(dec.T, -1)
    if ids.dim() != 2 or ids.shape[0] != dec.T:
        raise ValueError("token_ids: one sequence, or one row per tenant")
    ids = ids.cpu()
    means = []
    for begin, end, n_targets in ppl_windows(ids.shape[1], context_size, window_size):
        if n_targets < 1:
            raise ValueError("the window %d:%d has no token to score" % (begin, end))
        nll = dec.score(ids[:, begin:end].contiguous(), targets_from=end - begin - n_targets, **score_kw)
        means.append(torch.stack([v[-n_targets:].double().mean() for v in nll]))
    total = torch.stack(means).mean(dim=0)
    return [math.exp(v) for v in total.tolist()]
