"""The definition of bd_srv_step_stop_sequences (include/bitdelta_hip.h) restated in plain Python on host integers, for the tests: nothing here
imports the package.  A request carries sequences of token ids; after a step in which a tenant's count moved to n, y = out[t, 0:n] are this
turn's tokens, and
  hit   the lowest index q with 1 <= len_q <= n and y[n - len_q : n] == seq_q, or -1;
  hold  the largest k such that some q has k < len_q, k <= n and y[n - k : n] == seq_q[0:k] (0 when there is none), and 0 on a hit;
  a hit retires the tenant: active = 0, done |= 16, whatever the step end has written into done in the same step.
The prompt never takes part: the functions only ever see the turn's tokens."""


def scan(y, seqs):
    """(hit, hold) for the turn's tokens y and the request's sequences (lists of ids, in the caller's order; an empty list is an unused slot;
    a negative id matches nothing) -- by brute force over every (q, k) pair, the way the definition is worded"""
    y = [int(v) for v in y]
    n = len(y)
    hit = -1
    for q, s in enumerate(seqs):
        L = len(s)
        if 1 <= L <= n and all(int(s[j]) >= 0 and int(s[j]) == y[n - L + j] for j in range(L)):
            hit = q
            break
    if hit >= 0:
        return hit, 0
    hold = 0
    for s in seqs:
        for k in range(1, len(s)):                                       # k < len_q
            if k <= n and all(int(s[j]) >= 0 and int(s[j]) == y[n - k + j] for j in range(k)):
                hold = max(hold, k)
    return -1, hold


def table_seqs(seq_tok, seq_len, W):
    """one tenant's table rows ([Q][W] ids, [Q] lengths) as the list of sequences `scan` takes: a length outside 0 .. W counts as 0"""
    return [list(row[:l]) if 0 <= l <= W else [] for row, l in zip(seq_tok, seq_len)]


def step(out, n, ss_n, seq_tok, seq_len, hit, hold, active, done, out_cap=None):
    """The launch on host lists (one entry per tenant; out[t] = the tenant's output row, at least out_cap long): returns
    (ss_n', hit', hold', active', done') as new lists.  A tenant whose count did not move keeps every word, a stale hit included; n above the
    capacity of the row (or negative) compares nothing."""
    ss_n, hit, hold = list(ss_n), list(hit), list(hold)
    active, done = [int(bool(a)) for a in active], [int(d) for d in done]
    for t in range(len(n)):
        if n[t] == ss_n[t]:
            continue
        ss_n[t] = n[t]
        cap = len(out[t]) if out_cap is None else out_cap
        W = len(seq_tok[t][0])
        if 0 <= n[t] <= cap:
            h, k = scan(out[t][:n[t]], table_seqs(seq_tok[t], seq_len[t], W))
        else:
            h, k = -1, 0
        hit[t], hold[t] = h, k
        if h >= 0:
            active[t] = 0
            done[t] |= 16
    return ss_n, hit, hold, active, done


def first_hit(tokens, seqs):
    """A whole free-running turn cut where the session would stop it: (m, hit) with m the number of tokens after which tokens[:m] first ends
    with one of the sequences and hit its index, or (len(tokens), -1) when that never happens"""
    for m in range(1, len(tokens) + 1):
        h, _ = scan(tokens[:m], seqs)
        if h >= 0:
            return m, h
    return len(tokens), -1
