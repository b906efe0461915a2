"""The definition of bd_srv_constrain_rows / bd_srv_step_constrain / bd_srv_step_constrain_advance (include/bitdelta_hip.h) restated in plain
Python on lists of ints: the set a state allows, the mask, the transition and the final-state rule.  The only tensor work is the bit copy of the
16-bit logits.  No kernel under test and nothing of bitdelta_amd is used here."""
import torch

NEG_INF_BITS = {torch.float16: 0xfc00 - 0x10000, torch.bfloat16: 0xff80 - 0x10000}      # as int16 values


def _lists(x):
    return x.tolist() if isinstance(x, torch.Tensor) else x


def pack(automata, S, E, fill_tok=0):
    """per-row device-shaped arrays from a list of (off, edge_tok, edge_next, accepting) tuples of plain lists (an automaton's CSR form), padded to
    S states and E edges: returns int32 off [R, S + 1], edge_tok / edge_next [R, E] and uint8 accepting [R, S].  The padding of off repeats the
    last offset (states nobody reaches, empty), that of the edge arrays holds fill_tok / 0."""
    R = len(automata)
    off = torch.zeros(R, S + 1, dtype=torch.int32)
    tok = torch.full((R, E), fill_tok, dtype=torch.int32)
    nxt = torch.zeros(R, E, dtype=torch.int32)
    acc = torch.zeros(R, S, dtype=torch.uint8)
    for r, (o, et, en, a) in enumerate(automata):
        assert len(o) - 1 <= S and len(et) <= E and len(et) == len(en) and len(a) == len(o) - 1
        off[r, :len(o)] = torch.tensor(o, dtype=torch.int32)
        off[r, len(o):] = o[-1]
        if et:
            tok[r, :len(et)] = torch.tensor(et, dtype=torch.int32)
            nxt[r, :len(en)] = torch.tensor(en, dtype=torch.int32)
        acc[r, :len(a)] = torch.tensor(a, dtype=torch.uint8)
    return off, tok, nxt, acc


def edge_slice(off_row, s, E):
    """the clamped slice [b, e) of state s: offsets outside [0, E] are device values the host could not have written"""
    b = min(max(off_row[s], 0), E)
    e = min(max(off_row[s + 1], b), E)
    return b, e


def allowed(s, off_row, tok_row, acc_row, stops, V):
    """the set of token ids state s allows, or None when nothing is constrained (s < 0, or s >= S: a value the host could not have written)"""
    S = len(acc_row)
    if s < 0 or s >= S:
        return None
    b, e = edge_slice(off_row, s, len(tok_row))
    a = set(y for y in tok_row[b:e] if 0 <= y < V)
    if acc_row[s]:
        a |= set(y for y in (stops or []) if 0 <= y < V)
    return a


def is_final(s, off_row, acc_row, E):
    b, e = edge_slice(off_row, s, E)
    return bool(acc_row[s]) and b == e


def mask(logits, state, off, edge_tok, accepting, stop_ids=None, active=None, out=None):
    """the masked rows: logits [R, V] fp16 / bf16 (CPU); a row whose state allows a set keeps the BITS of its elements inside the set and holds
    -inf outside it; an unconstrained row is copied.  active (step form): an inactive row keeps its row of `out` (the previous contents of the
    output buffer; zeros when not given)."""
    assert logits.device.type == "cpu" and logits.dtype in NEG_INF_BITS
    R, V = logits.shape
    state, off, edge_tok, accepting = _lists(state), _lists(off), _lists(edge_tok), _lists(accepting)
    stops = _lists(stop_ids) if stop_ids is not None else [[]] * R
    live = [True] * R if active is None else [bool(a) for a in _lists(active)]
    res = logits.clone().view(torch.int16)
    for r in range(R):
        if not live[r]:
            res[r] = (torch.zeros_like(logits[r]) if out is None else out[r]).view(torch.int16)
            continue
        a = allowed(state[r], off[r], edge_tok[r], accepting[r], stops[r], V)
        if a is None:
            continue
        keep = torch.zeros(V, dtype=torch.bool)
        if a:
            keep[torch.tensor(sorted(a))] = True
        res[r][~keep] = NEG_INF_BITS[logits.dtype]
    return res.view(logits.dtype)


def advance(tok, n, c_n, state, off, edge_tok, edge_next, accepting, active, done):
    """(c_n', state', active', done') as lists: bd_srv_step_constrain_advance on host integers"""
    tok, n, c_n, state = [int(v) for v in _lists(tok.reshape(-1) if isinstance(tok, torch.Tensor) else tok)], _lists(n), list(_lists(c_n)), list(_lists(state))
    off, edge_tok, edge_next, accepting = _lists(off), _lists(edge_tok), _lists(edge_next), _lists(accepting)
    active, done = [int(bool(a)) for a in _lists(active)], [int(d) for d in _lists(done)]
    for t in range(len(state)):
        if n[t] == c_n[t]:
            continue
        c_n[t] = n[t]
        s, S, E = state[t], len(accepting[t]), len(edge_tok[t])
        if s < 0 or s >= S:
            continue
        b, e = edge_slice(off[t], s, E)
        for i in range(b, e):
            if edge_tok[t][i] == tok[t] and 0 <= edge_next[t][i] < S:
                s = edge_next[t][i]
                state[t] = s
                break
        if is_final(s, off[t], accepting[t], E) and active[t]:
            active[t] = 0
            done[t] |= 8
    return c_n, state, active, done


def same_bits(a, b):
    """two 16-bit float tensors hold exactly the same bits (NaN payloads included: the mask makes no float of a logit)"""
    assert a.dtype == b.dtype and a.shape == b.shape
    return torch.equal(a.contiguous().view(torch.int16), b.contiguous().view(torch.int16))
