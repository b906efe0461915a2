"""The definition of bd_srv_penalize_rows / bd_srv_step_penalize (include/bitdelta_hip.h) restated on torch CPU tensors: every fp32 operation
is one torch op (each rounded on its own), the final rounding is `.to(dtype)` (round to nearest even), and the step form's history update is
done first, as the kernel's owning thread does it.  No kernel under test is used here."""
import torch

BIT15 = -32768            # an int16 with bit 15 alone
COUNT_MAX = 32767


def history(context, counts=None, V=None):
    """an int16 history row of length V: bit 15 at the token ids of `context`, the count bits from `counts` ({id: count})"""
    h = torch.zeros(V, dtype=torch.int32)
    if len(context):
        h[torch.tensor(sorted(set(int(i) for i in context)))] = 0x8000
    for i, c in (counts or {}).items():
        h[i] |= min(int(c), COUNT_MAX)
    return bits16(h)


def bits16(x):
    """int32 values 0 .. 0xffff -> the int16 tensor with those bits"""
    x = x.to(torch.int32)
    return (x - (x >= 0x8000).to(torch.int32) * 0x10000).to(torch.int16)


def penalize(logits, hist, pen, bias_id=None, bias_val=None, tok=None, active=None, out=None):
    """(out, hist'): logits [R, V] fp16 / bf16, hist int16 [R, V], pen float32 [R, 4] = (r, r_inv, presence, frequency), bias_id int32 /
    bias_val float32 [R, nb] or None.  tok None: the rows form (every row live, hist' is hist).  Otherwise the step form: tok [R] (any shape
    with R elements) long, active [R] bool; a live row's element tok[t] is counted first (saturating) and stored; an inactive row keeps its
    hist row and its row of `out` (the previous contents of the output buffer; zeros when not given)."""
    assert logits.device.type == "cpu" and logits.dtype in (torch.float16, torch.bfloat16)
    R, V = logits.shape
    h = hist.to(torch.int32) & 0xffff
    live = torch.ones(R, dtype=torch.bool) if active is None else active.reshape(R).bool().clone()
    if tok is not None:
        tok = tok.reshape(R).tolist()
        for t in range(R):
            if live[t] and 0 <= tok[t] < V:
                c = int(h[t, tok[t]]) & 0x7fff
                h[t, tok[t]] = (int(h[t, tok[t]]) & 0x8000) | min(c + 1, COUNT_MAX)
    c = (h & 0x7fff).to(torch.float32)
    seen = h != 0
    pen = pen.to(torch.float32)
    r, r_inv, presence, frequency = (pen[:, i:i + 1] for i in range(4))
    rep = torch.isfinite(r) & (r > 0)                                    # r not in (0, inf): the repetition step is off
    presence = torch.where(torch.isnan(presence), torch.zeros_like(presence), presence)
    frequency = torch.where(torch.isnan(frequency), torch.zeros_like(frequency), frequency)
    x = logits.to(torch.float32)
    x = torch.where(seen & rep, torch.where(x > 0, x * r_inv, x * r), x)
    fc = frequency * c                                                   # one product ...
    x = x - fc                                                           # ... one subtraction
    x = torch.where(c > 0, x - presence, x)
    if bias_id is not None:
        for t in range(R):
            for j in range(bias_id.shape[1]):                            # list order: a repeated id is added twice
                i = int(bias_id[t, j])
                if 0 <= i < V:
                    x[t, i] = x[t, i] + bias_val[t, j].to(torch.float32)
    res = x.to(logits.dtype)
    if not bool(live.all()):
        keep = torch.zeros_like(res) if out is None else out
        res = torch.where(live[:, None], res, keep)
        h = torch.where(live[:, None], h, hist.to(torch.int32) & 0xffff)
    return res, bits16(h)


def same_bits(a, b):
    """two 16-bit float tensors hold the same bits, NaN elements compared as NaN (any payload)"""
    assert a.dtype == b.dtype and a.shape == b.shape
    ai, bi = a.contiguous().view(torch.int16), b.contiguous().view(torch.int16)
    both_nan = torch.isnan(a) & torch.isnan(b)
    return bool(((ai == bi) | both_nan).all())
