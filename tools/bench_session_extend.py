#!/usr/bin/env python3
"""The second turn of a conversation: TenantSession.extend (prefill of the new tokens alone, behind the keys the session kept) against the route it
replaces, a submit of the whole conversation (what the reference does with every request, demo/demo_backend.py:261-315).

1. ADMISSION LATENCY, host clock around the call and a device synchronise (the call ends in a host read of its first token either way), fp16,
   6 tenant slots, one tenant served: conversations of about 200 / 500 / 900 tokens, new turns of 16 / 64 tokens.  One Mistral-7B layer
   (mistral-1layer shapes, small vocabulary) and the same with two layers: `layer` = the difference, `x32` = one-layer time + 31 x layer, the
   32-layer model's admission by extrapolation.  Arms alternate (A B A' B'), median of --reps each; both passes are printed (the A/A spread).
   `extend` is measured on both attention arms: bd_srv_prefill_attention_cached, and the stock ops (hip_prefill_attention = False).
2. THE ATTENTION OF ONE LAYER alone, 32 / 8 heads, one tenant, at the same positions: RoPE + cache append + attention by the two HIP launches
   (rope_kv_append + prefill_attention_cached; its grid is heads x ceil(Sq / 128) workgroups) against the stock-op arm of TenantDecoder._layer
   (rope, two index_copy_, SDPA over the [1, 1, Sq, Lc] mask).  `eager`: device events around 20 back-to-back calls (launch overhead included, as
   a prefill runs); `graph`: the same 20 calls replayed from a captured graph (device time).  A row where the HIP arm is slower says LOSES."""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import torch.nn.functional as F

from bitdelta_amd import serving_ops as ops
from bitdelta_amd.serving_loop import MODEL_CONFIGS, TenantDecoder, _rope, _rope_tables, padded_length

DEV = "cuda:0"
MAX_LEN = 1152            # a 900-token conversation is padded to 1024 rows by its first submit; its next turn goes behind them


def median(v):
    return sorted(v)[len(v) // 2]


def host_ms(fn, reps, reset=None, warm=2):
    ts = []
    for i in range(warm + reps):
        if reset is not None:
            reset()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        if i >= warm:
            ts.append((time.perf_counter() - t0) * 1e3)
    return median(ts)


def admission(dec, C, n, reps, gen):
    """(extend hip, extend stock, submit) x two passes, ms"""
    t = 2
    history = torch.randint(1, 500, (C,), generator=gen).tolist()
    new = torch.randint(1, 500, (n,), generator=gen).tolist()
    sess = dec.session()
    sess.submit(t, history, max_new_tokens=1)              # the first turn: retired at admission, its rows stay
    keep = [v.clone() for v in sess._state()]
    last = int(sess.tok[t, 0])

    def reset():
        for v, k in zip(sess._state(), keep):
            v.copy_(k)

    def extend(hip):
        def run():
            dec.hip_prefill_attention = hip
            try:
                sess.extend(t, new, max_new_tokens=1)
            finally:
                dec.hip_prefill_attention = True
        return run
    whole = history + [last] + new                          # what the reference would be sent for the second turn
    submit = lambda: sess.submit(t, whole, max_new_tokens=1)
    out = []
    for _ in range(2):
        out.append((host_ms(extend(True), reps, reset), host_ms(extend(False), reps, reset), host_ms(submit, reps)))
        sess.submit(t, history, max_new_tokens=1)              # (the submit arm replaced the conversation: the first turn again)
        keep = [v.clone() for v in sess._state()]
    return out, padded_length(C), padded_length(len(whole))


def events_us(fn, reps, per=20):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(per):
            fn()
        e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1) / per * 1e3)
    return median(ts)


def graph_us(fn, reps, per=20):
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        for _ in range(3):
            fn()
        s.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):
            for _ in range(per):
                fn()
        g.replay()
        s.synchronize()
        ts = []
        for _ in range(reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(s)
            g.replay()
            e1.record(s)
            s.synchronize()
            ts.append(e0.elapsed_time(e1) / per * 1e3)
    return median(ts)


def attention_layer(q0, Sq, reps, gen, cos, sin):
    """us per layer: (hip eager, stock eager, hip graph, stock graph) x two passes"""
    _, _, _, heads, kvh, _ = MODEL_CONFIGS["mistral-1layer"]
    hd, T = 128, 1
    qkv0 = torch.randn(T, Sq, (heads + 2 * kvh) * hd, device=DEV, generator=gen).half()
    ck = torch.randn(T, kvh, MAX_LEN, hd, device=DEV, generator=gen).half()
    cv = torch.randn(T, kvh, MAX_LEN, hd, device=DEV, generator=gen).half()
    kvs = torch.zeros(T, dtype=torch.int32, device=DEV)
    pos_idx = torch.arange(q0, q0 + Sq, device=DEV)
    mask = (torch.arange(MAX_LEN, device=DEV)[None, :] <= pos_idx[:, None])[None, None]
    nq, nk = heads * hd, kvh * hd

    def hip():
        qkv = qkv0.clone()
        ops.rope_kv_append_(qkv, cos, sin, ck, cv, heads, kvh, q0)
        return ops.prefill_attention_cached(qkv[..., :nq].view(T, Sq, heads, hd), ck, cv, q0, kv_start=kvs)

    def stock():
        qkv = qkv0.clone()
        q, k, v = qkv.split([nq, nk, nk], dim=-1)
        c, s_ = cos[pos_idx], sin[pos_idx]
        q = _rope(q.view(T, Sq, heads, hd).transpose(1, 2), c, s_)
        k = _rope(k.view(T, Sq, kvh, hd).transpose(1, 2), c, s_)
        ck.index_copy_(2, pos_idx, k)
        cv.index_copy_(2, pos_idx, v.view(T, Sq, kvh, hd).transpose(1, 2))
        a = F.scaled_dot_product_attention(q, ck, cv, attn_mask=mask, enable_gqa=True)
        return a.transpose(1, 2).reshape(T, Sq, heads * hd)
    err = float((hip().float() - stock().float()).abs().max())
    out = [(events_us(hip, reps), events_us(stock, reps), graph_us(hip, reps), graph_us(stock, reps)) for _ in range(2)]
    return out, err


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--out", default=None, help="also write the table to this file")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "a measurement needs the device"
    gen = torch.Generator().manual_seed(0)
    cases = [(C, n) for C in (200, 500, 900) for n in (16, 64)]
    lines = ["second-turn admission, Mistral-7B layer shapes, fp16, 6 slots, one tenant served; ms = host clock around the call + synchronise, median of %d;"
             % a.reps, "two passes per arm, arms alternating (the A/A spread); rows = cache rows the call prefills",
             "%-6s %-5s %-4s | %-11s %-11s | %23s | %23s | %23s | %s" % ("layers", "conv", "new", "extend rows", "submit rows", "extend hip ms (A/A)",
                                                                        "extend stock ms (A/A)", "submit ms (A/A)", "submit / extend hip")]
    res = {}
    for nl in (1, 2):
        dec = TenantDecoder.synthetic("mistral-1layer", 6, DEV, dtype=torch.float16, seed=3, layers=nl, max_len=MAX_LEN)
        for C, n in cases:
            r, rows_first, rows_submit = admission(dec, C, n, a.reps, gen)
            res[(nl, C, n)] = r
            best = [min(x[i] for x in r) for i in range(3)]
            lines.append("%-6d %-5d %-4d | %-11d %-11d | %10.2f (%10.2f) | %10.2f (%10.2f) | %10.2f (%10.2f) | %.2fx%s"
                         % (nl, C, n, n + 1, rows_submit, r[0][0], r[1][0], r[0][1], r[1][1], r[0][2], r[1][2], best[2] / best[0],
                            " (LOSES)" if best[2] < best[0] else ""))
        del dec
        torch.cuda.empty_cache()
    lines.append("")
    lines.append("32-layer model by extrapolation: one-layer time + 31 x (two-layer time - one-layer time), best of the two passes, ms")
    lines.append("%-5s %-4s | %12s %12s %12s | %12s %12s %12s | %s" % ("conv", "new", "layer hip", "layer stock", "layer submit", "x32 hip", "x32 stock",
                                                                       "x32 submit", "submit / extend hip"))
    for C, n in cases:
        b1 = [min(x[i] for x in res[(1, C, n)]) for i in range(3)]
        b2 = [min(x[i] for x in res[(2, C, n)]) for i in range(3)]
        layer = [y - x for x, y in zip(b1, b2)]
        x32 = [x + 31 * l for x, l in zip(b1, layer)]
        lines.append("%-5d %-4d | %12.3f %12.3f %12.3f | %12.2f %12.2f %12.2f | %.2fx" % (C, n, *layer, *x32, x32[2] / x32[0]))
    lines.append("")
    lines.append("attention of one layer (RoPE + cache append + attention), 32 / 8 heads, one tenant, Lc = %d, us per layer, median of %d, two passes (A/A)"
                 % (MAX_LEN, a.reps))
    lines.append("%-6s %-4s %-5s | %21s %21s %-16s | %21s %21s %-16s | %s" % ("q0", "Sq", "grid", "hip eager (A/A)", "stock eager (A/A)", "stock / hip",
                                                                              "hip graph (A/A)", "stock graph (A/A)", "stock / hip", "max |hip - stock|"))
    dgen = torch.Generator(device=DEV).manual_seed(1)
    cos, sin = _rope_tables(MAX_LEN, 128, torch.device(DEV), torch.float16)
    for C, n in cases:
        q0, Sq = padded_length(C), n + 1
        r, err = attention_layer(q0, Sq, a.reps, dgen, cos, sin)
        b = [min(x[i] for x in r) for i in range(4)]
        tag = lambda s_, h: "%.2fx%s" % (s_ / h, " (LOSES)" if s_ < h else "")
        lines.append("%-6d %-4d %-5d | %9.1f (%9.1f) %9.1f (%9.1f) %-16s | %9.1f (%9.1f) %9.1f (%9.1f) %-16s | %.4f"
                     % (q0, Sq, 32 * ((Sq + 127) // 128), r[0][0], r[1][0], r[0][1], r[1][1], tag(b[1], b[0]), r[0][2], r[1][2], r[0][3], r[1][3],
                        tag(b[3], b[2]), err))
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
