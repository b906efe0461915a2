#!/usr/bin/env python3
"""What a sliding window buys the attention launches of a long conversation: device time per launch, a chain of launches inside ONE captured graph
(tools/bench_tenant_rope_step.py's kernel_us), every arm twice and alternated so that the pair's own spread stands next to the differences.

    python tools/bench_sliding_window.py > profiles/sliding_window_step.txt

Decode (6-tenant Mistral-7B geometry, 32 query / 8 kv heads, Lc = 16384, lockstep form):
    window      pos = 16127, W = 4096     streams rows 12032 .. 16127
    full        pos = 16127, no window    streams the whole conversation
    full_4096   pos = 4095, no window     streams 4096 rows as well: the windowed launch should stand here
Chunk (prefill_chunk's attention launch: 512 query rows at q0 = 8192 over the same caches):
    chunk_window  W = 4096                chunk_full  no window
Before timing, the windowed outputs are compared with the un-windowed entry run on a cache whose rows below the window are marked invalid
(decode) / hidden behind kv_start (chunk, last row only): the arms must be computing the window they claim."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tenants", type=int, default=6)
    ap.add_argument("--cache-len", type=int, default=16384)
    ap.add_argument("--pos", type=int, default=16127)
    ap.add_argument("--window", type=int, default=4096)
    ap.add_argument("--chunk", type=int, default=512)
    ap.add_argument("--chunk-q0", type=int, default=8192)
    ap.add_argument("--kernel-iters", type=int, default=100)
    args = ap.parse_args()
    from bitdelta_amd import serving_ops as ops
    from bitdelta_amd.serving_loop import _rope_tables
    dev = torch.device("cuda", 0)
    T, Lc, W, heads, kvh = args.tenants, args.cache_len, args.window, 32, 8
    g = torch.Generator().manual_seed(4321)
    cos, sin = _rope_tables(Lc, 128, dev, torch.float16)
    qkv = torch.randn(T, 1, (heads + 2 * kvh) * 128, generator=g).half().to(dev)
    kc = torch.randn(T, kvh, Lc, 128, generator=g).half().to(dev)
    vc = torch.randn(T, kvh, Lc, 128, generator=g).half().to(dev)
    valid = torch.ones(T, Lc, dtype=torch.bool, device=dev)
    pos = torch.tensor([args.pos], dtype=torch.long, device=dev)
    pos_w = torch.tensor([W - 1], dtype=torch.long, device=dev)
    qc = torch.randn(T, args.chunk, heads, 128, generator=g).half().to(dev)
    q0 = args.chunk_q0

    # the arms compute what they claim (the append rewrites row pos with the same bits every launch, so the caches are stable under timing)
    hidden = valid.clone()
    hidden[:, :args.pos + 1 - W] = False
    a = ops.decode_attention(qkv, cos, sin, kc, vc, valid, pos, heads, kvh, window=W)
    b = ops.decode_attention(qkv, cos, sin, kc, vc, hidden, pos, heads, kvh)
    decode_err = float((a.float() - b.float()).abs().max())
    last = q0 + args.chunk - 1
    kvs = torch.full((T,), last - W + 1, dtype=torch.int32, device=dev)
    a = ops.prefill_attention_cached(qc, kc, vc, q0, window=W)[:, -1]
    b = ops.prefill_attention_cached(qc, kc, vc, q0, kv_start=kvs)[:, -1]
    chunk_err = float((a.float() - b.float()).abs().max())
    assert decode_err < 2e-3 and chunk_err < 2e-3, (decode_err, chunk_err)

    side = torch.cuda.Stream(device=dev)

    def kernel_us(fn):
        """--kernel-iters launches in a row inside ONE captured graph (no host in the loop): replay time / launches, median of 5 replays"""
        side.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.stream(side):
            for _ in range(3):
                fn()
        torch.cuda.synchronize()
        gr = torch.cuda.CUDAGraph()
        with torch.cuda.graph(gr, stream=side):
            for _ in range(args.kernel_iters):
                fn()
        gr.replay()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        times = []
        for _ in range(5):
            e0.record()
            gr.replay()
            e1.record()
            torch.cuda.synchronize()
            times.append(e0.elapsed_time(e1) / args.kernel_iters * 1e3)
        return sorted(times)[len(times) // 2]
    arms = {
        "decode/window": lambda: ops.decode_attention(qkv, cos, sin, kc, vc, valid, pos, heads, kvh, window=W),
        "decode/full": lambda: ops.decode_attention(qkv, cos, sin, kc, vc, valid, pos, heads, kvh),
        "decode/full_%d" % W: lambda: ops.decode_attention(qkv, cos, sin, kc, vc, valid, pos_w, heads, kvh),
        "chunk/window": lambda: ops.prefill_attention_cached(qc, kc, vc, q0, window=W),
        "chunk/full": lambda: ops.prefill_attention_cached(qc, kc, vc, q0),
    }
    us = {}
    for rep in ("", "_b"):                                  # each twice, alternated: the pair's own spread
        for n, fn in arms.items():
            us[n + rep] = kernel_us(fn)
    mean = lambda n: (us[n] + us[n + "_b"]) / 2
    spread = max(abs(us[n + "_b"] / us[n] - 1) * 100 for n in arms)
    out = {"tenants": T, "heads": heads, "kv_heads": kvh, "cache_len": Lc, "pos": args.pos, "window": W, "chunk": args.chunk, "chunk_q0": q0,
           "kernel_iters": args.kernel_iters, "launch_us_in_graph": {n: round(v, 3) for n, v in us.items()}, "repeat_spread_pct": spread,
           "decode_window_over_full_pct": (mean("decode/window") / mean("decode/full") - 1) * 100,
           "decode_window_over_full_%d_pct" % W: (mean("decode/window") / mean("decode/full_%d" % W) - 1) * 100,
           "chunk_window_over_full_pct": (mean("chunk/window") / mean("chunk/full") - 1) * 100,
           "decode_max_abs_diff": decode_err, "chunk_max_abs_diff": chunk_err}
    print(json.dumps(out))
    for n, v in us.items():
        print(f"# {n:24s} {v:9.3f} us per launch (a chain of launches in one graph)", file=sys.stderr)
    print(f"# largest repeat spread {spread:.2f} %;  decode window / full {out['decode_window_over_full_pct']:+.1f} %, window / full at pos {W - 1} "
          f"{out['decode_window_over_full_%d_pct' % W]:+.2f} %;  chunk window / full {out['chunk_window_over_full_pct']:+.1f} %", file=sys.stderr)


if __name__ == "__main__":
    main()
