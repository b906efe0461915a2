#!/usr/bin/env python3
"""The int8 base at more than one row per tenant: bd_binary_linear_w8 on the tile-major bytes (arm A) against what an int8 decoder ran
before it, binary_linear on the reference-dequantised 16-bit weight (arm B).  The four Llama-2-7B Linear shapes (fused q|k|v, o, fused
gate|up, down) at M = 2048 (B = 1), 6 x 64 and 6 x 8, fp16.  Same process, each arm replayed from a captured graph, arms alternated
(A B A' B'): the A/A spread is printed, and a shape is a WIN / LOSS only beyond spread + 1 %.  Then torch.cuda.memory_allocated of a 4-layer
Llama-2-geometry int8 decoder with and without the 16-bit base (dense_base)."""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from bitdelta_amd.binary_gemm_kernel import binary_linear
from bitdelta_amd.quant import dequantize_base_int8, quantize_base_int8, tile_weight_int8, weight_scale
from bitdelta_amd.serving_loop import TenantDecoder

DEV = "cuda:0"
SHAPES = (("qkv", 12288, 4096), ("o", 4096, 4096), ("gate_up", 22016, 4096), ("down", 4096, 11008))
ROWS = ((1, 2048), (6, 64), (6, 8))


def graph_us(fn, reps, per_graph=10):
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        for _ in range(3):                # on the capture stream: its persistent workspace exists before the capture starts
            fn()
        s.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):
            for _ in range(per_graph):
                fn()
        g.replay()
        s.synchronize()

    def once():
        ts = []
        with torch.cuda.stream(s):
            for _ in range(reps):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(s)
                g.replay()
                e1.record(s)
                s.synchronize()
                ts.append(e0.elapsed_time(e1) / per_graph * 1e3)
        return sorted(ts)[len(ts) // 2]
    return once


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    gen = torch.Generator(device=DEV).manual_seed(0)
    lines = ["shape        B x M      int8 us   16-bit us   A/A spread   int8 / 16-bit   verdict"]
    for name, N, K in SHAPES:
        w = (torch.randn(N, K, device=DEV, generator=gen) * 0.02).half()
        cb, scb = quantize_base_int8(w)
        w16, w8, ws = dequantize_base_int8(cb, scb, torch.float16), tile_weight_int8(cb), weight_scale(scb)
        del w, cb
        for B, M in ROWS:
            x = torch.randn(B, M, K, device=DEV, generator=gen).half()
            mask = torch.randint(-2 ** 31, 2 ** 31 - 1, (B, K // 32, N), generator=gen, dtype=torch.int32, device=DEV)
            alpha = torch.rand(B, 1, device=DEV, generator=gen) * 1e-3
            ya, yb = torch.empty(B, M, N, device=DEV, dtype=torch.float16), torch.empty(B, M, N, device=DEV, dtype=torch.float16)
            a = graph_us(lambda: binary_linear(x, w8, mask, alpha, weight_scale=ws, out=ya), args.reps)
            b = graph_us(lambda: binary_linear(x, w16, mask, alpha, out=yb), args.reps)
            a1, b1, a2, b2 = a(), b(), a(), b()
            ta, tb = min(a1, a2), min(b1, b2)
            spread = max(abs(a1 - a2) / ta, abs(b1 - b2) / tb)
            ratio = ta / tb
            verdict = "WIN" if ratio < 1 - spread - 0.01 else "LOSS" if ratio > 1 + spread + 0.01 else "parity"
            lines.append("%-8s %5d x %-5d %9.1f %11.1f %11.1f%% %13.3f     %s" % (name, B, M, ta, tb, 100 * spread, ratio, verdict))
            print(lines[-1], flush=True)
        del w16, w8
    torch.cuda.empty_cache()
    cfg = (4096, 11008, 4, 32, 32, 32000)
    for dense in (True, False):
        base = torch.cuda.memory_allocated()
        dec = TenantDecoder.synthetic(cfg, 2, DEV, dtype=torch.float16, shared_heads=True, base_int8=True, dense_base=dense)
        lines.append("4-layer Llama-2-7B geometry, 2 tenants, base_int8, dense_base=%s: %.2f GB allocated" %
                     (dense, (torch.cuda.memory_allocated() - base) / 1e9))
        print(lines[-1], flush=True)
        del dec
        torch.cuda.empty_cache()
    if args.out:
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
