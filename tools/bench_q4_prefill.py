#!/usr/bin/env python3
"""The 4-bit GPTQ base at more than one row per tenant: bd_binary_linear_q4 on the tile-major nibbles (arm A) against (B) what a 4-bit decoder
ran before it, binary_linear on the reference-dequantised 16-bit weight, and (C) bd_binary_linear_w8 on an int8 base of the same shape.  The four
Llama-2-7B Linear shapes (fused q|k|v, o, fused gate|up, down) at M = 2048 (B = 1), 6 x 64 and 6 x 8, fp16 and bf16.  Same process, each arm
replayed from a captured graph, arms alternated (A B C A' B' C'): the A/A spread is printed, and a row is a WIN / LOSS only beyond spread + 1 %.
The environment variable BD_Q4_TILES=1 / 2 forces the column tiles per wave of arm A (the two-tile A/B: run the tool once with each and compare
the A columns; arm B is the common yardstick of the two runs).  Then torch.cuda.memory_allocated of a 4-layer Llama-2-geometry 4-bit decoder
with the 16-bit base (base_gptq4=True) and without it ("only")."""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from bench_w8_prefill import DEV, ROWS, SHAPES, graph_us
from bitdelta_amd.binary_gemm_kernel import binary_linear
from bitdelta_amd.quant import (dequantize_base_gptq4, pack_gptq4_params, quantize_base_gptq4, quantize_base_int8, tile_weight_gptq4,
                                tile_weight_int8, weight_scale)
from bitdelta_amd.serving_loop import TenantDecoder


def verdict(ratio, spread):
    return "WIN" if ratio < 1 - spread - 0.01 else "LOSS" if ratio > 1 + spread + 0.01 else "parity"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--out", default=None)
    ap.add_argument("--dtypes", default="float16,bfloat16")
    ap.add_argument("--no-footprint", action="store_true")
    args = ap.parse_args()
    gen = torch.Generator(device=DEV).manual_seed(0)
    lines = ["BD_Q4_TILES=%s" % os.environ.get("BD_Q4_TILES", "(plan)"),
             "dtype    shape        B x M       q4 us   16-bit us   int8 us   A/A spread   q4/16-bit  verdict   q4/int8  verdict"]
    for dname in args.dtypes.split(","):
        dt = getattr(torch, dname)
        for name, N, K in SHAPES:
            w = (torch.randn(N, K, device=DEV, generator=gen) * 0.02).to(dt)
            qw, qz, sc = quantize_base_gptq4(w, 128)
            w16, w4, gp = dequantize_base_gptq4(qw, qz, sc, dt), tile_weight_gptq4(qw), pack_gptq4_params(qz, sc)
            cb, scb = quantize_base_int8(w)
            w8, ws = tile_weight_int8(cb), weight_scale(scb)
            del w, cb, qw
            for B, M in ROWS:
                x = torch.randn(B, M, K, device=DEV, generator=gen).to(dt)
                mask = torch.randint(-2 ** 31, 2 ** 31 - 1, (B, K // 32, N), generator=gen, dtype=torch.int32, device=DEV)
                alpha = torch.rand(B, 1, device=DEV, generator=gen) * 1e-3
                ya, yb, yc = (torch.empty(B, M, N, device=DEV, dtype=dt) for _ in range(3))
                a = graph_us(lambda: binary_linear(x, w4, mask, alpha, group_params=gp, group_size=128, out=ya), args.reps)
                b = graph_us(lambda: binary_linear(x, w16, mask, alpha, out=yb), args.reps)
                c = graph_us(lambda: binary_linear(x, w8, mask, alpha, weight_scale=ws, out=yc), args.reps)
                a1, b1, c1, a2, b2, c2 = a(), b(), c(), a(), b(), c()
                ta, tb, tc = min(a1, a2), min(b1, b2), min(c1, c2)
                spread = max(abs(a1 - a2) / ta, abs(b1 - b2) / tb, abs(c1 - c2) / tc)
                lines.append("%-8s %-8s %5d x %-5d %9.1f %11.1f %9.1f %11.1f%% %10.3f  %-7s %9.3f  %s" %
                             (dname, name, B, M, ta, tb, tc, 100 * spread, ta / tb, verdict(ta / tb, spread), ta / tc, verdict(ta / tc, spread)))
                print(lines[-1], flush=True)
            del w16, w4, w8
    torch.cuda.empty_cache()
    cfg = (4096, 11008, 4, 32, 32, 32000)
    for mode in (() if args.no_footprint else (True, "only")):
        base = torch.cuda.memory_allocated()
        dec = TenantDecoder.synthetic(cfg, 2, DEV, dtype=torch.float16, shared_heads=True, base_gptq4=mode)
        lines.append("4-layer Llama-2-7B geometry, 2 tenants, base_gptq4=%r: %.2f GB allocated" % (mode, (torch.cuda.memory_allocated() - base) / 1e9))
        print(lines[-1], flush=True)
        del dec
        torch.cuda.empty_cache()
    if args.out:
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
