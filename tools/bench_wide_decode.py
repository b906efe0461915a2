#!/usr/bin/env python3
"""The decode Linear for MORE than 16 tenants: what FusedDeltaLinear.forward calls today (arm A: binary_linear, which runs consecutive
16-row launches that each stream the base weight again) against the wide launch (arm B: binary_linear_decode(layout="wide"), ONE launch).
The four Llama-2-7B Linears (fused q|k|v, o, fused gate|up, down), T = 24 / 32 / 48 / 64 tenants, fp16 and bf16.  Same process; each arm
is a chain of launches in one captured graph (tools/step_ab.kernel_timer) whose operands ROTATE over enough copies that a launch never
finds its weights or sign words in the 256-MB Infinity Cache; the arms are alternated (A B A' B'), the A/A spread is printed, and a row is a
WIN / LOSS only beyond spread + 1 %.  TB/s = the ALGORITHMIC bytes of each arm (A: ceil(T/16) x W + signs; B: W + signs) over its time."""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import torch

from bitdelta_amd.binary_gemm_kernel import binary_linear, binary_linear_decode, pack_decode_masks_wide, tile_weight
from step_ab import kernel_timer

DEV = "cuda:0"
SHAPES = (("qkv", 12288, 4096), ("o", 4096, 4096), ("gate_up", 22016, 4096), ("down", 4096, 11008))
TENANTS = (24, 32, 48, 64)
COLD_BYTES = 512e6          # traffic between two uses of one operand copy: twice the Infinity Cache


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=12, help="launches of every operand copy per captured graph")
    ap.add_argument("--shapes", default=",".join(s[0] for s in SHAPES))
    ap.add_argument("--tenants", default=",".join(map(str, TENANTS)))
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    tenants = [int(t) for t in args.tenants.split(",")]
    gen = torch.Generator(device=DEV).manual_seed(0)
    lines = ["shape     dtype   T   chunked us  (TB/s)    wide us  (TB/s)   A/A spread   wide / chunked   verdict"]
    for name, N, K in SHAPES:
        if name not in args.shapes.split(","):
            continue
        Tmax = max(tenants)
        # the fewest bytes a launch of this shape moves decide how many operand copies keep every launch cold
        copies = min(8, max(2, -(-int(COLD_BYTES) // (2 * N * K + min(tenants) * N * K // 8))))
        mask0 = torch.randint(-2 ** 31, 2 ** 31 - 1, (Tmax, K // 32, N), generator=gen, dtype=torch.int32, device=DEV)
        wide0 = pack_decode_masks_wide(mask0)          # (a T < Tmax launch reads the first ceil(T/16) groups: same bytes as its own pack)
        masks, wides = [mask0] + [mask0.clone() for _ in range(copies - 1)], [wide0] + [wide0.clone() for _ in range(copies - 1)]
        for dtype in (torch.float16, torch.bfloat16):
            w0 = (torch.randn(N, K, device=DEV, generator=gen) * 0.02).to(dtype)
            ws = [w0] + [w0.clone() for _ in range(copies - 1)]
            wts = [tile_weight(w) for w in ws]
            for T in tenants:
                x = (torch.randn(T, 1, K, device=DEV, generator=gen) * 1.5).to(dtype)
                alpha = torch.rand(T, 1, device=DEV, generator=gen) * 1e-3 + 2e-4
                ya, yb = torch.empty(T, 1, N, device=DEV, dtype=dtype), torch.empty(T, 1, N, device=DEV, dtype=dtype)
                ng = (T + 15) // 16
                turn = {"a": 0, "b": 0}

                def arm_a():
                    i = turn["a"] = (turn["a"] + 1) % copies
                    binary_linear(x, ws[i], masks[i][:T], alpha, out=ya)

                def arm_b():
                    i = turn["b"] = (turn["b"] + 1) % copies
                    binary_linear_decode(x, wts[i], wides[i][:ng], alpha, layout="wide", weight_tiled=True, out=yb)
                arm_a(), arm_b()
                torch.cuda.synchronize()
                err = ((ya.double() - yb.double()).norm() / ya.double().norm()).item()
                assert err < 2e-3, f"{name} {dtype} T={T}: the arms disagree (rel {err:.2e})"
                timer = kernel_timer(torch.device(DEV), copies * args.rounds)
                a1, b1, a2, b2 = timer(arm_a), timer(arm_b), timer(arm_a), timer(arm_b)
                ta, tb = min(a1, a2), min(b1, b2)
                spread = max(abs(a1 - a2) / ta, abs(b1 - b2) / tb)
                ratio = tb / ta
                small = 2 * T * K + 2 * T * N
                bytes_a, bytes_b = ng * 2 * N * K + T * N * K // 8 + small, 2 * N * K + T * N * K // 8 + small
                verdict = "WIN" if ratio < 1 - spread - 0.01 else "LOSS" if ratio > 1 + spread + 0.01 else "PARITY"
                lines.append("%-8s  %-5s  %2d  %10.1f  (%4.2f)  %9.1f  (%4.2f)  %9.1f%%  %15.3f   %s" %
                             (name, "fp16" if dtype == torch.float16 else "bf16", T, ta, bytes_a / ta / 1e6, tb, bytes_b / tb / 1e6,
                              100 * spread, ratio, verdict))
                print(lines[-1], flush=True)
            del ws, wts
        del masks, wides, mask0, wide0
        torch.cuda.empty_cache()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
