#!/usr/bin/env python3
"""Same-process A/B of the scoring tail (TenantDecoder.score's chunk loop) at the workload's shape: 6 tenants x 512 scored rows, hidden 4096,
vocabulary 32000, fp16.  Two arms on the same hidden rows and lm_head: HIP (serving_ops.token_nll on the 16-bit logits) and stock
(log_softmax(logits.float()) + gather).  Timed: the chunk as score runs it (torch.bmm + the NLL), and the NLL alone on logits that are rotated
over three buffers (590 MB: past L2 and the Infinity Cache).  The arms alternate round by round and each is measured twice per round, so the
table carries its own A/A spread; peak allocated bytes are taken per arm.  Bytes are counted from the shapes: the HIP launch reads R * V * 2.

usage: python tools/bench_score.py [--out profiles/score_nll.txt] [--tenants 6] [--rows 512] [--hidden 4096] [--vocab 32000] [--rounds 9]"""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import torch.nn.functional as F

from bitdelta_amd import serving_ops as ops

HBM_ACHIEVABLE = 6.3e12      # bytes/s: what a streaming kernel reaches on an MI355X (of 8 TB/s nominal)


def nll_hip(logits, labels):
    return ops.token_nll(logits, labels)


def nll_stock(logits, labels):
    lp = F.log_softmax(logits.float(), dim=-1)
    return torch.where(labels >= 0, -lp.gather(1, labels.clamp(min=0)[:, None])[:, 0], torch.zeros((), device=logits.device))


def timed(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for i in range(reps):
        fn(i)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps * 1e3          # us


def peak_bytes(fn):
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    fn(0)
    torch.cuda.synchronize()
    return torch.cuda.max_memory_allocated() - base


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--tenants", type=int, default=6)
    ap.add_argument("--rows", type=int, default=512)
    ap.add_argument("--hidden", type=int, default=4096)
    ap.add_argument("--vocab", type=int, default=32000)
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--reps", type=int, default=20)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_score.py measures on a ROCm device; none found")
    dev, dt = "cuda", torch.float16
    T, M, H, V = a.tenants, a.rows, a.hidden, a.vocab
    g = torch.Generator(device=dev).manual_seed(0)
    h = torch.randn(T, M, H, device=dev, generator=g).to(dt)
    head_t = (torch.randn(T, V, H, device=dev, generator=g) * 0.02).to(dt).transpose(1, 2)
    labels = torch.randint(0, V, (T * M,), device=dev, generator=g)
    labels[::17] = -100
    sets = [torch.bmm((torch.randn(T, M, H, device=dev, generator=g)).to(dt), head_t).view(T * M, V) for _ in range(3)]

    arms = {"hip": nll_hip, "stock": nll_stock}
    chunk = {k: (lambda i, f=f: f(torch.bmm(h, head_t).view(T * M, V), labels)) for k, f in arms.items()}
    alone = {k: (lambda i, f=f: f(sets[i % len(sets)], labels)) for k, f in arms.items()}
    # the arms compute the same thing at the timed size
    x, y = nll_hip(sets[0], labels), nll_stock(sets[0], labels)
    agree = float(((x.double() - y.double()).abs() / (1 + y.double().abs())).max())
    assert agree <= 2.0 ** -18, agree
    for fn in list(chunk.values()) + list(alone.values()):      # warm-up: code objects, BLAS algorithm choice, allocator
        for i in range(3):
            fn(i)
    series = {(w, k, j): [] for w in ("chunk", "alone") for k in arms for j in (0, 1)}
    for _ in range(a.rounds):
        for j in (0, 1):                                        # hip, stock, hip, stock: each arm twice per round
            for k in arms:
                series[("chunk", k, j)].append(timed(chunk[k], a.reps))
                series[("alone", k, j)].append(timed(alone[k], a.reps))
    med = {key: statistics.median(v) for key, v in series.items()}
    peaks = {k: peak_bytes(chunk[k]) for k in arms}
    bmm_us = statistics.median(timed(lambda i: torch.bmm(h, head_t), a.reps) for _ in range(a.rounds))
    read = T * M * V * 2
    lines = ["scoring tail, %d tenants x %d rows, hidden %d, vocabulary %d, fp16; %s; medians of %d rounds x %d launches, arms alternated"
             % (T, M, H, V, torch.cuda.get_device_name(0), a.rounds, a.reps),
             "arms agree: largest |hip - stock| / (1 + |stock|) = %.2e" % agree,
             "%-28s %12s %12s %10s" % ("", "hip [us]", "stock [us]", "hip/stock")]
    for w, name in (("chunk", "bmm + NLL (one chunk)"), ("alone", "NLL alone (cold logits)")):
        hip, stock = (med[(w, "hip", 0)] + med[(w, "hip", 1)]) / 2, (med[(w, "stock", 0)] + med[(w, "stock", 1)]) / 2
        lines.append("%-28s %12.1f %12.1f %10.3f" % (name, hip, stock, hip / stock))
        lines.append("%-28s %11.2f%% %11.2f%%" % ("  A/A spread (two series)", 100 * abs(med[(w, "hip", 0)] - med[(w, "hip", 1)]) / hip,
                                                   100 * abs(med[(w, "stock", 0)] - med[(w, "stock", 1)]) / stock))
    hip_alone = (med[("alone", "hip", 0)] + med[("alone", "hip", 1)]) / 2
    lines.append("bmm alone: %.1f us" % bmm_us)
    lines.append("HIP NLL launch: reads %.1f MB, %.2f TB/s = %.0f%% of the %.1f TB/s achievable"
                 % (read / 1e6, read / hip_alone / 1e6, 100 * read / (hip_alone * 1e-6) / HBM_ACHIEVABLE, HBM_ACHIEVABLE / 1e12))
    lines.append("peak allocated over one chunk (logits included): hip %.1f MB, stock %.1f MB" % (peaks["hip"] / 1e6, peaks["stock"] / 1e6))
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(text)


if __name__ == "__main__":
    main()
