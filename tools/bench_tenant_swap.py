#!/usr/bin/env python3
"""Loading ONE fine-tune into one tenant slot of a live layer: FusedDeltaLinear.load_tenant (the sign-load kernel: one tenant's words read once,
written into `mask` and into slot t of `mask_packed`) against the only route there was before it -- pack_decode_masks over the whole re-stacked
tenant set plus copy_ into the existing buffers.  One full-width Mistral-7B layer (mistral-1layer shapes), fp16, once per t_pad in {1, 6, 16}
(T = t_pad tenants).

Per Linear and per layer: microseconds, algorithmic bytes (signs read once, written twice) and TB/s.  The COMPARISON is like with like, both
arms eager on an idle stream with device events around one call, median of --reps, which is how a caller runs either (a decoder-level load
refuses to run under capture):
  call     load_tenant (its alpha updates and host enqueue included);
  rebuild  the old route, and its peak extra device memory.
The two run twice each, alternating (A B A' B'): the A/A spread is printed next to both.  One more column is NOT comparable with them and
is there for the bytes per second only:
  kernel   the sign-load launches alone, 20 loads replayed from a captured graph (8 rotating source sets, rotating slots): device time
           with no host enqueue in it."""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from bitdelta_amd.binary_gemm_kernel import load_decode_masks, pack_decode_masks
from bitdelta_amd.serving_loop import MODEL_CONFIGS, FusedDeltaLinear, fused_columns, fused_perm

DEV = "cuda:0"


def median(v):
    return sorted(v)[len(v) // 2]


def event_times(fn, reps, warm=3):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1) * 1e3)
    return median(ts)


def graph_times(fn, reps, per_graph=20):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):
            for _ in range(per_graph):
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
            ts.append(e0.elapsed_time(e1) / per_graph * 1e3)
    return median(ts)


def words(gen, *shape):
    return torch.randint(-2 ** 31, 2 ** 31 - 1, shape, generator=gen, dtype=torch.int32, device=DEV)


def bench_linear(name, shapes, T, inter8, reps, gen):
    K = shapes[0][1]
    widths = [n for n, _ in shapes]
    ws = [(torch.randn(n, K, device=DEV, generator=gen) * 0.02).half() for n in widths]
    mod = FusedDeltaLinear(ws, [words(gen, T, K // 32, n) for n in widths], [torch.rand(T, device=DEV, generator=gen) * 1e-3 for _ in widths],
                           interleave8=inter8)
    del ws
    assert mod.mask_packed is not None and mod.mask_packed.shape[-1] == T
    sets = [[words(gen, K // 32, n) for n in widths] for _ in range(8)]
    coeffs = [torch.rand((), device=DEV, generator=gen) * 1e-3 for _ in widths]
    maps = fused_columns(widths, inter8)[1]
    perm = fused_perm(widths, inter8, DEV)
    i = [0]

    def kernel():
        i[0] += 1
        t = i[0] % T
        for m, (off, blk, stride) in zip(sets[i[0] % 8], maps):
            load_decode_masks(m, mask=mod.mask[t], packed=mod.mask_packed, slot=t, col_off=off, col_blk=blk, col_stride=stride)

    def call():
        i[0] += 1
        mod.load_tenant(i[0] % T, sets[i[0] % 8], coeffs)

    def rebuild():
        i[0] += 1
        t = i[0] % T
        new = torch.cat(sets[i[0] % 8], 1)
        mod.mask[t].copy_(new if perm is None else new[:, perm])
        mod.mask_packed.copy_(pack_decode_masks(mod.mask))

    c1 = event_times(call, reps)
    r1 = event_times(rebuild, reps)
    c2 = event_times(call, reps)
    r2 = event_times(rebuild, reps)
    k = graph_times(kernel, reps)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    rebuild()
    torch.cuda.synchronize()
    extra = torch.cuda.max_memory_allocated() - before
    # the result of the last kernel-route load is what the rebuild route makes of the same set
    call()
    assert torch.equal(mod.mask_packed, pack_decode_masks(mod.mask))
    nbytes = 3 * mod.mask[0].numel() * 4
    return dict(name=name, bytes=nbytes, kernel=k, call=(c1, c2), rebuild=(r1, r2), extra=extra)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=21)
    ap.add_argument("--t-pads", type=int, nargs="*", default=[1, 6, 16])
    ap.add_argument("--out", default=None, help="also write the table to this file")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "a measurement needs the device"
    hid, inter, _, heads, kvh, _ = MODEL_CONFIGS["mistral-1layer"]
    hd = hid // heads
    layer = [("qkv", [(heads * hd, hid), (kvh * hd, hid), (kvh * hd, hid)], False), ("o", [(hid, heads * hd)], False),
             ("gate_up", [(inter, hid), (inter, hid)], True), ("down", [(hid, inter)], False)]
    lines = ["load one fine-tune into one slot of a Mistral-7B layer (fp16, T = t_pad tenants); bytes = one tenant's signs read once + written twice",
             "call / rebuild: eager, device events around one call, median of %d; (A/A) = the same arm measured again, arms alternating" % a.reps,
             "kernel: sign-load launches alone replayed from a graph -- device time, not comparable with the two eager columns",
             "%-6s %-8s %8s | %21s | %23s %9s | %-14s | %9s %6s" % ("t_pad", "linear", "MB", "call us (A/A)", "rebuild us (A/A)", "extra MB",
                                                                "rebuild / call", "kernel us", "TB/s")]
    fmt = "%-6d %-8s %8.2f | %9.1f (%9.1f) | %10.1f (%10.1f) %9.1f | %-14s | %9.1f %6.2f"
    gen = torch.Generator(device=DEV).manual_seed(0)
    for T in a.t_pads:
        tot = dict(bytes=0, k=0.0, c=[0.0, 0.0], r=[0.0, 0.0], extra=0)
        for name, shapes, inter8 in layer:
            r = bench_linear(name, shapes, T, inter8, a.reps, gen)
            c, rb = min(r["call"]), min(r["rebuild"])
            lines.append(fmt % (T, name, r["bytes"] / 1e6, r["call"][0], r["call"][1], r["rebuild"][0], r["rebuild"][1], r["extra"] / 1e6,
                                "%.2fx%s" % (rb / c, " (LOSES)" if rb < c else ""), r["kernel"], r["bytes"] / r["kernel"] / 1e6))
            tot["bytes"] += r["bytes"]
            tot["k"] += r["kernel"]
            tot["extra"] = max(tot["extra"], r["extra"])
            for j in range(2):
                tot["c"][j] += r["call"][j]
                tot["r"][j] += r["rebuild"][j]
            torch.cuda.empty_cache()
        c, rb = min(tot["c"]), min(tot["r"])
        lines.append(fmt % (T, "LAYER", tot["bytes"] / 1e6, tot["c"][0], tot["c"][1], tot["r"][0], tot["r"][1], tot["extra"] / 1e6,
                            "%.2fx%s" % (rb / c, " (LOSES)" if rb < c else ""), tot["k"], tot["bytes"] / tot["k"] / 1e6) +
                     "   32 x layer: call %.2f ms, rebuild %.2f ms, kernel %.2f ms" % (32 * c / 1e3, 32 * rb / 1e3, 32 * tot["k"] / 1e3))
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
