#!/usr/bin/env python3
"""What an e4m3 KV cache does to a decode step: same-process A/B of a greedy session's step on a decoder with a 16-bit cache against the same
weights on a decoder with kv_cache="fp8".  hipGraph replay, tools/bench_tenant_rope_step.py's protocol: every arm captured once, the arms timed
alternately, `--rounds` rounds of `--steps` replays each.

    python tools/bench_kv8_step.py --model mistral-7b --tenants 6 --kv-len 512 >> profiles/kv8_decode_step.txt

Arms: fp16 / fp16_b (the 16-bit session's graph twice: the run's own A/A spread), fp8.  The two decoders share every weight tensor; each has its
own KV cache.  A prompt of 64 tokens is submitted, then every tenant's position is moved to --kv-len over cache rows filled with random finite
values (prompts stop at 1024 tokens; the step's time depends on the rows it reads, not on what they hold), so the arms' tokens are not compared
here -- tests/test_gpu_kv8_*.py hold the arithmetic.  Then the device time of the attention launch alone on the step's shape, both forms, with
the K / V bytes it has to read per launch and the resulting bytes/s, and the resident cache bytes of both decoders."""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import step_ab  # noqa: E402


def main():
    args = step_ab.parse_args(warm_steps=100, kernel_iters=100)
    from bitdelta_amd import serving_ops as ops
    from bitdelta_amd.serving_loop import TenantDecoder
    dev = torch.device("cuda", 0)
    T = args.tenants
    max_len = args.kv_len + 256
    dec = TenantDecoder.synthetic(args.model, T, dev, dtype=torch.float16, seed=4321, layers=args.layers, max_len=max_len)
    twin = TenantDecoder(dec.cfg, T, dev, torch.float16, max_len=max_len, kv_cache="fp8")
    twin.layers, twin.embed, twin.final_norm, twin.lm_head = dec.layers, dec.embed, dec.final_norm, dec.lm_head
    vocab, heads, kvh = dec.cfg[5], dec.cfg[3], dec.cfg[4]
    g = torch.Generator().manual_seed(4321)
    prompts = [torch.randint(1, vocab, (64,), generator=g).tolist() for _ in range(T)]
    arms, resident = {}, {}

    def arm(name, d):
        sess = d.session()
        sess.submit_all(prompts, max_new_tokens=1 << 30)
        for c in sess.cache["k"] + sess.cache["v"]:         # finite values in every row the step will read
            if c.dtype == torch.float8_e4m3fn:
                c.view(torch.uint8).copy_(torch.randint(0, 0x70, c.shape, device=dev, dtype=torch.uint8))
            else:
                c.normal_()
        sess.cache["valid"][:, :args.kv_len] = True
        sess.pos.fill_(args.kv_len)
        resident[name] = sum(c.numel() * c.element_size() for c in sess.cache["k"] + sess.cache["v"])
        arms[name] = step_ab.capture(sess)
    arm("fp16", dec)
    arms["fp16_b"] = arms["fp16"]
    arm("fp8", twin)
    arms = {n: arms[n] for n in ("fp16", "fp8", "fp16_b")}
    ms, med = step_ab.time_arms(arms, args)
    base = (med["fp16"] + med["fp16_b"]) / 2

    # the launch alone: device time per decode attention launch on the step's shape (ragged form, every tenant near kv-len)
    Lc = max_len
    qkv = torch.randn(T, 1, (heads + 2 * kvh) * 128, generator=g).half().to(dev)
    kc, vc = (torch.randn(T, kvh, Lc, 128, device=dev).half() for _ in range(2))
    k8, v8 = (torch.randint(0, 0x70, (T, kvh, Lc, 128), device=dev, dtype=torch.uint8).view(torch.float8_e4m3fn) for _ in range(2))
    sc, inv = ops.kv8_scale_pair(torch.ones(T, kvh), dev)
    pos = torch.tensor([args.kv_len + 3 * t for t in range(T)], dtype=torch.long, device=dev)
    valid = (torch.arange(Lc, device=dev)[None, :] < pos[:, None]).contiguous()
    act = torch.ones(T, dtype=torch.bool, device=dev)
    kernel_us = step_ab.kernel_timer(dev, args.kernel_iters)
    kern = {}
    for rep in ("", "_b"):                                  # each twice, alternated: the pair's own spread
        kern["fp16" + rep] = kernel_us(lambda: ops.decode_attention_ragged(qkv, dec.cos, dec.sin, kc, vc, valid, pos, act, heads, kvh))
        kern["fp8" + rep] = kernel_us(lambda: ops.decode_attention_kv8(qkv, dec.cos, dec.sin, k8, v8, sc, sc, inv, inv, valid, pos, heads, kvh, active=act))
    rows = int(pos.sum()) * kvh * 128 * 2                   # K and V elements a launch has to read
    launch = {n: {"us": round(v, 3), "kv_bytes": rows * (1 if n.startswith("fp8") else 2),
                  "GBps": round(rows * (1 if n.startswith("fp8") else 2) / v / 1e3, 1)} for n, v in kern.items()}
    out = {"model": args.model, "tenants": T, "kv_len": args.kv_len, "layers": len(dec.layers), "max_len": max_len, "steps": args.steps,
           "rounds": args.rounds, "arms": step_ab.arms_json(ms, med),
           "aa_spread_fp16_pct": abs(med["fp16_b"] / med["fp16"] - 1) * 100, "fp8_over_fp16_pct": (med["fp8"] / base - 1) * 100,
           "fp8_over_fp16_us": (med["fp8"] - base) * 1e3, "launch_in_graph": launch, "resident_cache_bytes": resident}
    print(json.dumps(out))
    step_ab.print_arms(out["arms"], 8)
    print(f"# A/A spread (fp16): {out['aa_spread_fp16_pct']:.2f} %;  fp8 cache over the 16-bit cache's step: {out['fp8_over_fp16_pct']:+.2f} % "
          f"({out['fp8_over_fp16_us']:+.1f} us)", file=sys.stderr)
    for n, v in launch.items():
        print(f"# attention launch {n:8s} {v['us']:9.3f} us, {v['kv_bytes'] / 1e6:8.2f} MB of K / V: {v['GBps']:8.1f} GB/s", file=sys.stderr)
    print(f"# resident cache: 16-bit {resident['fp16'] / 1e6:.1f} MB, fp8 {resident['fp8'] / 1e6:.1f} MB", file=sys.stderr)


if __name__ == "__main__":
    main()
