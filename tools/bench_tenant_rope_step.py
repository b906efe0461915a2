#!/usr/bin/env python3
"""What per-tenant rotary tables cost a decode step: same-process A/B of a greedy session's step on a decoder with ONE shared [Lmax, 128] table
pair against the same weights on a decoder with a pair PER TENANT, [T, Lmax, 128], whose specs are all neutral -- the tokens are then the same,
and only the table addressing (bd_srv_decode_attention_ragged_tab: + t * s_tab) and the resident footprint differ.  hipGraph replay,
tools/bench_penalty_step.py's protocol: every arm captured once, the arms timed alternately, `--rounds` rounds of `--steps` replays each.

    python tools/bench_tenant_rope_step.py --tenants 6 --kv-len 512 > profiles/tenant_rope_step.txt

Arms: shared / shared_b (the shared-table session's graph twice: the run's own A/A spread), per_tenant.  The two decoders share every weight
tensor (the second is a shell over the first one's layers); each has its own KV cache and its own tables.  Then the device time of the decode
attention launch alone on the step's shape, ragged form, with the 2-D and with the 3-D tables."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="mistral-7b")
    ap.add_argument("--tenants", type=int, default=6)
    ap.add_argument("--kv-len", type=int, default=512)
    ap.add_argument("--layers", type=int, default=None)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--warm-steps", type=int, default=200, help="replays of every arm before the first timed round (clocks)")
    ap.add_argument("--kernel-iters", type=int, default=200)
    args = ap.parse_args()
    from bitdelta_amd import dist as bdd
    from bitdelta_amd import serving_ops as ops
    from bitdelta_amd.serving_loop import ROPE_DEFAULT, TenantDecoder
    dev = torch.device("cuda", 0)
    T = args.tenants
    assert max(args.warm_steps, args.steps + 1) < 256, "the arms must not run into the end of the cache (kv-len + 256 rows)"
    max_len = args.kv_len + 256
    dec = TenantDecoder.synthetic(args.model, T, dev, dtype=torch.float16, seed=4321, layers=args.layers, max_len=max_len)
    twin = TenantDecoder(dec.cfg, T, dev, torch.float16, max_len=max_len, rope=[ROPE_DEFAULT] * T)
    twin.layers, twin.embed, twin.final_norm, twin.lm_head = dec.layers, dec.embed, dec.final_norm, dec.lm_head
    assert twin.cos.shape == (T, max_len, 128) and all(torch.equal(twin.cos[t], dec.cos) and torch.equal(twin.sin[t], dec.sin) for t in range(T))
    vocab, heads, kvh = dec.cfg[5], dec.cfg[3], dec.cfg[4]
    g = torch.Generator().manual_seed(4321)
    prompts = [torch.randint(1, vocab, (args.kv_len,), generator=g).tolist() for _ in range(T)]

    arms, first = {}, {}

    def arm(name, d):
        sess = d.session()
        sess.submit_all(prompts, max_new_tokens=1 << 30)
        snap = [v.clone() for v in sess._state()]

        def restore():
            for v, s_ in zip(sess._state(), snap):
                v.copy_(s_)
        run = sess._runner()
        restore()
        for _ in range(8):                                  # the tokens of the first steps: the arms must agree
            run()
        first[name] = sess.out[:, :9].clone()
        restore()
        arms[name] = (run, restore)
    arm("shared", dec)
    arms["shared_b"] = arms["shared"]
    arm("per_tenant", twin)
    assert torch.equal(first["shared"], first["per_tenant"]), "neutral per-tenant tables must give the shared table's tokens"
    arms = {n: arms[n] for n in ("shared", "per_tenant", "shared_b")}
    for run, restore in arms.values():
        restore()
        for _ in range(args.warm_steps):
            run()
    ms = {n: [] for n in arms}
    for _ in range(args.rounds):
        for n, (run, restore) in arms.items():
            restore()
            run()
            ms[n].append(bdd.timed_region(run, args.steps, device_sync=torch.cuda.synchronize) / args.steps * 1e3)
    med = {n: sorted(v)[len(v) // 2] for n, v in ms.items()}
    base = (med["shared"] + med["shared_b"]) / 2

    # the launch alone: device time per decode attention launch on the step's shape (ragged form, every tenant at its own position near kv-len)
    Lc = max_len
    qkv = torch.randn(T, 1, (heads + 2 * kvh) * 128, generator=g).half().to(dev)
    kc = torch.randn(T, kvh, Lc, 128, generator=g).half().to(dev)
    vc = torch.randn(T, kvh, Lc, 128, generator=g).half().to(dev)
    pos = torch.tensor([args.kv_len + 3 * t for t in range(T)], dtype=torch.long, device=dev)
    valid = (torch.arange(Lc, device=dev)[None, :] < pos[:, None]).contiguous()
    act = torch.ones(T, dtype=torch.bool, device=dev)
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
    kern = {}
    for rep in ("", "_b"):                                  # each twice, alternated: the pair's own spread
        kern["decode_attention_ragged/shared" + rep] = kernel_us(lambda: ops.decode_attention_ragged(qkv, dec.cos, dec.sin, kc, vc, valid, pos, act, heads, kvh))
        kern["decode_attention_ragged/per_tenant" + rep] = kernel_us(lambda: ops.decode_attention_ragged(qkv, twin.cos, twin.sin, kc, vc, valid, pos, act, heads, kvh))
    table_bytes = {"shared": 2 * dec.cos.numel() * 2, "per_tenant": 2 * twin.cos.numel() * 2}
    out = {"model": args.model, "tenants": T, "kv_len": args.kv_len, "layers": len(dec.layers), "max_len": max_len, "steps": args.steps,
           "rounds": args.rounds, "arms": {n: {"min_ms": min(v), "median_ms": med[n], "all_ms": [round(x, 4) for x in v]} for n, v in ms.items()},
           "aa_spread_shared_pct": abs(med["shared_b"] / med["shared"] - 1) * 100,
           "per_tenant_over_shared_pct": (med["per_tenant"] / base - 1) * 100,
           "per_tenant_over_shared_us": (med["per_tenant"] - base) * 1e3,
           "launch_us_in_graph": {n: round(v, 3) for n, v in kern.items()}, "table_bytes": table_bytes, "tokens_equal": True}
    print(json.dumps(out))
    for n, a in out["arms"].items():
        print(f"# {n:12s} min {a['min_ms']:.4f}  median {a['median_ms']:.4f} ms/step", file=sys.stderr)
    print(f"# A/A spread (shared): {out['aa_spread_shared_pct']:.2f} %;  per-tenant tables over the shared table's step: "
          f"{out['per_tenant_over_shared_pct']:+.2f} % ({out['per_tenant_over_shared_us']:+.1f} us)", file=sys.stderr)
    for n, v in out["launch_us_in_graph"].items():
        print(f"# {n:40s} {v:8.3f} us per launch (a chain of launches in one graph)", file=sys.stderr)
    print(f"# resident tables: shared {table_bytes['shared'] / 1e6:.2f} MB, per tenant {table_bytes['per_tenant'] / 1e6:.2f} MB", file=sys.stderr)


if __name__ == "__main__":
    main()
