#!/usr/bin/env python3
"""What per-tenant rotary tables cost a decode step: same-process A/B of a greedy session's step on a decoder with ONE shared [Lmax, 128] table
pair against the same weights on a decoder with a pair PER TENANT, [T, Lmax, 128], whose specs are all neutral -- the tokens are then the same,
and only the table addressing (bd_srv_decode_attention_ragged_tab: + t * s_tab) and the resident footprint differ.  hipGraph replay,
tools/bench_penalty_step.py's protocol: every arm captured once, the arms timed alternately, `--rounds` rounds of `--steps` replays each.

    python tools/bench_tenant_rope_step.py --tenants 6 --kv-len 512 > profiles/tenant_rope_step.txt

Arms: shared / shared_b (the shared-table session's graph twice: the run's own A/A spread), per_tenant.  The two decoders share every weight
tensor (the second is a shell over the first one's layers); each has its own KV cache and its own tables.  Then the device time of the decode
attention launch alone on the step's shape, ragged form, with the 2-D and with the 3-D tables."""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import step_ab  # noqa: E402


def main():
    args = step_ab.parse_args()
    from bitdelta_amd import serving_ops as ops
    from bitdelta_amd.serving_loop import ROPE_DEFAULT, TenantDecoder
    dev = torch.device("cuda", 0)
    T = args.tenants
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
        run, restore = step_ab.capture(sess)
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
    ms, med = step_ab.time_arms(arms, args)
    base = (med["shared"] + med["shared_b"]) / 2

    # the launch alone: device time per decode attention launch on the step's shape (ragged form, every tenant at its own position near kv-len)
    Lc = max_len
    qkv = torch.randn(T, 1, (heads + 2 * kvh) * 128, generator=g).half().to(dev)
    kc = torch.randn(T, kvh, Lc, 128, generator=g).half().to(dev)
    vc = torch.randn(T, kvh, Lc, 128, generator=g).half().to(dev)
    pos = torch.tensor([args.kv_len + 3 * t for t in range(T)], dtype=torch.long, device=dev)
    valid = (torch.arange(Lc, device=dev)[None, :] < pos[:, None]).contiguous()
    act = torch.ones(T, dtype=torch.bool, device=dev)
    kernel_us = step_ab.kernel_timer(dev, args.kernel_iters)
    kern = {}
    for rep in ("", "_b"):                                  # each twice, alternated: the pair's own spread
        kern["decode_attention_ragged/shared" + rep] = kernel_us(lambda: ops.decode_attention_ragged(qkv, dec.cos, dec.sin, kc, vc, valid, pos, act, heads, kvh))
        kern["decode_attention_ragged/per_tenant" + rep] = kernel_us(lambda: ops.decode_attention_ragged(qkv, twin.cos, twin.sin, kc, vc, valid, pos, act, heads, kvh))
    table_bytes = {"shared": 2 * dec.cos.numel() * 2, "per_tenant": 2 * twin.cos.numel() * 2}
    out = {"model": args.model, "tenants": T, "kv_len": args.kv_len, "layers": len(dec.layers), "max_len": max_len, "steps": args.steps,
           "rounds": args.rounds, "arms": step_ab.arms_json(ms, med),
           "aa_spread_shared_pct": abs(med["shared_b"] / med["shared"] - 1) * 100,
           "per_tenant_over_shared_pct": (med["per_tenant"] / base - 1) * 100,
           "per_tenant_over_shared_us": (med["per_tenant"] - base) * 1e3,
           "launch_us_in_graph": {n: round(v, 3) for n, v in kern.items()}, "table_bytes": table_bytes, "tokens_equal": True}
    print(json.dumps(out))
    step_ab.print_arms(out["arms"], 12)
    print(f"# A/A spread (shared): {out['aa_spread_shared_pct']:.2f} %;  per-tenant tables over the shared table's step: "
          f"{out['per_tenant_over_shared_pct']:+.2f} % ({out['per_tenant_over_shared_us']:+.1f} us)", file=sys.stderr)
    for n, v in out["launch_us_in_graph"].items():
        print(f"# {n:40s} {v:8.3f} us per launch (a chain of launches in one graph)", file=sys.stderr)
    print(f"# resident tables: shared {table_bytes['shared'] / 1e6:.2f} MB, per tenant {table_bytes['per_tenant'] / 1e6:.2f} MB", file=sys.stderr)


if __name__ == "__main__":
    main()
