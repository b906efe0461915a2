#!/usr/bin/env python3
"""Same-process A/B of the lockstep decode step (TenantDecoder.generate's captured graph) against the session's ragged step (TenantSession), hipGraph
replay, tools/ab_decode_step.py's protocol: every arm captured once, the arms timed alternately, `--rounds` rounds of `--steps` replays each.

    python tools/ab_ragged_step.py --tenants 6 --kv-len 512 > profiles/ragged_decode_step.txt

Arms: lockstep / lockstep_b (the same graph twice: the run's own A/A spread), ragged / ragged_b (the session's graph with every tenant at the
lockstep position; A/A likewise), ragged_mixed (the same graph with the tenants' positions spread over 64 .. kv-len: no bar applies to it).  The
tokens of the ragged arm over 8 steps must equal the lockstep arm's."""
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
    ap.add_argument("--replay-only", default=None, help="replay this one arm for --steps steps and exit (a kernel-trace run under a profiler)")
    args = ap.parse_args()
    from bitdelta_amd import dist as bdd
    from bitdelta_amd.serving_loop import TenantDecoder
    dev = torch.device("cuda", 0)
    T = args.tenants
    assert max(args.warm_steps, args.steps + 1, 9) < 256, "the arms must not run into the end of the cache (kv-len + 256 rows)"
    dec = TenantDecoder.synthetic(args.model, T, dev, dtype=torch.float16, seed=4321, layers=args.layers, max_len=args.kv_len + 256)
    vocab = dec.cfg[5]
    g = torch.Generator().manual_seed(4321)
    prompts = [torch.randint(1, vocab, (args.kv_len,), generator=g).tolist() for _ in range(T)]

    # lockstep arm: the state generate() keeps, on a cache of its own
    ids, am = dec.prepare(prompts)
    cache = dec.new_cache()
    first = torch.argmax(dec.prefill(ids, am, cache), dim=-1)
    st = {"cache": cache, "tok": first[:, None].clone(), "pos": torch.tensor([ids.shape[1]], device=dev),
          "step": torch.tensor([1], device=dev), "stop_ids": torch.full((T, 1), -1, dtype=torch.long, device=dev),
          "out": torch.zeros(T, 4096, dtype=torch.long, device=dev), "stopped": torch.zeros(T, dtype=torch.bool, device=dev)}
    snap = {k: v.clone() for k, v in st.items() if torch.is_tensor(v)}
    valid0 = cache["valid"].clone()

    def restore_lock():
        for k, v in snap.items():
            st[k].copy_(v)
        cache["valid"].copy_(valid0)
    lock = dec._graph_runner(st)

    # ragged arms: a session on the decoder's cache, every tenant admitted at once
    sess = dec.session()
    sess.submit_all(prompts, max_new_tokens=1 << 30)
    rsnap = [v.clone() for v in sess._state()]
    L = ids.shape[1]
    lo = min(64, L)
    spread = torch.tensor([lo + (L - lo) * t // max(T - 1, 1) for t in range(T)], device=dev)

    def restore_ragged(mixed=False):
        for v, s_ in zip(sess._state(), rsnap):
            v.copy_(s_)
        if mixed:                       # (timing only: each tenant keeps a prefix of its prefilled rows)
            sess.pos.copy_(spread)
            sess.cache["valid"] &= torch.arange(sess.Lc, device=dev)[None, :] < spread[:, None]
    ragged = sess._runner()
    restore_ragged()

    arms = {"lockstep": (lock, restore_lock), "ragged": (ragged, restore_ragged), "lockstep_b": (lock, restore_lock),
            "ragged_b": (ragged, restore_ragged), "ragged_mixed": (ragged, lambda: restore_ragged(True))}
    if args.replay_only:
        run, restore = arms[args.replay_only]
        restore()
        for _ in range(args.steps):
            run()
        torch.cuda.synchronize()
        return
    toks = {}
    for n in ("lockstep", "ragged"):
        run, restore = arms[n]
        restore()
        for _ in range(8):
            run()
        torch.cuda.synchronize()
        toks[n] = (st["out"] if n == "lockstep" else sess.out)[:, 1:9].cpu().clone()
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
    out = {"model": args.model, "tenants": T, "kv_len": args.kv_len, "layers": len(dec.layers), "steps": args.steps, "rounds": args.rounds,
           "mixed_positions": spread.tolist(), "tokens_equal": bool(torch.equal(toks["lockstep"], toks["ragged"])),
           "arms": {n: {"min_ms": min(v), "median_ms": med[n], "all_ms": [round(x, 4) for x in v]} for n, v in ms.items()},
           "aa_spread_lockstep_pct": abs(med["lockstep_b"] / med["lockstep"] - 1) * 100, "aa_spread_ragged_pct": abs(med["ragged_b"] / med["ragged"] - 1) * 100,
           "ragged_over_lockstep_pct": ((med["ragged"] + med["ragged_b"]) / (med["lockstep"] + med["lockstep_b"]) - 1) * 100,
           "mixed_over_lockstep_pct": (2 * med["ragged_mixed"] / (med["lockstep"] + med["lockstep_b"]) - 1) * 100}
    print(json.dumps(out))
    for n, a in out["arms"].items():
        print(f"# {n:14s} min {a['min_ms']:.4f}  median {a['median_ms']:.4f} ms/step", file=sys.stderr)
    print(f"# A/A spread: lockstep {out['aa_spread_lockstep_pct']:.2f} %, ragged {out['aa_spread_ragged_pct']:.2f} %;  ragged over lockstep "
          f"{out['ragged_over_lockstep_pct']:+.2f} %, mixed {out['mixed_over_lockstep_pct']:+.2f} %;  tokens equal: {out['tokens_equal']}", file=sys.stderr)


if __name__ == "__main__":
    main()
