#!/usr/bin/env python3
"""What per-request sampling costs a decode step: same-process A/B of the greedy session's step (step_end_ragged) against a sampling session's
(step_end_sample), hipGraph replay, tools/ab_ragged_step.py's protocol: every arm captured once, the arms timed alternately, `--rounds` rounds of
`--steps` replays each.

    python tools/bench_sampling_step.py --tenants 6 --kv-len 512 > profiles/sampling_step.txt

Arms: greedy / greedy_b (the plain session's graph twice: the run's own A/A spread), sample_k50_p90 (every tenant at tau = 1, top_k = 50,
top_p = 0.9), sample_tau1 (tau = 1, no filter), sample_greedy (the sampling session with every tenant at tau = 0).  Then the device time of the two
step-end launches alone, on the step's own logits shape [tenants, vocab] with N(0, 3^2) values: step_end_ragged, and step_end_sample per
parameter set."""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import step_ab  # noqa: E402

SETS = {"sample_k50_p90": dict(temperature=1.0, top_k=50, top_p=0.9), "sample_tau1": dict(temperature=1.0), "sample_greedy": {},
        "sample_k50": dict(temperature=1.0, top_k=50), "sample_p90": dict(temperature=1.0, top_p=0.9)}


def main():
    args = step_ab.parse_args()
    from bitdelta_amd import serving_ops as ops
    from bitdelta_amd.serving_loop import TenantDecoder
    dev = torch.device("cuda", 0)
    T = args.tenants
    dec = TenantDecoder.synthetic(args.model, T, dev, dtype=torch.float16, seed=4321, layers=args.layers, max_len=args.kv_len + 256)
    vocab = dec.cfg[5]
    g = torch.Generator().manual_seed(4321)
    prompts = [torch.randint(1, vocab, (args.kv_len,), generator=g).tolist() for _ in range(T)]

    arms = {}

    def arm(name, sampling, params):
        sess = dec.session(sampling=sampling)
        sess.submit_all(prompts, max_new_tokens=1 << 30, seed=list(range(1, T + 1)) if sampling else 0, **params)
        arms[name] = step_ab.capture(sess)
        return sess
    arm("greedy", False, {})
    arms["greedy_b"] = arms["greedy"]
    for name in ("sample_k50_p90", "sample_tau1", "sample_greedy"):
        arm(name, True, SETS[name])
    arms = {n: arms[n] for n in ("greedy", "sample_k50_p90", "sample_tau1", "greedy_b", "sample_greedy")}
    ms, med = step_ab.time_arms(arms, args)
    base = (med["greedy"] + med["greedy_b"]) / 2

    # the two step-end launches alone: device time per launch
    logits = (torch.randn(T, vocab, generator=g) * 3).half().to(dev)
    big = lambda: torch.full((T,), 1 << 40, dtype=torch.long, device=dev)
    st = dict(tok=torch.zeros(T, 1, dtype=torch.long, device=dev), out=torch.zeros(T, 8, dtype=torch.long, device=dev),
              n=torch.zeros(T, dtype=torch.long, device=dev), pos=torch.zeros(T, dtype=torch.long, device=dev), limit=big(),
              stop=torch.full((T, 8), -1, dtype=torch.long, device=dev), act=torch.ones(T, dtype=torch.bool, device=dev),
              done=torch.zeros(T, dtype=torch.uint8, device=dev))

    kernel_us = step_ab.kernel_timer(dev, args.kernel_iters)
    common = (logits, st["tok"], st["out"], st["n"], st["pos"], st["limit"], st["stop"], st["act"], st["done"], 1 << 30)
    kern = {"step_end_ragged": kernel_us(lambda: ops.step_end_ragged(*common))}
    for name, p in SETS.items():
        tau = torch.full((T,), p.get("temperature", 0.0), dtype=torch.float32, device=dev)
        k = torch.full((T,), p.get("top_k", 0), dtype=torch.int32, device=dev)
        pp = torch.full((T,), p.get("top_p", 1.0), dtype=torch.float32, device=dev)
        seed = torch.arange(1, T + 1, dtype=torch.long, device=dev)
        kern["step_end_sample/" + name] = kernel_us(lambda: ops.step_end_sample(*common, tau, k, pp, seed))
    out = {"model": args.model, "tenants": T, "kv_len": args.kv_len, "layers": len(dec.layers), "vocab": vocab, "steps": args.steps,
           "rounds": args.rounds, "arms": step_ab.arms_json(ms, med),
           "aa_spread_greedy_pct": abs(med["greedy_b"] / med["greedy"] - 1) * 100,
           "over_greedy_pct": {n: (med[n] / base - 1) * 100 for n in arms if n.startswith("sample")},
           "over_greedy_us": {n: (med[n] - base) * 1e3 for n in arms if n.startswith("sample")},
           "launch_us_in_graph": {n: round(v, 3) for n, v in kern.items()}}
    print(json.dumps(out))
    step_ab.print_arms(out["arms"], 16)
    print(f"# A/A spread (greedy): {out['aa_spread_greedy_pct']:.2f} %;  over greedy: " +
          ", ".join(f"{n} {v:+.2f} % ({out['over_greedy_us'][n]:+.1f} us)" for n, v in out["over_greedy_pct"].items()), file=sys.stderr)
    for n, v in out["launch_us_in_graph"].items():
        print(f"# {n:32s} {v:8.3f} us per launch (a chain of launches in one graph)", file=sys.stderr)


if __name__ == "__main__":
    main()
