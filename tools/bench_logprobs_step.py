#!/usr/bin/env python3
"""What per-token log-probabilities cost a decode step: same-process A/B of a session's step without and with logprobs=k (one more launch,
step_logprobs, behind the step-end launch), hipGraph replay, tools/bench_sampling_step.py's protocol: every arm captured once, the arms timed
alternately, `--rounds` rounds of `--steps` replays each.

    python tools/bench_logprobs_step.py --tenants 6 --kv-len 512 > profiles/logprobs_step.txt

Arms: greedy / greedy_b (the plain session's graph twice: the run's own A/A spread), greedy_lp0 / greedy_lp5 / greedy_lp20 (the greedy session with
logprobs=0, 5, 20), sample / sample_lp5 (every tenant at tau = 1, top_k = 50, top_p = 0.9, without and with logprobs=5).  The baseline of every
ratio is the arm without logprobs in this process.  Then the device time of the launches alone, on the step's own logits shape [tenants, vocab]
with N(0, 3^2) values: step_end_ragged, and the log-probability kernel for top_n = 0, 5, 20 -- through token_logprobs, the same kernel without the
step form's counter (a chain of step_logprobs launches would do its work once and then find nothing new)."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

SAMPLE = dict(temperature=1.0, top_k=50, top_p=0.9)
ARMS = {"greedy": (False, None), "greedy_lp0": (False, 0), "greedy_lp5": (False, 5), "greedy_lp20": (False, 20), "sample": (True, None),
        "sample_lp5": (True, 5)}
ORDER = ("greedy", "greedy_lp0", "greedy_lp5", "sample", "greedy_lp20", "greedy_b", "sample_lp5")
BASE = {"greedy_lp0": "greedy", "greedy_lp5": "greedy", "greedy_lp20": "greedy", "sample_lp5": "sample"}


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
    from bitdelta_amd.serving_loop import TenantDecoder
    dev = torch.device("cuda", 0)
    T = args.tenants
    assert max(args.warm_steps, args.steps + 1) < 256, "the arms must not run into the end of the cache (kv-len + 256 rows)"
    dec = TenantDecoder.synthetic(args.model, T, dev, dtype=torch.float16, seed=4321, layers=args.layers, max_len=args.kv_len + 256)
    vocab = dec.cfg[5]
    g = torch.Generator().manual_seed(4321)
    prompts = [torch.randint(1, vocab, (args.kv_len,), generator=g).tolist() for _ in range(T)]

    arms = {}
    for name, (sampling, k) in ARMS.items():
        sess = dec.session(sampling=sampling, logprobs=k)
        sess.submit_all(prompts, max_new_tokens=1 << 30, **(dict(SAMPLE, seed=list(range(1, T + 1))) if sampling else {}))
        snap = [v.clone() for v in sess._state()]

        def restore(sess=sess, snap=snap):
            for v, s_ in zip(sess._state(), snap):
                v.copy_(s_)
        run = sess._runner()
        restore()
        arms[name] = (run, restore)
    arms["greedy_b"] = arms["greedy"]
    arms = {n: arms[n] for n in ORDER}
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
    base = {"greedy": (med["greedy"] + med["greedy_b"]) / 2, "sample": med["sample"]}

    # the launches alone: device time per launch
    logits = (torch.randn(T, vocab, generator=g) * 3).half().to(dev)
    big = torch.full((T,), 1 << 40, dtype=torch.long, device=dev)
    st = dict(tok=torch.zeros(T, 1, dtype=torch.long, device=dev), out=torch.zeros(T, 8, dtype=torch.long, device=dev),
              n=torch.zeros(T, dtype=torch.long, device=dev), pos=torch.zeros(T, dtype=torch.long, device=dev), limit=big,
              stop=torch.full((T, 8), -1, dtype=torch.long, device=dev), act=torch.ones(T, dtype=torch.bool, device=dev),
              done=torch.zeros(T, dtype=torch.uint8, device=dev))
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
    kern = {"step_end_ragged": kernel_us(lambda: ops.step_end_ragged(logits, st["tok"], st["out"], st["n"], st["pos"], st["limit"], st["stop"],
                                                                     st["act"], st["done"], 1 << 30))}
    tok = torch.argmax(logits, dim=-1)
    for k in (0, 5, 20):
        outs = (torch.empty(T, dtype=torch.float32, device=dev), torch.empty(T, k, dtype=torch.int32, device=dev),
                torch.empty(T, k, dtype=torch.float32, device=dev))
        kern["token_logprobs/top_n=%d" % k] = kernel_us(lambda: ops.token_logprobs(logits, tok, k, out=outs))
    out = {"model": args.model, "tenants": T, "kv_len": args.kv_len, "layers": len(dec.layers), "vocab": vocab, "steps": args.steps,
           "rounds": args.rounds, "arms": {n: {"min_ms": min(v), "median_ms": med[n], "all_ms": [round(x, 4) for x in v]} for n, v in ms.items()},
           "aa_spread_greedy_pct": abs(med["greedy_b"] / med["greedy"] - 1) * 100,
           "over_base_pct": {n: (med[n] / base[b] - 1) * 100 for n, b in BASE.items()},
           "over_base_us": {n: (med[n] - base[b]) * 1e3 for n, b in BASE.items()},
           "launch_us_in_graph": {n: round(v, 3) for n, v in kern.items()}}
    print(json.dumps(out))
    for n, a in out["arms"].items():
        print(f"# {n:16s} min {a['min_ms']:.4f}  median {a['median_ms']:.4f} ms/step", file=sys.stderr)
    print(f"# A/A spread (greedy): {out['aa_spread_greedy_pct']:.2f} %;  over the arm without logprobs: " +
          ", ".join(f"{n} {v:+.2f} % ({out['over_base_us'][n]:+.1f} us)" for n, v in out["over_base_pct"].items()), file=sys.stderr)
    for n, v in out["launch_us_in_graph"].items():
        print(f"# {n:32s} {v:8.3f} us per launch (a chain of launches in one graph)", file=sys.stderr)


if __name__ == "__main__":
    main()
