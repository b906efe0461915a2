#!/usr/bin/env python3
"""What the request penalties cost a decode step: same-process A/B of a sampling session's step against the same session made with
penalties=True, hipGraph replay, tools/bench_sampling_step.py's protocol: every arm captured once, the arms timed alternately, `--rounds` rounds
of `--steps` replays each.

    python tools/bench_penalty_step.py --tenants 6 --kv-len 512 > profiles/penalty_step.txt

Arms: sample / sample_b (the sampling session's graph twice, every tenant at tau = 1, top_k = 50, top_p = 0.9: the run's own A/A spread),
pen_neutral (the same with penalties=True and neutral parameters: one more launch, step_penalize, in front of step_end_sample), pen_active (every
tenant at repetition_penalty = 1.1, presence_penalty = frequency_penalty = 0.5 and 8 logit_bias entries).  Then the device time of the launch
alone on the step's own shape [tenants, vocab] with N(0, 3^2) logits and a history with 512 context tokens and 64 counted ones per tenant:
step_penalize with neutral and with the active parameters, penalize_rows, and step_end_sample re-measured next to them."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

SAMPLE = dict(temperature=1.0, top_k=50, top_p=0.9)


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
    from bitdelta_amd.serving_loop import TenantDecoder, penalty_row
    dev = torch.device("cuda", 0)
    T = args.tenants
    assert max(args.warm_steps, args.steps + 1) < 256, "the arms must not run into the end of the cache (kv-len + 256 rows)"
    dec = TenantDecoder.synthetic(args.model, T, dev, dtype=torch.float16, seed=4321, layers=args.layers, max_len=args.kv_len + 256)
    vocab = dec.cfg[5]
    g = torch.Generator().manual_seed(4321)
    prompts = [torch.randint(1, vocab, (args.kv_len,), generator=g).tolist() for _ in range(T)]
    active = dict(repetition_penalty=1.1, presence_penalty=0.5, frequency_penalty=0.5,
                  logit_bias={int(i): 1.5 for i in torch.randperm(vocab, generator=g)[:8]})

    arms = {}

    def arm(name, penalties, params):
        sess = dec.session(sampling=True, penalties=penalties)
        sess.submit_all(prompts, max_new_tokens=1 << 30, seed=list(range(1, T + 1)), **SAMPLE, **params)
        snap = [v.clone() for v in sess._state()]

        def restore():
            for v, s_ in zip(sess._state(), snap):
                v.copy_(s_)
        run = sess._runner()
        restore()
        arms[name] = (run, restore)
    arm("sample", False, {})
    arms["sample_b"] = arms["sample"]
    arm("pen_neutral", True, {})
    arm("pen_active", True, active)
    arms = {n: arms[n] for n in ("sample", "pen_neutral", "pen_active", "sample_b")}
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
    base = (med["sample"] + med["sample_b"]) / 2

    # the launch alone: device time per launch on the step's shape
    logits = (torch.randn(T, vocab, generator=g) * 3).half().to(dev)
    plogits = torch.zeros_like(logits)
    hist = torch.zeros(T, vocab, dtype=torch.int16)
    for t in range(T):
        hist[t, torch.randperm(vocab, generator=g)[:512]] = -32768
        hist[t, torch.randperm(vocab, generator=g)[:64]] += 3
    hist = hist.to(dev)
    tok = torch.randint(0, vocab, (T, 1), generator=g).to(dev)
    act = torch.ones(T, dtype=torch.bool, device=dev)
    pen_n = torch.tensor([penalty_row((1.0, 0.0, 0.0, ()))] * T, dtype=torch.float32).to(dev)
    pen_a = torch.tensor([penalty_row((1.1, 0.5, 0.5, ()))] * T, dtype=torch.float32).to(dev)
    bias_id = torch.full((T, 16), -1, dtype=torch.int32)
    bias_id[:, :8] = torch.tensor(sorted(active["logit_bias"]), dtype=torch.int32)
    bias_val = torch.zeros(T, 16)
    bias_val[:, :8] = 1.5
    bias_id, bias_val = bias_id.to(dev), bias_val.to(dev)
    empty_id, empty_val = torch.full_like(bias_id, -1), torch.zeros_like(bias_val)
    big = lambda: torch.full((T,), 1 << 40, dtype=torch.long, device=dev)
    st = dict(tok=torch.zeros(T, 1, dtype=torch.long, device=dev), out=torch.zeros(T, 8, dtype=torch.long, device=dev),
              n=torch.zeros(T, dtype=torch.long, device=dev), pos=torch.zeros(T, dtype=torch.long, device=dev), limit=big(),
              stop=torch.full((T, 8), -1, dtype=torch.long, device=dev), act=torch.ones(T, dtype=torch.bool, device=dev),
              done=torch.zeros(T, dtype=torch.uint8, device=dev))
    tau = torch.full((T,), 1.0, dtype=torch.float32, device=dev)
    k = torch.full((T,), 50, dtype=torch.int32, device=dev)
    pp = torch.full((T,), 0.9, dtype=torch.float32, device=dev)
    seed = torch.arange(1, T + 1, dtype=torch.long, device=dev)

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
    kern = {
        "step_penalize/neutral": kernel_us(lambda: ops.step_penalize(logits, plogits, hist, tok, act, pen_n, empty_id, empty_val)),
        "step_penalize/active_8_bias": kernel_us(lambda: ops.step_penalize(logits, plogits, hist, tok, act, pen_a, bias_id, bias_val)),
        "penalize_rows/active_8_bias": kernel_us(lambda: ops.penalize_rows(logits, hist, pen_a, bias_id, bias_val, out=plogits)),
        "step_end_sample/k50_p90": kernel_us(lambda: ops.step_end_sample(logits, st["tok"], st["out"], st["n"], st["pos"], st["limit"], st["stop"],
                                                                         st["act"], st["done"], 1 << 30, tau, k, pp, seed)),
    }
    moved = T * vocab * 6
    out = {"model": args.model, "tenants": T, "kv_len": args.kv_len, "layers": len(dec.layers), "vocab": vocab, "steps": args.steps,
           "rounds": args.rounds, "arms": {n: {"min_ms": min(v), "median_ms": med[n], "all_ms": [round(x, 4) for x in v]} for n, v in ms.items()},
           "aa_spread_sample_pct": abs(med["sample_b"] / med["sample"] - 1) * 100,
           "over_sample_pct": {n: (med[n] / base - 1) * 100 for n in arms if n.startswith("pen")},
           "over_sample_us": {n: (med[n] - base) * 1e3 for n in arms if n.startswith("pen")},
           "launch_us_in_graph": {n: round(v, 3) for n, v in kern.items()}, "launch_bytes": moved}
    print(json.dumps(out))
    for n, a in out["arms"].items():
        print(f"# {n:16s} min {a['min_ms']:.4f}  median {a['median_ms']:.4f} ms/step", file=sys.stderr)
    print(f"# A/A spread (sample): {out['aa_spread_sample_pct']:.2f} %;  over the sampling session's step: " +
          ", ".join(f"{n} {v:+.2f} % ({out['over_sample_us'][n]:+.1f} us)" for n, v in out["over_sample_pct"].items()), file=sys.stderr)
    for n, v in out["launch_us_in_graph"].items():
        print(f"# {n:32s} {v:8.3f} us per launch (a chain of launches in one graph; {moved} bytes of logits, history and output)", file=sys.stderr)


if __name__ == "__main__":
    main()
