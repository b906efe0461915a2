#!/usr/bin/env python3
"""What stop sequences cost a decode step: same-process A/B of a sampling session's step against the same session made with
stop_sequences=True, hipGraph replay, tools/bench_constraint_step.py's protocol: every arm captured once, the arms timed alternately,
`--rounds` rounds of `--steps` replays each.

    python tools/bench_stop_step.py --tenants 6 --kv-len 512 > profiles/stop_sequence_step.txt

Arms: sample / sample_b (the sampling session's graph twice, every tenant at tau = 1, top_k = 50, top_p = 0.9: the run's own A/A spread),
ss_none (the same with stop_sequences=True at the default sizes and no sequence on any tenant: one more launch, step_stop_sequences, at the
very end of the step), ss_4x8 (every tenant with 4 random sequences of 8 tokens), ss_16x32 (a session of the ABI's largest sizes, every
tenant with 16 random sequences of 32 tokens).  Random sequences over the whole vocabulary do not occur in sampled text, so nobody retires
(asserted).  Then the device time of the launch alone behind a one-element add that moves the counter (and that add alone): tables of 4 x 8
and 16 x 32, empty, random (a pair is decided by its first comparison) and the worst case -- a row of one repeated token under sequences of
that token with another last id, so that every (sequence, length) pair compares its whole length and nothing ever hits -- and with a counter
that did not move; step_end_sample re-measured next to them."""
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
    from bitdelta_amd.serving_loop import TenantDecoder
    dev = torch.device("cuda", 0)
    T = args.tenants
    assert max(args.warm_steps, args.steps + 1) < 256, "the arms must not run into the end of the cache (kv-len + 256 rows)"
    dec = TenantDecoder.synthetic(args.model, T, dev, dtype=torch.float16, seed=4321, layers=args.layers, max_len=args.kv_len + 256)
    vocab = dec.cfg[5]
    g = torch.Generator().manual_seed(4321)
    prompts = [torch.randint(1, vocab, (args.kv_len,), generator=g).tolist() for _ in range(T)]
    rand_seqs = lambda q, w: [[torch.randint(1, vocab, (w,), generator=g).tolist() for _ in range(q)] for _ in range(T)]

    arms = {}

    def arm(name, kw, seqs):
        sess = dec.session(sampling=True, **kw)
        sess.submit_all(prompts, max_new_tokens=1 << 30, seed=list(range(1, T + 1)), **SAMPLE, **({"stop_sequences": seqs} if seqs else {}))
        assert all(sess.active())
        snap = [v.clone() for v in sess._state()]

        def restore():
            for v, s_ in zip(sess._state(), snap):
                v.copy_(s_)
        run = sess._runner()
        restore()
        arms[name] = (run, restore, sess)
    arm("sample", {}, None)
    arms["sample_b"] = arms["sample"]
    arm("ss_none", dict(stop_sequences=True), None)
    arm("ss_4x8", dict(stop_sequences=True), rand_seqs(4, 8))
    arm("ss_16x32", dict(stop_sequences=True, max_stop_sequences=16, max_stop_sequence_len=32), rand_seqs(16, 32))
    arms = {n: arms[n] for n in ("sample", "ss_none", "ss_4x8", "ss_16x32", "sample_b")}
    for run, restore, _ in arms.values():
        restore()
        for _ in range(args.warm_steps):
            run()
    torch.cuda.synchronize()
    assert all(all(s.active()) for _, _, s in arms.values()), "a tenant retired during the warm-up: the arm would time an idle step"
    ms = {n: [] for n in arms}
    for _ in range(args.rounds):
        for n, (run, restore, _) in arms.items():
            restore()
            run()
            ms[n].append(bdd.timed_region(run, args.steps, device_sync=torch.cuda.synchronize) / args.steps * 1e3)
    assert all(all(s.active()) for _, _, s in arms.values())
    med = {n: sorted(v)[len(v) // 2] for n, v in ms.items()}
    base = (med["sample"] + med["sample_b"]) / 2

    # the launch alone: device time per launch, the counter moved by a one-element add in front of it so that every launch does its work
    cap = 8192
    assert 3 + 6 * args.kernel_iters < cap, "the counter must stay inside the row: past it the launch compares nothing"
    out = torch.full((T, cap), 7, dtype=torch.long, device=dev)
    out_rand = torch.randint(1, vocab, (T, cap), generator=g).to(dev)

    def state(Q, W, seqs):
        tok = torch.full((T, Q, W), -1, dtype=torch.int32)
        lens = torch.zeros(T, Q, dtype=torch.int32)
        for t, ss in enumerate(seqs or []):
            for q, s_ in enumerate(ss):
                tok[t, q, :len(s_)] = torch.tensor(s_, dtype=torch.int32)
                lens[t, q] = len(s_)
        return dict(tok=tok.to(dev), lens=lens.to(dev), n=torch.zeros(T, dtype=torch.long, device=dev), ss_n=torch.zeros(T, dtype=torch.long, device=dev),
                    hit=torch.full((T,), -1, dtype=torch.int32, device=dev), hold=torch.zeros(T, dtype=torch.int32, device=dev),
                    act=torch.ones(T, dtype=torch.bool, device=dev), done=torch.zeros(T, dtype=torch.uint8, device=dev))
    worst = lambda q, w: [[[7] * (w - 1) + [8]] * q] * T
    cases = {"4x8/empty": (out_rand, state(4, 8, None)), "4x8/random": (out_rand, state(4, 8, rand_seqs(4, 8))),
             "4x8/every_pair_compares_its_whole_length": (out, state(4, 8, worst(4, 8))),
             "16x32/empty": (out_rand, state(16, 32, None)), "16x32/random": (out_rand, state(16, 32, rand_seqs(16, 32))),
             "16x32/every_pair_compares_its_whole_length": (out, state(16, 32, worst(16, 32)))}

    def launch(o, s, move=True):
        def fn():
            if move:
                s["n"].add_(1)
            ops.step_stop_sequences(o, s["n"], s["ss_n"], s["tok"], s["lens"], s["hit"], s["hold"], s["act"], s["done"])
        return fn

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
    kern = {"add_1+step_stop_sequences/" + n: kernel_us(launch(o, s)) for n, (o, s) in cases.items()}
    for n, (o, s) in cases.items():
        assert int(s["n"].max()) <= cap and s["ss_n"].tolist() == s["n"].tolist() and all(s["act"].tolist()) and s["hit"].tolist() == [-1] * T, n
    w8, w32 = cases["4x8/every_pair_compares_its_whole_length"][1], cases["16x32/every_pair_compares_its_whole_length"][1]
    assert w8["hold"].tolist() == [7] * T and w32["hold"].tolist() == [31] * T
    one = torch.zeros(1, dtype=torch.long, device=dev)
    kern["add_1"] = kernel_us(lambda: one.add_(1))
    kern["step_stop_sequences/16x32/counter_did_not_move"] = kernel_us(launch(out, w32, move=False))
    logits = (torch.randn(T, vocab, generator=g) * 3).half().to(dev)
    big = lambda: torch.full((T,), 1 << 40, dtype=torch.long, device=dev)
    st = dict(tok=torch.zeros(T, 1, dtype=torch.long, device=dev), out=torch.zeros(T, 8, dtype=torch.long, device=dev),
              n=torch.zeros(T, dtype=torch.long, device=dev), pos=torch.zeros(T, dtype=torch.long, device=dev), limit=big(),
              stop=torch.full((T, 8), -1, dtype=torch.long, device=dev), act=torch.ones(T, dtype=torch.bool, device=dev),
              done=torch.zeros(T, dtype=torch.uint8, device=dev))
    tau = torch.full((T,), 1.0, dtype=torch.float32, device=dev)
    k = torch.full((T,), 50, dtype=torch.int32, device=dev)
    pp = torch.full((T,), 0.9, dtype=torch.float32, device=dev)
    seed = torch.arange(1, T + 1, dtype=torch.long, device=dev)
    kern["step_end_sample/k50_p90"] = kernel_us(lambda: ops.step_end_sample(logits, st["tok"], st["out"], st["n"], st["pos"], st["limit"], st["stop"],
                                                                            st["act"], st["done"], 1 << 30, tau, k, pp, seed))
    res = {"model": args.model, "tenants": T, "kv_len": args.kv_len, "layers": len(dec.layers), "vocab": vocab, "steps": args.steps,
           "rounds": args.rounds, "arms": {n: {"min_ms": min(v), "median_ms": med[n], "all_ms": [round(x, 4) for x in v]} for n, v in ms.items()},
           "aa_spread_sample_pct": abs(med["sample_b"] / med["sample"] - 1) * 100,
           "over_sample_pct": {n: (med[n] / base - 1) * 100 for n in arms if n.startswith("ss")},
           "over_sample_us": {n: (med[n] - base) * 1e3 for n in arms if n.startswith("ss")},
           "launch_us_in_graph": {n: round(v, 3) for n, v in kern.items()}}
    print(json.dumps(res))
    for n, a in res["arms"].items():
        print(f"# {n:16s} min {a['min_ms']:.4f}  median {a['median_ms']:.4f} ms/step", file=sys.stderr)
    print(f"# A/A spread (sample): {res['aa_spread_sample_pct']:.2f} %;  over the sampling session's step: " +
          ", ".join(f"{n} {v:+.2f} % ({res['over_sample_us'][n]:+.1f} us)" for n, v in res["over_sample_pct"].items()), file=sys.stderr)
    for n, v in res["launch_us_in_graph"].items():
        print(f"# {n:64s} {v:8.3f} us per launch (a chain of launches in one graph)", file=sys.stderr)


if __name__ == "__main__":
    main()
