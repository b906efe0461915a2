#!/usr/bin/env python3
"""What the tail truncation (min_p / typical_p / epsilon_cutoff / eta_cutoff) costs a decode step: same-process A/B of a sampling session's step
against the same session made with truncation=True, hipGraph replay, tools/bench_ban_step.py's protocol: every arm captured once, the arms
timed alternately, `--rounds` rounds of `--steps` replays each.

    python tools/bench_truncation_step.py --tenants 6 --kv-len 512 > profiles/truncation_step.txt

Arms: sample / sample_b (the sampling session's graph twice, every tenant at tau = 1, top_k = 50, top_p = 0.9: the run's own A/A spread),
trunc_neutral (the same with truncation=True and neutral parameters: one more launch, step_truncate, in front of the step end: a copy),
trunc_min_p (every tenant with min_p = 0.05), trunc_typical (typical_p = 0.9), trunc_eta (eta_cutoff = 3e-4), trunc_all (all four set).  Nobody
retires (asserted).  Then the device time of the launch alone at each setting -- a chain of launches in one captured graph, on N(0, 3) rows --
with the number of elements it keeps, next to step_end_sample on the raw row AND on each truncated row: the sampling kernel is slower on rows
with few finite elements, and these filters produce such rows."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

SAMPLE = dict(temperature=1.0, top_k=50, top_p=0.9)
SETTINGS = {"neutral": {}, "min_p": dict(min_p=0.05), "typical": dict(typical_p=0.9), "eta": dict(eta_cutoff=3e-4),
            "all": dict(min_p=0.05, typical_p=0.9, epsilon_cutoff=3e-4, eta_cutoff=3e-4), "epsilon": dict(epsilon_cutoff=3e-4)}


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
    from bitdelta_amd.serving_loop import TenantDecoder, truncation_params
    dev = torch.device("cuda", 0)
    T = args.tenants
    assert max(args.warm_steps, args.steps + 1) < 256, "the arms must not run into the end of the cache (kv-len + 256 rows)"
    dec = TenantDecoder.synthetic(args.model, T, dev, dtype=torch.float16, seed=4321, layers=args.layers, max_len=args.kv_len + 256)
    vocab = dec.cfg[5]
    g = torch.Generator().manual_seed(4321)
    prompts = [torch.randint(1, vocab, (args.kv_len,), generator=g).tolist() for _ in range(T)]

    arms = {}

    def arm(name, kw, req):
        sess = dec.session(sampling=True, **kw)
        sess.submit_all(prompts, max_new_tokens=1 << 30, seed=list(range(1, T + 1)), **SAMPLE, **req)
        assert all(sess.active())
        snap = [v.clone() for v in sess._state()]

        def restore():
            for v, s_ in zip(sess._state(), snap):
                v.copy_(s_)
        run = sess._runner()
        restore()
        arms[name] = (run, restore, sess)
    arm("sample", {}, {})
    arms["sample_b"] = arms["sample"]
    order = ("neutral", "min_p", "typical", "eta", "all")
    for n in order:
        arm("trunc_" + n, dict(truncation=True), SETTINGS[n])
    arms = {n: arms[n] for n in ("sample",) + tuple("trunc_" + n for n in order) + ("sample_b",)}
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
    # what the filters kept in the sessions' own last step (the synthetic model's rows), mean over the tenants
    kept_session = {n: float(torch.isfinite(s.tlogits.float()).sum(1).float().mean()) for n, (_, _, s) in arms.items() if n.startswith("trunc")}

    # the launch alone: device time per launch; it is a pure function of its inputs, so a chain of identical launches does the same work each time
    logits = (torch.randn(T, vocab, generator=g) * 3).half().to(dev)
    act = torch.ones(T, dtype=torch.bool, device=dev)
    tau = torch.full((T,), 1.0, dtype=torch.float32, device=dev)
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

    big = lambda: torch.full((T,), 1 << 40, dtype=torch.long, device=dev)
    st = dict(tok=torch.zeros(T, 1, dtype=torch.long, device=dev), out=torch.zeros(T, 8, dtype=torch.long, device=dev),
              n=torch.zeros(T, dtype=torch.long, device=dev), pos=torch.zeros(T, dtype=torch.long, device=dev), limit=big(),
              stop=torch.full((T, 8), -1, dtype=torch.long, device=dev), act=torch.ones(T, dtype=torch.bool, device=dev),
              done=torch.zeros(T, dtype=torch.uint8, device=dev))
    k = torch.full((T,), 50, dtype=torch.int32, device=dev)
    pp = torch.full((T,), 0.9, dtype=torch.float32, device=dev)
    seed = torch.arange(1, T + 1, dtype=torch.long, device=dev)
    end = lambda row: (lambda: ops.step_end_sample(row, st["tok"], st["out"], st["n"], st["pos"], st["limit"], st["stop"], st["act"], st["done"],
                                                   1 << 30, tau, k, pp, seed))
    kern, kept = {}, {}
    kern["step_end_sample/k50_p90/raw_row"] = kernel_us(end(logits))
    for n in ("neutral", "min_p", "epsilon", "typical", "eta", "all"):
        prm = torch.tensor([truncation_params(**SETTINGS[n])] * T, dtype=torch.float32).to(dev)
        out = torch.empty_like(logits)
        kern["step_truncate/" + n] = kernel_us(lambda: ops.step_truncate(logits, out, tau, prm, act))
        kern["truncate_rows/" + n] = kernel_us(lambda: ops.truncate_rows(logits, tau, prm, out=out))
        torch.cuda.synchronize()
        kept[n] = float(torch.isfinite(out.float()).sum(1).float().mean())
        kern["step_end_sample/k50_p90/after_" + n] = kernel_us(end(out))
    res = {"model": args.model, "tenants": T, "kv_len": args.kv_len, "layers": len(dec.layers), "vocab": vocab, "steps": args.steps,
           "rounds": args.rounds, "arms": {n: {"min_ms": min(v), "median_ms": med[n], "all_ms": [round(x, 4) for x in v]} for n, v in ms.items()},
           "aa_spread_sample_pct": abs(med["sample_b"] / med["sample"] - 1) * 100,
           "over_sample_pct": {n: (med[n] / base - 1) * 100 for n in arms if n.startswith("trunc")},
           "over_sample_us": {n: (med[n] - base) * 1e3 for n in arms if n.startswith("trunc")},
           "kept_per_row_in_the_sessions_last_step": kept_session,
           "launch_us_in_graph": {n: round(v, 3) for n, v in kern.items()}, "kept_per_row_of_the_launch_alone": kept}
    print(json.dumps(res))
    for n, a in res["arms"].items():
        print(f"# {n:16s} min {a['min_ms']:.4f}  median {a['median_ms']:.4f} ms/step", file=sys.stderr)
    print(f"# A/A spread (sample): {res['aa_spread_sample_pct']:.2f} %;  over the sampling session's step: " +
          ", ".join(f"{n} {v:+.2f} % ({res['over_sample_us'][n]:+.1f} us)" for n, v in res["over_sample_pct"].items()), file=sys.stderr)
    print("# kept per row in the sessions' last step: " + ", ".join(f"{n} {v:.0f}" for n, v in kept_session.items()), file=sys.stderr)
    for n, v in res["launch_us_in_graph"].items():
        print(f"# {n:64s} {v:8.3f} us per launch (a chain of launches in one graph)", file=sys.stderr)
    print("# kept per row of the launch alone (N(0, 3) rows): " + ", ".join(f"{n} {v:.0f}" for n, v in kept.items()), file=sys.stderr)


if __name__ == "__main__":
    main()
