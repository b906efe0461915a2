#!/usr/bin/env python3
"""What the hard bans (no_repeat_ngram_size / bad_words / min_new_tokens) cost a decode step: same-process A/B of a sampling session's step
against the same session made with bans=True, hipGraph replay, tools/bench_stop_step.py's protocol: every arm captured once, the arms timed
alternately, `--rounds` rounds of `--steps` replays each.

    python tools/bench_ban_step.py --tenants 6 --kv-len 1024 > profiles/ban_step.txt

Arms: sample / sample_b (the sampling session's graph twice, every tenant at tau = 1, top_k = 50, top_p = 0.9: the run's own A/A spread),
ban_none (the same with bans=True and neutral parameters: one more launch, step_ban, in front of the step end), ban_ngram3 (every tenant with
no_repeat_ngram_size = 3 over its --kv-len-token prompt: the launch walks the whole history in every block), ban_words16x8 (every tenant with
16 random bad words of 8 ids), ban_all (both, and min_new_tokens past the run with one stop id).  Nobody retires (asserted).  Then the device
time of the launch alone at each setting -- a chain of launches in one captured graph -- next to step_constrain without a constraint (the same
masked copy without a search) and step_end_sample."""
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
    ap.add_argument("--kv-len", type=int, default=1024)
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
    rand_words = lambda q, w: [[torch.randint(1, vocab, (w,), generator=g).tolist() for _ in range(q)] for _ in range(T)]

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
    on = dict(bans=True, max_bad_words=16, max_bad_word_len=8)
    words = rand_words(16, 8)
    arm("sample", {}, {})
    arms["sample_b"] = arms["sample"]
    arm("ban_none", on, {})
    arm("ban_ngram3", on, dict(no_repeat_ngram_size=3))
    arm("ban_words16x8", on, dict(bad_words=words))
    arm("ban_all", on, dict(no_repeat_ngram_size=3, bad_words=words, min_new_tokens=1 << 20, stop_token_ids=[[2]] * T))
    arms = {n: arms[n] for n in ("sample", "ban_none", "ban_ngram3", "ban_words16x8", "ban_all", "sample_b")}
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

    # the launch alone: device time per launch; it is a pure function of its inputs, so a chain of identical launches does the same work each time
    Lc, cap, n_out = args.kv_len + 256, args.kv_len + 256, 200
    logits = (torch.randn(T, vocab, generator=g) * 3).half().to(dev)
    out = torch.empty_like(logits)
    ctx = torch.randint(1, vocab, (T, Lc), generator=g).int().to(dev)
    toks = torch.randint(1, vocab, (T, cap), generator=g).to(dev)
    act = torch.ones(T, dtype=torch.bool, device=dev)
    stops = torch.full((T, 8), -1, dtype=torch.long, device=dev)
    stops[:, 0] = 2
    i32 = lambda v: torch.full((T,), v, dtype=torch.int32, device=dev)

    def table(Q, W, ws):
        tok = torch.full((T, Q, W), -1, dtype=torch.int32)
        lens = torch.zeros(T, Q, dtype=torch.int32)
        for t, row in enumerate(ws or []):
            for q, w in enumerate(row):
                tok[t, q, :len(w)] = torch.tensor(w, dtype=torch.int32)
                lens[t, q] = len(w)
        return tok.to(dev), lens.to(dev)
    empty16, words16, words64 = table(16, 8, None), table(16, 8, words), table(64, 32, rand_words(64, 32))
    # a history that is one repeated token: every candidate of the n-gram walk compares its whole tail and bans (the worst case of the walk)
    same = torch.full((T, Lc), 7, dtype=torch.int32, device=dev)
    same_toks = torch.full((T, cap), 7, dtype=torch.long, device=dev)
    n_t = torch.full((T,), n_out, dtype=torch.long, device=dev)
    cases = {
        "neutral": (ctx, toks, i32(args.kv_len), i32(0), empty16, i32(0)),
        "ngram3/history_%d+%d" % (args.kv_len, n_out): (ctx, toks, i32(args.kv_len), i32(3), empty16, i32(0)),
        "ngram8/history_%d+%d" % (args.kv_len, n_out): (ctx, toks, i32(args.kv_len), i32(8), empty16, i32(0)),
        "ngram8/history_%d+%d/one_repeated_token" % (args.kv_len, n_out): (same, same_toks, i32(args.kv_len), i32(8), empty16, i32(0)),
        "words16x8": (ctx, toks, i32(args.kv_len), i32(0), words16, i32(0)),
        "words64x32": (ctx, toks, i32(args.kv_len), i32(0), words64, i32(0)),
        "ngram3+words16x8+min_new": (ctx, toks, i32(args.kv_len), i32(3), words16, i32(1 << 20)),
    }

    def launch(c, h, cl, ng, tab, mn):
        return lambda: ops.step_ban(logits, out, c, cl, h, n_t, ng, tab[0], tab[1], mn, stops, act)

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
    kern = {"step_ban/" + n: kernel_us(launch(*c)) for n, c in cases.items()}
    r_len, r_g, r_min = i32(args.kv_len), i32(3), i32(1)
    kern["ban_rows/ngram3+words16x8+min_new/n_absent"] = kernel_us(
        lambda: ops.ban_rows(logits, ctx, r_len, r_g, words16[0], words16[1], r_min, stops, out=out))
    S, E = 4, 8
    c_state = torch.full((T,), -1, dtype=torch.int32, device=dev)
    c_off, c_tok = torch.zeros(T, S + 1, dtype=torch.int32, device=dev), torch.zeros(T, E, dtype=torch.int32, device=dev)
    c_acc = torch.zeros(T, S, dtype=torch.uint8, device=dev)
    kern["step_constrain/no_constraint"] = kernel_us(lambda: ops.step_constrain(logits, out, c_state, c_off, c_tok, c_acc, stops, act))
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
           "over_sample_pct": {n: (med[n] / base - 1) * 100 for n in arms if n.startswith("ban")},
           "over_sample_us": {n: (med[n] - base) * 1e3 for n in arms if n.startswith("ban")},
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
