#!/usr/bin/env python3
"""What the token-automaton constraint costs a decode step: same-process A/B of a sampling session's step against the same session made with
constraints=True, hipGraph replay, tools/bench_penalty_step.py's protocol: every arm captured once, the arms timed alternately, `--rounds`
rounds of `--steps` replays each.

    python tools/bench_constraint_step.py --tenants 6 --kv-len 512 > profiles/constraint_step.txt

Arms: sample / sample_b (the sampling session's graph twice, every tenant at tau = 1, top_k = 50, top_p = 0.9: the run's own A/A spread),
con_none (the same with constraints=True and no constraint on any tenant, state = -1: two more launches, step_constrain in front of
step_end_sample and step_constrain_advance behind it), con_trie (every tenant under 64 choices of 4 tokens each -- as a ring: the last edge of
every choice leads back to the root instead of to a final leaf, so that the tenants keep generating for the whole run; the states, the slices
and the searches are the trie's: a root of 64 edges, one edge everywhere else), con_set (every tenant under allowed_set of 4096 tokens: one
state whose slice is the session's whole edge array).  Then the device time of the launches alone on the step's own shape [tenants, vocab]
with N(0, 3^2) logits: step_constrain in the three situations, constrain_rows, step_constrain_advance (behind a one-element add that moves the
counter, and that add alone), step_penalize / step_end_sample re-measured next to them, and step_end_sample on rows the mask has
left 1 / 64 / 4096 finite elements in: the sampling launch's own time depends on the row it is given."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

SAMPLE = dict(temperature=1.0, top_k=50, top_p=0.9)


def ring_of_choices(TokenAutomaton, vocab, g, choices=64, length=4):
    """`choices` random token lists of `length` tokens with distinct first tokens, as an automaton whose last edges lead back to the root"""
    firsts = torch.randperm(vocab, generator=g)[:choices].tolist()
    edges, nstates = [], 1
    for f in firsts:
        s = 0
        for j, y in enumerate([f] + torch.randint(0, vocab, (length - 1,), generator=g).tolist()):
            nx = 0 if j == length - 1 else nstates
            edges.append((s, y, nx))
            if nx:
                nstates += 1
            s = nx
    return TokenAutomaton.from_edges(nstates, edges, [0] * nstates)


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
    from bitdelta_amd.constraint import TokenAutomaton
    from bitdelta_amd.serving_loop import TenantDecoder, penalty_row
    dev = torch.device("cuda", 0)
    T = args.tenants
    assert max(args.warm_steps, args.steps + 1) < 256, "the arms must not run into the end of the cache (kv-len + 256 rows)"
    dec = TenantDecoder.synthetic(args.model, T, dev, dtype=torch.float16, seed=4321, layers=args.layers, max_len=args.kv_len + 256)
    vocab = dec.cfg[5]
    g = torch.Generator().manual_seed(4321)
    prompts = [torch.randint(1, vocab, (args.kv_len,), generator=g).tolist() for _ in range(T)]
    trie = [ring_of_choices(TokenAutomaton, vocab, g) for _ in range(T)]
    aset = [TokenAutomaton.allowed_set(torch.randperm(vocab, generator=g)[:4096].tolist()) for _ in range(T)]

    arms = {}

    def arm(name, constraints, cons):
        sess = dec.session(sampling=True, constraints=constraints)
        sess.submit_all(prompts, max_new_tokens=1 << 30, seed=list(range(1, T + 1)), **SAMPLE, **({"constraint": cons} if constraints else {}))
        assert all(sess.active())
        snap = [v.clone() for v in sess._state()]

        def restore():
            for v, s_ in zip(sess._state(), snap):
                v.copy_(s_)
        run = sess._runner()
        restore()
        arms[name] = (run, restore, sess)
    arm("sample", False, None)
    arms["sample_b"] = arms["sample"]
    arm("con_none", True, None)
    arm("con_trie", True, trie)
    arm("con_set", True, aset)
    arms = {n: arms[n] for n in ("sample", "con_none", "con_trie", "con_set", "sample_b")}
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

    # the launches alone: device time per launch on the step's shape, the automata at the session's default sizes
    S, E = 256, 4096
    logits = (torch.randn(T, vocab, generator=g) * 3).half().to(dev)
    clogits = torch.zeros_like(logits)

    def packed(autos):
        off = torch.zeros(T, S + 1, dtype=torch.int32)
        etok, enext, acc = torch.zeros(T, E, dtype=torch.int32), torch.zeros(T, E, dtype=torch.int32), torch.zeros(T, S, dtype=torch.uint8)
        for t, a in enumerate(autos):
            off[t, :a.n_states + 1] = torch.tensor(a.off, dtype=torch.int32)
            off[t, a.n_states + 1:] = a.off[-1]
            etok[t, :a.n_edges] = torch.tensor(a.edge_tok, dtype=torch.int32)
            enext[t, :a.n_edges] = torch.tensor(a.edge_next, dtype=torch.int32)
            acc[t, :a.n_states] = torch.tensor(a.accepting, dtype=torch.uint8)
        return off.to(dev), etok.to(dev), enext.to(dev), acc.to(dev)
    p_trie, p_set = packed(trie), packed(aset)
    act = torch.ones(T, dtype=torch.bool, device=dev)
    stops = torch.full((T, 8), -1, dtype=torch.long, device=dev)
    free = torch.full((T,), -1, dtype=torch.int32, device=dev)
    root = torch.zeros(T, dtype=torch.int32, device=dev)
    big = lambda: torch.full((T,), 1 << 40, dtype=torch.long, device=dev)
    st = dict(tok=torch.zeros(T, 1, dtype=torch.long, device=dev), out=torch.zeros(T, 8, dtype=torch.long, device=dev),
              n=torch.zeros(T, dtype=torch.long, device=dev), pos=torch.zeros(T, dtype=torch.long, device=dev), limit=big(),
              stop=torch.full((T, 8), -1, dtype=torch.long, device=dev), act=torch.ones(T, dtype=torch.bool, device=dev),
              done=torch.zeros(T, dtype=torch.uint8, device=dev))
    tau = torch.full((T,), 1.0, dtype=torch.float32, device=dev)
    k = torch.full((T,), 50, dtype=torch.int32, device=dev)
    pp = torch.full((T,), 0.9, dtype=torch.float32, device=dev)
    seed = torch.arange(1, T + 1, dtype=torch.long, device=dev)
    hist = torch.zeros(T, vocab, dtype=torch.int16, device=dev)
    pen_n = torch.tensor([penalty_row((1.0, 0.0, 0.0, ()))] * T, dtype=torch.float32).to(dev)
    # the advance launch: a token of each tenant's set (a self-loop: the search runs over 4096 edges and the state stays), the counter moved by an add
    a_tok = torch.tensor([[a.edge_tok[1234]] for a in aset], dtype=torch.long).to(dev)
    a_n, a_cn = torch.zeros(T, dtype=torch.long, device=dev), torch.zeros(T, dtype=torch.long, device=dev)
    a_state, a_act, a_done = torch.zeros(T, dtype=torch.int32, device=dev), torch.ones(T, dtype=torch.bool, device=dev), torch.zeros(T, dtype=torch.uint8, device=dev)

    def advance_after_add():
        a_n.add_(1)
        ops.step_constrain_advance(a_tok, a_n, a_cn, a_state, p_set[0], p_set[1], p_set[2], p_set[3], a_act, a_done)

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
        "step_constrain/none": kernel_us(lambda: ops.step_constrain(logits, clogits, free, p_trie[0], p_trie[1], p_trie[3], stops, act)),
        "step_constrain/trie_root_64_edges": kernel_us(lambda: ops.step_constrain(logits, clogits, root, p_trie[0], p_trie[1], p_trie[3], stops, act)),
        "step_constrain/set_4096_edges": kernel_us(lambda: ops.step_constrain(logits, clogits, root, p_set[0], p_set[1], p_set[3], stops, act)),
        "constrain_rows/set_4096_edges": kernel_us(lambda: ops.constrain_rows(logits, root, p_set[0], p_set[1], p_set[3], stops, out=clogits)),
        "add_1+step_constrain_advance/set_4096_edges": kernel_us(advance_after_add),
        "add_1": kernel_us(lambda: a_n.add_(1)),
        "step_constrain_advance/counter_did_not_move": kernel_us(lambda: ops.step_constrain_advance(a_tok, a_n, a_cn, a_state, p_set[0], p_set[1], p_set[2],
                                                                                                p_set[3], a_act, a_done)),
        "step_penalize/neutral": kernel_us(lambda: ops.step_penalize(logits, clogits, hist, st["tok"], act, pen_n)),
        "step_end_sample/k50_p90": kernel_us(lambda: ops.step_end_sample(logits, st["tok"], st["out"], st["n"], st["pos"], st["limit"], st["stop"],
                                                                         st["act"], st["done"], 1 << 30, tau, k, pp, seed)),
    }
    assert a_state.tolist() == [0] * T and all(a_act.tolist()) and a_cn.tolist() == a_n.tolist()
    # what the unchanged sampling launch takes on a MASKED row: its radix select and its masses see a row that is -inf but for 1 / 64 / 4096 elements
    one = torch.ones(T, dtype=torch.int32, device=dev)                  # state 1 of the ring: a single edge
    for name, state, p in (("1_token", one, p_trie), ("64_tokens", root, p_trie), ("4096_tokens", root, p_set)):
        masked = ops.constrain_rows(logits, state, p[0], p[1], p[3], stops)
        kern["step_end_sample/k50_p90/row_masked_to_" + name] = kernel_us(
            lambda: ops.step_end_sample(masked, st["tok"], st["out"], st["n"], st["pos"], st["limit"], st["stop"], st["act"], st["done"], 1 << 30,
                                        tau, k, pp, seed))
    moved = T * vocab * 4
    out = {"model": args.model, "tenants": T, "kv_len": args.kv_len, "layers": len(dec.layers), "vocab": vocab, "steps": args.steps,
           "rounds": args.rounds, "arms": {n: {"min_ms": min(v), "median_ms": med[n], "all_ms": [round(x, 4) for x in v]} for n, v in ms.items()},
           "aa_spread_sample_pct": abs(med["sample_b"] / med["sample"] - 1) * 100,
           "over_sample_pct": {n: (med[n] / base - 1) * 100 for n in arms if n.startswith("con")},
           "over_sample_us": {n: (med[n] - base) * 1e3 for n in arms if n.startswith("con")},
           "launch_us_in_graph": {n: round(v, 3) for n, v in kern.items()}, "mask_launch_bytes": moved}
    print(json.dumps(out))
    for n, a in out["arms"].items():
        print(f"# {n:16s} min {a['min_ms']:.4f}  median {a['median_ms']:.4f} ms/step", file=sys.stderr)
    print(f"# A/A spread (sample): {out['aa_spread_sample_pct']:.2f} %;  over the sampling session's step: " +
          ", ".join(f"{n} {v:+.2f} % ({out['over_sample_us'][n]:+.1f} us)" for n, v in out["over_sample_pct"].items()), file=sys.stderr)
    for n, v in out["launch_us_in_graph"].items():
        print(f"# {n:52s} {v:8.3f} us per launch (a chain of launches in one graph; the mask moves {moved} bytes of logits)", file=sys.stderr)


if __name__ == "__main__":
    main()
