"""The protocol the step A/B tools (tools/bench_*_step.py) share: same-process A/B of captured session steps, hipGraph replay.  A tool makes its
arms -- one session each, admitted, nobody retiring -- and hands each to `capture`; `time_arms` warms every arm and then times the arms alternately,
`--rounds` rounds of `--steps` replays each; `kernel_timer` gives the device time of one launch from a chain of them in one captured graph.  What
the arms are, the command line's defaults, the JSON keys and the stderr lines stay with each tool."""
import argparse
import sys

import torch


def parse_args(kv_len=512, warm_steps=200, kernel_iters=200):
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="mistral-7b")
    ap.add_argument("--tenants", type=int, default=6)
    ap.add_argument("--kv-len", type=int, default=kv_len)
    ap.add_argument("--layers", type=int, default=None)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--warm-steps", type=int, default=warm_steps, help="replays of every arm before the first timed round (clocks)")
    ap.add_argument("--kernel-iters", type=int, default=kernel_iters)
    args = ap.parse_args()
    assert max(args.warm_steps, args.steps + 1) < 256, "the arms must not run into the end of the cache (kv-len + 256 rows)"
    return args


def capture(sess):
    """(run, restore) of an admitted session: its state is snapshot, the step captured (TenantSession._runner) and the state put back; restore()
    puts it back again, so every timed window replays the same steps"""
    snap = [v.clone() for v in sess._state()]

    def restore():
        for v, s_ in zip(sess._state(), snap):
            v.copy_(s_)
    run = sess._runner()
    restore()
    return run, restore


def time_arms(arms, args, sessions=()):
    """arms: {name: (run, restore)} in the order they are timed.  Every arm is warmed, then the arms are timed alternately.  sessions: the ones
    that must still have every tenant active after the warm-up and at the end.  Returns (ms, med): per arm the ms/step of every round, and
    their median."""
    from bitdelta_amd import dist as bdd
    for run, restore in arms.values():
        restore()
        for _ in range(args.warm_steps):
            run()
    torch.cuda.synchronize()
    assert all(all(s.active()) for s in sessions), "a tenant retired during the warm-up: the arm would time an idle step"
    ms = {n: [] for n in arms}
    for _ in range(args.rounds):
        for n, (run, restore) in arms.items():
            restore()
            run()
            ms[n].append(bdd.timed_region(run, args.steps, device_sync=torch.cuda.synchronize) / args.steps * 1e3)
    assert all(all(s.active()) for s in sessions)
    return ms, {n: sorted(v)[len(v) // 2] for n, v in ms.items()}


def arms_json(ms, med):
    """the "arms" entry of a tool's JSON line"""
    return {n: {"min_ms": min(v), "median_ms": med[n], "all_ms": [round(x, 4) for x in v]} for n, v in ms.items()}


def print_arms(arms, width):
    for n, a in arms.items():
        print(f"# {n:{width}s} min {a['min_ms']:.4f}  median {a['median_ms']:.4f} ms/step", file=sys.stderr)


def kernel_timer(dev, iters):
    """kernel_us(fn): `iters` launches in a row inside ONE captured graph (no host in the loop): replay time / launches, median of 5 replays"""
    side = torch.cuda.Stream(device=dev)

    def kernel_us(fn):
        side.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.stream(side):
            for _ in range(3):
                fn()
        torch.cuda.synchronize()
        gr = torch.cuda.CUDAGraph()
        with torch.cuda.graph(gr, stream=side):
            for _ in range(iters):
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
            times.append(e0.elapsed_time(e1) / iters * 1e3)
        return sorted(times)[len(times) // 2]
    return kernel_us

