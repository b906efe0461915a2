"""The prefill-size GEMM dispatch, pinned WITHOUT a GPU (csrc/bd_api.hip: tile_plan decides, launch_tile_plan lifts each planned launch to one
row of TILE_ROWS).  Every tile form computes the same result, so the output tests cannot see a call that takes the wrong tile, slice count, tail
column, grid or LDS size -- it is only slower -- and a workspace that is too small silently keeps the unsplit variant.  tests/golden/tile_dispatch.txt
records the decisions (tests/golden/make_tile_dispatch_golden.py: the real entry points in dry-run mode); the recorded cases are replayed against the
built library and must agree line by line.  (The set of tile kernels the library compiles is pinned next to the streaming kernel's, in
tests/test_stream_dispatch.py.)"""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
sys.path.insert(0, GOLDEN)
import make_tile_dispatch_golden as sweep  # noqa: E402


def golden_lines():
    with open(sweep.OUT) as fh:
        return [l.rstrip("\n") for l in fh if l.strip()]


def test_sweep_reaches_every_variant_and_arm_and_refuses_enough():
    lines = golden_lines()
    missing, arms, refusals, seen = sweep.coverage(lines)
    assert not missing, f"shipped variants no accepted case reaches: {missing}"
    assert not arms, f"automatic arms no case reaches: {arms}"
    assert seen["dtype"] == {0, 1} and seen["f32"] == {0, 1} and seen["ws"] == {"W", "w", "s", "0"}, seen
    assert refusals >= 0.10, refusals
    # the refusals the dispatch owns: forced variants on the wrong kind of call and A/B-only ones, accumulate where no epilogue takes it,
    # bad alignment under a forced tile, a missing workspace under a forced split
    codes = {(sweep.inputs_of(l)[0], sweep.inputs_of(l)[8], l.split("|")[1].split()[0]) for l in lines}
    for want in (("lin", 13, "-5"), ("bmm", 8, "-5"), ("lin", 4, "-5"), ("lin", 6, "-5"), ("bmm", 7, "-5"), ("lin", 0, "-5"), ("lin", 5, "-5"),
                 ("res", 10, "-5"), ("res", 1, "-5"), ("linu", 9, "-5"), ("lin", 10, "-6"), ("lin", 19, "-6"), ("sw", 14, "-5"), ("lin", 15, "-5")):
        assert want in codes, want
    assert os.path.getsize(sweep.OUT) <= os.path.getsize(os.path.join(GOLDEN, "stream_dispatch.txt"))
    assert all(f"{e} {'hb'[dt]} {f32} {B} {M} {N} {K} w -1 0 " in "\n".join(lines) for e, dt, f32, B, M, N, K in sweep.GPU_CASES)


def test_dispatch_replay_matches_golden():
    import torch
    if torch.cuda.is_available():
        cus = torch.cuda.get_device_properties(torch.cuda.current_device()).multi_processor_count
        if cus != sweep.CUS:
            pytest.skip(f"the recording assumes {sweep.CUS} CUs, this device has {cus}")
    L, n = sweep.load()
    want = golden_lines()
    got = sweep.sweep(L, n, [sweep.inputs_of(l) for l in want])      # (asserts that no dry run answers BD_E_LAUNCH: the device is never reached)
    assert len(got) == len(want)
    bad = [(g, w) for g, w in zip(got, want) if g != w]
    assert not bad, f"{len(bad)} of {len(want)} cases decide differently; first: got '{bad[0][0]}', recorded '{bad[0][1]}'"
