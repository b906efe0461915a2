#!/usr/bin/env python3
"""Which tile kernel serves which prefill-size Linear / delta GEMM, and with what launch: a sweep of the library's real entry points in DRY-RUN
mode (bd_set_gemm_dry_run: the call is planned, recorded and answered, the device is never touched), written to tests/golden/tile_dispatch.txt.

Every tile form computes the same result, so a wrong decision of csrc/bd_api.hip's tile_plan() is only slower -- and one decision is silent by
design: with a workspace that is too small the rule takes the unsplit variant.  This file is the record; tests/test_tile_dispatch.py replays it
against the built library line by line, so a change to the dispatch has to regenerate the file on purpose:

    python tests/golden/make_tile_dispatch_golden.py            # needs the built library; no GPU (256 CUs are assumed without one)

One line per case:
    <entry> <dtype h|b> <fp32 output 0|1> <B> <M> <N> <K> <workspace W|w|s|0> <forced variant> <flags> | <return code> [<record>]
entry: lin / res / rn / sw = bd_binary_linear / _residual / _residual_norm / _swiglu, bmm / bmma / bmms = bd_delta_bmm plain / accumulating onto
C with a scale / scaled without accumulate (the library zeroes C first); a trailing `u` hands in an activation pointer that is not 16-byte aligned.
workspace: W = 256 MiB, w = exactly bd_gemm_workspace_bytes(B, M, N, K), s = one byte less, 0 = none.
flags: bit 0 = bd_set_tail_split(0); flags >> 1 = bd_set_tile_group_m.
record (accepted calls only) = bd_last_gemm_plan without its return code: variant, k slices, tail-split column, workspace bytes needed (low, high),
post-norm on the reduce launch, then the main / tail / reduce launch (14 values each, `-` = not issued).
The pointers handed in are placeholders -- non-null, never dereferenced on the host.
"""
import ctypes
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
OUT = os.path.join(HERE, "tile_dispatch.txt")
CUS = 256                    # num_cus() without a device, and the MI355X's count
BD_F16, BD_BF16, BD_F32 = 0, 1, 2
X, W, P, ALPHA, Y, NORM, H, WS = (0x100000 * i for i in range(1, 9))      # placeholders
WS_BIG = 256 << 20

ENTRIES = ("lin", "res", "rn", "sw", "bmm", "bmma", "bmms")
# every variant an entry point reaches in the shipped library, and the automatic arms as (entry, variant or "tail" / "norm" / "fallback")
SHIPPED = (0, 1, 2, 3, 5, 8, 9, 10, 11, 12, 13, 14, 15, 16, 17, 18, 19, 20, 21, 100)
AUTO_ARMS = ([("sw", 15), ("sw", 21), ("rn", "norm"), ("rn", "fallback"), ("lin", "tail"), ("res", "tail")] +
             [("lin", v) for v in (100, 17, 18, 19, 10, 11, 12, 8, 9, 14, 20)] + [("res", v) for v in (17, 18, 19, 11, 12, 8, 9, 14, 20)] +
             [("bmm", v) for v in (100, 0, 5, 13, 1, 2, 3)])


# one case per automatic arm at the smallest shape that still takes it, run on the device by tests/test_gpu_tile_plan.py (workspace mode w):
# pairs with an even and an odd entry count (19), a k-tile count the slice count does not divide (17), too little k to split (18); a 17- and a
# 65-row call (10 on 64- and 128-row tiles); 64-row tiles narrow and wide (11 / 12); one tile row with a second, mostly empty round (20; 9 with fp32
# output) and 520 tile columns = two full rounds + 8 (14 with the tail split at column 512; 8); the residual and post-norm forms; SwiGLU (15 / 21);
# delta only: each side of the 80 % fill line (0 / 13), 256x128 tiles (5), the small-M tiles (1 / 2 / 3), the zero-fill in front; the generic kernel
GPU_CASES = ([("lin", 1, 0, *s) for s in ((2, 64, 1024, 1024), (3, 64, 1024, 1024), (3, 64, 512, 1088), (3, 64, 1024, 512), (1, 17, 1024, 1024),
                                          (1, 65, 1024, 1024), (1, 48, 16384, 1024), (1, 48, 32768, 1024), (1, 256, 38400, 256), (1, 256, 66560, 256),
                                          (1, 300, 1024, 96))] +
             [("lin", 0, 1, 1, 256, 4096, 256), ("lin", 0, 1, 1, 256, 38400, 256), ("lin", 0, 1, 1, 256, 66560, 256), ("res", 1, 0, 3, 64, 1024, 1024), ("res", 0, 0, 1, 256, 66560, 256),
              ("rn", 1, 0, 3, 64, 1024, 1024), ("rn", 0, 0, 1, 65, 1024, 1024), ("sw", 1, 0, 1, 256, 1024, 256), ("sw", 0, 0, 3, 64, 1024, 256)] +
             [("bmm", 0, 0, *s) for s in ((1, 1024, 4096, 1024), (1, 1024, 13056, 1024), (1, 1024, 13312, 1024), (1, 100, 1024, 1024),
                                          (1, 48, 1024, 1024), (1, 20, 1024, 1024), (1, 100, 1024, 96))] + [("bmms", 1, 1, 1, 100, 1024, 1024)])


def call(L, entry, dtype, f32, B, M, N, K, ws_mode, bufs=None):
    """bufs (the device test): real addresses x, w, p, alpha, y, norm, h, ws and the output's strides sYb, sYm, sHb, sHm"""
    i64, vp = ctypes.c_int64, ctypes.c_void_p
    unaligned = entry.endswith("u")
    entry = entry.rstrip("u")
    if bufs:
        return call_at(L, entry, dtype, f32, B, M, N, K, ws_mode, **bufs)
    x = vp(X + (2 if unaligned else 0))
    n_out = N // 2 if entry == "sw" else N
    return call_at(L, entry, dtype, f32, B, M, N, K, ws_mode, x.value, W, P, ALPHA, Y, NORM, H, WS, M * n_out, n_out, M * N, N)


def call_at(L, entry, dtype, f32, B, M, N, K, ws_mode, x, w, p, alpha, y, norm, h, ws, sYb, sYm, sHb, sHm):
    i64, vp = ctypes.c_int64, ctypes.c_void_p
    X, W, P, ALPHA, Y, NORM, H, WS = x, w, p, alpha, y, norm, h, ws
    x = vp(X)
    out = BD_F32 if f32 else dtype
    wsb = {"W": WS_BIG, "0": 0}.get(ws_mode)
    if wsb is None:
        wsb = L.bd_gemm_workspace_bytes(B, M, N, K) - (1 if ws_mode == "s" else 0)
    ws = vp(WS) if wsb > 0 else None
    wsb = max(wsb, 0)
    sPb = (K // 32) * N if B > 1 else 0
    xs = (B, M, N, K, i64(M * K), i64(K))
    if entry in ("lin", "res"):
        fn = L.bd_binary_linear if entry == "lin" else L.bd_binary_linear_residual
        return fn(x, vp(W), vp(P), vp(ALPHA), vp(Y), *xs, i64(K), i64(sPb), i64(1), 1, i64(sYb), i64(sYm), dtype, out, ws, i64(wsb), None)
    if entry == "rn":
        return L.bd_binary_linear_residual_norm(x, vp(W), vp(P), vp(ALPHA), vp(Y), *xs, i64(K), i64(sPb), i64(1), 1, i64(sYb), i64(sYm), dtype,
                                                vp(NORM), i64(N), ctypes.c_float(1e-5), vp(H), i64(sHb), i64(sHm), ws, i64(wsb), None)
    if entry == "sw":
        return L.bd_binary_linear_swiglu(x, vp(W), vp(P), vp(ALPHA), vp(Y), *xs, i64(K), i64(sPb), i64(2), i64(sYb), i64(sYm), dtype, None)
    alpha, acc = (None, 0) if entry == "bmm" else (vp(ALPHA), 1 if entry == "bmma" else 0)
    return L.bd_delta_bmm(x, vp(P), vp(Y), *xs, i64(sPb), i64(sYb), i64(sYm), dtype, out, 0, alpha, i64(1), 1, acc, ws, i64(wsb), None)


def cases():
    """(entry, dtype, f32, B, M, N, K, workspace, forced, flags).  The shapes: Llama / Mistral projections at the row counts where the rule
    changes arm (17, 64, 65, 128, 129, 512, 513 rows; 1 - 6 entries), the smallest shapes that still take each arm (tests/test_gpu_tile_plan.py),
    and the multi-round gate|up launches whose last round is mostly empty."""
    out = []
    h, b = BD_F16, BD_BF16
    fused = [(6, 64, 4096, 4096), (6, 64, 4096, 4160), (6, 64, 6144, 4096), (6, 64, 28672, 4096), (6, 64, 4096, 14336), (2, 64, 1024, 1024),
             (3, 64, 1024, 1024), (3, 64, 512, 1088), (3, 17, 1024, 1024), (5, 16, 4096, 4096), (2, 33, 4096, 4096), (5, 64, 4100, 4096),
             (1, 100, 4096, 4096), (1, 17, 1024, 1024), (1, 65, 1024, 1024), (1, 64, 28672, 4096), (1, 64, 32768, 4096), (1, 48, 16384, 1024),
             (1, 48, 32768, 1024), (1, 512, 4096, 4096), (1, 513, 4096, 4096), (1, 2048, 4096, 4096), (1, 768, 4096, 4096), (1, 128, 11008, 4096),
             (1, 2048, 22016, 4096), (1, 256, 38400, 256), (1, 256, 66560, 256), (1, 2048, 28672, 4096), (4, 512, 4096, 4096), (2, 2048, 22016, 4096),
             (1, 300, 4096, 96), (1, 300, 4100, 4096), (1, 8192, 4096, 4096), (7, 40, 14336, 4096), (1, 1024, 11008, 4096), (8, 128, 4096, 4096)]
    delta = [(1, 2048, 4096, 4096), (1, 4096, 4096, 4096), (1, 2560, 4096, 4096), (1, 100, 4096, 4096), (1, 48, 4096, 4096), (1, 20, 4096, 4096),
             (1, 1024, 4096, 1024), (1, 1280, 4096, 1024), (1, 300, 4096, 96), (4, 512, 4096, 4096), (6, 64, 4096, 4096), (1, 129, 1024, 1024),
             (1, 8192, 11008, 4096), (3, 300, 4100, 1024)]
    for s in fused:
        for e in ("lin", "res"):
            out += [(e, h, 0, *s, "W", -1, 0), (e, b, 1, *s, "W", -1, 0)]
        out += [("lin", b, 0, *s, "w", -1, 0), ("lin", h, 0, *s, "0", -1, 0), ("res", h, 0, *s, "s", -1, 0), ("rn", h, 0, *s, "w", -1, 0),
                ("rn", b, 0, *s, "0", -1, 0), ("sw", h, 0, *s, "0", -1, 0), ("linu", h, 0, *s, "W", -1, 0)]
    for s in delta:
        out += [("bmm", h, 0, *s, "0", -1, 0), ("bmm", b, 1, *s, "0", -1, 0), ("bmma", b, 0, *s, "0", -1, 0), ("bmms", h, 1, *s, "0", -1, 0),
                ("bmmu", h, 0, *s, "0", -1, 0)]
    # forced variants: every tile id (A/B-only ones and one past the table included) on each kind of call, with and without the workspace
    for v in list(range(0, 23)) + [100]:
        for s in ((1, 2048, 4096, 4096), (6, 64, 4096, 4096), (1, 100, 4096, 1024)):
            out += [("lin", h, 0, *s, "W", v, 0), ("lin", b, 1, *s, "w", v, 0), ("res", b, 0, *s, "W", v, 0), ("sw", h, 0, *s, "0", v, 0),
                    ("bmm", b, 0, *s, "0", v, 0), ("bmma", h, 1, *s, "0", v, 0)]
        out += [("rn", h, 0, 6, 64, 4096, 4096, "w", v, 0), ("lin", h, 0, 6, 64, 4096, 4096, "0", v, 0), ("res", h, 0, 6, 64, 4096, 4096, "s", v, 0), ("lin", h, 0, 6, 64, 4096, 4160, "W", v, 0), ("lin", h, 0, 6, 64, 4096, 64, "W", v, 0),
                ("linu", h, 0, 1, 100, 4096, 1024, "W", v, 0), ("lin", b, 0, 1, 100, 4096, 1024, "s", v, 0), ("lin", b, 0, 1, 100, 4096, 1024, "0", v, 0),
                ("lin", h, 0, 3, 64, 4100, 1024, "W", v, 0)]
    # the hooks that change a planned launch, and calls that leave the tile path or are refused before it
    for s in ((1, 2048, 22016, 4096), (1, 256, 66560, 256)):
        out += [("lin", h, 0, *s, "W", -1, 1), ("lin", h, 0, *s, "W", -1, 2 << 1), ("lin", h, 0, *s, "W", -1, 64 << 1), ("lin", h, 0, *s, "W", 14, 0)]
    out += [("bmm", h, 0, 1, 2048, 4096, 4096, "0", -1, 1 << 1), ("bmm", h, 0, 1, 2048, 4096, 4096, "0", -1, 3 << 1)]
    out += [("lin", h, 0, 1, 16, 4096, 4096, "W", -1, 0), ("bmm", h, 0, 4, 16, 4096, 4096, "W", -1, 0), ("lin", h, 0, 1, 300, 4096, 4100, "W", -1, 0),
            ("sw", h, 0, 1, 16, 4096, 4096, "0", -1, 0), ("sw", h, 0, 1, 300, 4104, 4096, "0", -1, 0), ("lin", h, 0, 1, 300, 4096, 0, "W", -1, 0),
            ("lin", h, 0, 70000, 17, 64, 64, "W", -1, 0), ("res", h, 0, 1, 300, 4096, 96, "W", -1, 0), ("lin", h, 0, 1, 300, 4096, 4096, "W", 200, 0),
            ("bmm", h, 0, 1, 300, 4096, 4096, "0", 800, 0), ("lin", h, 0, 1, 300, 4096, 4096, "W", 700, 0), ("rn", h, 0, 1, 300, 8200, 4096, "W", -1, 0)]
    out += [(e, dt, f32, B, M, N, K, "w", -1, 0) for e, dt, f32, B, M, N, K in GPU_CASES]
    return list(dict.fromkeys(out))


def inputs_of(line):
    """the case a line of the file records"""
    e, dt, f32, B, M, N, K, ws, forced, flags = line.split("|")[0].split()
    return e, "hb".index(dt), int(f32), int(B), int(M), int(N), int(K), ws, int(forced), int(flags)


def load():
    sys.path.insert(0, ROOT)
    from bitdelta_amd import _lib
    return _lib.lib(), _lib.BD_GEMM_PLAN_INTS


def fmt_record(rec):
    """bd_last_gemm_plan's values after the return code, a launch that is not issued as `-`"""
    parts = [" ".join(str(v) for v in rec[1:7])]
    for l in range(3):
        v = rec[7 + 14 * l: 21 + 14 * l]
        parts.append("-" if v[0] < 0 else " ".join(str(x) for x in v))
    return " | ".join(parts)


def sweep(L, n_ints, cs):
    """One line per case, from library L."""
    rec = (ctypes.c_int32 * n_ints)()
    lines = []
    L.bd_set_gemm_dry_run(1)
    try:
        for e, dtype, f32, B, M, N, K, ws, forced, flags in cs:
            L.bd_set_gemm_variant(forced)
            L.bd_set_tail_split(0 if flags & 1 else 1)
            L.bd_set_tile_group_m(flags >> 1)
            rc = call(L, e, dtype, f32, B, M, N, K, ws)
            line = f"{e} {'hb'[dtype]} {f32} {B} {M} {N} {K} {ws} {forced} {flags} | {rc}"
            assert rc != -7, f"{line}: a dry run reached the device (BD_E_LAUNCH)"
            if rc == 0 and B and M and N:
                L.bd_last_gemm_plan(rec, n_ints)
                assert rec[0] == 0 and rec[1] == L.bd_last_gemm_variant(), line
                line += " " + fmt_record(list(rec))
            lines.append(line)
    finally:
        L.bd_set_gemm_dry_run(0)
        L.bd_set_gemm_variant(-1)
        L.bd_set_tail_split(1)
        L.bd_set_tile_group_m(0)
    return lines


def coverage(lines):
    """(shipped variants no accepted case reaches, automatic arms no case reaches, share of refusals, inputs seen per column)"""
    variants, arms, refused = set(), set(), 0
    seen = {"dtype": set(), "f32": set(), "ws": set()}
    for l in lines:
        e, dt, f32, B, M, N, K, ws, forced, flags = inputs_of(l)
        res = l.split("|")[1].split()
        if res[0] != "0":
            refused += 1
            continue
        if len(res) == 1:
            continue
        v, tail, pn = int(res[1]), int(res[3]), int(res[6])
        variants.add(v)
        seen["dtype"].add(dt); seen["f32"].add(f32); seen["ws"].add(ws)
        if forced < 0 and flags == 0 and not e.endswith("u") or v == 100:
            e = e.rstrip("u")
            arms.add((e, v))
            if tail >= 0:
                arms.add((e, "tail"))
            if e == "rn":
                arms.add((e, "norm" if pn else "fallback"))
    return [v for v in SHIPPED if v not in variants], [a for a in AUTO_ARMS if a not in arms], refused / len(lines), seen


if __name__ == "__main__":
    L, n = load()
    lines = sweep(L, n, cases())
    with open(OUT, "w") as fh:
        fh.write("\n".join(lines) + "\n")
    missing, arms, refusals, seen = coverage(lines)
    print(f"{len(lines)} cases, {refusals:.1%} refusals, {os.path.getsize(OUT)} bytes; variants not reached: {missing}; arms not reached: {arms}")
