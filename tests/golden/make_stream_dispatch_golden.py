#!/usr/bin/env python3
"""Which gemv_stream_kernel serves which decode Linear: a sweep of the library's real entry points in DRY-RUN mode (bd_set_decode_dry_run:
the launch is decided, recorded and answered, the device is never touched), written to tests/golden/stream_dispatch.txt.

Every form of the decode Linear produces the same bits by design, so no output test can see a launch that takes the wrong prefetch depth, cache
policy, grid or LDS layout -- it is only slower.  This file is the record of the decision; tests/test_stream_dispatch.py replays the cases it
holds against the built library and demands equality line by line, so a change to the dispatch has to regenerate the file on purpose:

    python tests/golden/make_stream_dispatch_golden.py            # needs the built library; no GPU (256 CUs are assumed without one)

One line per case:  <kind> <dtype> <tenants> <K> <N> <bd_set_stream_tuning flags> <forced variant> | <return code> [<bd_last_decode_plan record>]
(the record only where the call was accepted).  The pointers handed in are placeholders -- 16-byte aligned, non-null, never dereferenced on the
host -- and only calls that end in the streaming kernel or in a refusal before any launch are issued (checked below: an accepted call must
report variant 600).
"""
import ctypes
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
OUT = os.path.join(HERE, "stream_dispatch.txt")
FORMS = os.path.join(HERE, "stream_kernel_forms.txt")
CUS = 256                    # num_cus() without a device, and the MI355X's count

FLAGS = (0, 16, 32, 64, 128, 256, 512, 1024, 128 | 512, 64 | 256, 16 | 128 | 1024, 32 | 64 | 512)      # tests/test_gpu_decode_forms.py
TENANTS = (1, 2, 3, 4, 5, 6, 7, 8, 9, 12, 16)
KS = (1024, 1152, 2048, 4096, 4224, 8192, 14336)
NS = (512, 4096, 4112, 6144, 8192, 8208, 14336, 28672)       # 16-column tiles around one and two per CU at 256 CUs
FORCED = (-1, 601, 616)
BD_F16, BD_BF16 = 0, 1
X, W, P, ALPHA, Y, NORM, SSQ_IN, SSQ_OUT, XW, WSCALE, Q4P = (0x100000 * i for i in range(1, 12))      # placeholders


def t_pad_of(t):
    return next(p for p in (1, 2, 4, 6, 8, 12, 16) if p >= t)


# kind -> (entry point, options).  tiled: tile-major base weight; norm / swiglu: fused prologue / epilogue; ssq: hand-off role
KINDS = {
    "d1": ("decode", dict(layout=1)),
    "d2": ("decode", dict(layout=2)),
    "d2t": ("decode", dict(layout=2, tiled=True)),
    "fn": ("fused", dict(norm=True)), "fs": ("fused", dict(swiglu=True)), "fb": ("fused", dict(norm=True, swiglu=True)),
    "fnt": ("fused", dict(tiled=True, norm=True)), "fst": ("fused", dict(tiled=True, swiglu=True)),
    "fbt": ("fused", dict(tiled=True, norm=True, swiglu=True)),
    "hc": ("handoff", dict(tiled=True, ssq="in")), "hcs": ("handoff", dict(tiled=True, ssq="in", swiglu=True)),
    "hp": ("handoff", dict(tiled=True, ssq="out")), "hpx": ("handoff", dict(tiled=True, ssq="outx")),
    "hpr": ("handoff", dict(ssq="out")),
    "w8": ("w8", {}), "w8n": ("w8", dict(norm=True)), "w8s": ("w8", dict(swiglu=True)), "w8b": ("w8", dict(norm=True, swiglu=True)),
    "w8c": ("w8", dict(ssq="in")), "w8cs": ("w8", dict(ssq="in", swiglu=True)), "w8p": ("w8", dict(ssq="outx")),
    "q4": ("q4", {}), "q4n": ("q4", dict(norm=True)), "q4s": ("q4", dict(swiglu=True)), "q4b": ("q4", dict(norm=True, swiglu=True)),
    "q4c": ("q4", dict(ssq="in", group=1024)), "q4cs": ("q4", dict(ssq="in", swiglu=True)), "q4p": ("q4", dict(ssq="outx")),
    "lin": ("linear", {}),                      # bd_binary_linear, reference-layout masks: one mask per tenant, M = 1
    "linm": ("linear", dict(shared=True)),      # ... one shared mask, M = tenants rows
    "bmm": ("bmm", {}),                         # bd_delta_bmm (delta only): only under a forced streaming variant
    "bmmm": ("bmm", dict(shared=True)),
    "tl": ("tenant", {}),
}
PRODUCERS = ("hp", "hpx", "hpr", "w8p", "q4p")
FLAGGED = [k for k, (e, o) in KINDS.items() if e not in ("linear", "bmm", "tenant") and o.get("layout") != 1]     # packed layout: the flags act


def issued(kind, t, forced):
    """False for the calls that would leave the streaming kernel (and launch something else): reference-layout masks run it for at most 8
    masks and only as a fused Linear, unless a streaming variant is forced (then the library refuses what does not fit)."""
    entry, o = KINDS[kind]
    if entry == "bmm":
        return forced >= 600
    if entry == "linear":
        return forced >= 600 or o.get("shared") or t <= 8
    return True


def call(L, kind, dtype, t, K, N):
    entry, o = KINDS[kind]
    i64, vp = ctypes.c_int64, ctypes.c_void_p
    swiglu, norm, ssq = o.get("swiglu", False), o.get("norm", False), o.get("ssq")
    G = 2 if swiglu else 1
    n_out = N // 2 if swiglu else N
    tp = t_pad_of(t)
    norm_w = NORM if (norm or ssq == "outx") else None
    ssq_in = SSQ_IN if ssq == "in" else None
    ssq_out = SSQ_OUT if ssq in ("out", "outx") else None
    xw = XW if ssq == "outx" else None
    acc = 1 if ssq_out else 0
    common = (t, 1, N, K, i64(K), i64(K))                                     # B, M, N, K, sXb, sXm
    tail = (i64(G), G, i64(n_out), i64(n_out), dtype, dtype, acc)             # sAlb, G, sYb, sYm, dtype, out_dtype, accumulate
    fuse = (vp(norm_w), i64(K if ssq != "outx" else N), ctypes.c_float(1e-5), 1 if swiglu else 0)
    hand = (vp(ssq_in), vp(ssq_out), vp(xw))
    if entry in ("decode", "fused", "handoff"):
        layout = o.get("layout", 2)
        ldw = 0 if o.get("tiled") else K
        sPb = (K // 32) * ((N + 15) // 16 * 16) if layout == 1 else 1
        head = (vp(X), vp(W), vp(P)) + ((layout,) if entry == "decode" else ()) + (tp, vp(ALPHA), vp(Y))
        args = head + common + (i64(ldw), i64(sPb)) + tail
        if entry == "decode":
            return L.bd_binary_linear_decode(*args, None)
        if entry == "fused":
            return L.bd_binary_linear_decode_fused(*args, *fuse, None)
        return L.bd_binary_linear_decode_handoff(*args, *fuse, *hand, None)
    if entry == "w8":
        return L.bd_binary_linear_decode_w8(vp(X), vp(W), vp(WSCALE), vp(P), tp, vp(ALPHA), vp(Y), *common, i64(1), *tail, *fuse, *hand, None)
    if entry == "q4":
        return L.bd_binary_linear_decode_q4(vp(X), vp(W), vp(Q4P), o.get("group", 128), vp(P), tp, vp(ALPHA), vp(Y), *common, i64(1), *tail,
                                            *fuse, *hand, None)
    B, M = (1, t) if o.get("shared") else (t, 1)
    sPb = 0 if o.get("shared") else (K // 32) * N
    if entry == "linear":
        return L.bd_binary_linear(vp(X), vp(W), vp(P), vp(ALPHA), vp(Y), B, M, N, K, i64(M * K), i64(K), i64(K), i64(sPb), i64(1), 1,
                                  i64(M * N), i64(N), dtype, dtype, None, i64(0), None)
    if entry == "bmm":
        return L.bd_delta_bmm(vp(X), vp(P), vp(Y), B, M, N, K, i64(M * K), i64(K), i64(sPb), i64(M * N), i64(N), dtype, dtype, 0, None, i64(0), 1,
                              0, None, i64(0), None)
    return L.bd_tenant_linear(vp(X), vp(W), vp(Y), t, 1, N, K, i64(K), i64(K), i64(N * K), i64(K), i64(N), i64(N), dtype, dtype, None)


def pool():
    """The candidate calls (kind, dtype, tenants, K, N, flags, forced): every axis in full against the others' representative values, and
    both dtypes on every form.  About nine thousand -- too many lines to keep, so select() keeps a part of them."""
    out = []
    for kind in KINDS:
        for t in TENANTS:
            out += [(kind, BD_F16, t, K, 6144, 0, -1) for K in KS]                                  # every K x tenants
            out += [(kind, BD_BF16, t, K, 6144, 0, -1) for K in (1152, 4096, 14336)]
        for t in (1, 2, 4, 6, 8):
            out += [(kind, BD_F16, t, 4096, N, 0, -1) for N in NS if N != 6144]                     # every N
        out += [(kind, BD_BF16, t, 4096, 4096, 0, -1) for t in (2, 4)]                              # (one block per CU where N = 6144 is fine grid)
        for forced in FORCED[1:]:
            for t in (1, 6, 12):
                out += [(kind, BD_BF16, t, K, N, 0, forced) for K, N in ((4096, 4096), (2048, 8208))]
    for kind in PRODUCERS:                                                                          # ssq_out rounds cpb to whole tiles: N around the steps
        for t in range(1, 9):
            out += [(kind, BD_F16, t, 4096, N, 0, -1) for N in (8208, 14336, 28672)] + [(kind, BD_F16, t, 4096, 512, 0, 601)]
    for dt in (BD_F16, BD_BF16):
        out += [(kind, dt, t, 4096, 4096, 0, 616) for kind in ("bmm", "bmmm") for t in TENANTS]     # the delta-only forms
        out += [("tl", dt, 6, 4096, 6144, flags, -1) for flags in (2048, 4096)]                     # bd_tenant_linear's weight-load A/B (bits 11 / 12)
    for kind in FLAGGED:
        for t in TENANTS:                                                                           # nt policy off: the AUX = 0 twins
            out += [(kind, dt, t, K, 6144, 32, -1) for K in (1152, 4096, 14336) for dt in (BD_F16, BD_BF16)]
        for flags in FLAGS[1:]:                                                                     # every flag set
            for t in (1, 6):
                out += [(kind, BD_F16, t, K, N, flags, -1) for K, N in ((4096, 6144), (4096, 4096), (2048, 512), (1152, 8208))]
    return [c for c in dict.fromkeys(out) if issued(c[0], c[2], c[6])]


def core(c):
    """The part of the pool that is always kept: each axis in full on the launch kinds of a decode step (where the rules have their edges), the
    hand-off producers wherever their own rule (whole tiles per block) changes cpb and grid, and the shared-mask / delta-only entry points."""
    kind, dtype, t, K, N, flags, forced = c
    if kind in PRODUCERS and dtype == BD_F16 and flags == 0 and t <= 8 and K == 4096 and (N != 6144 or t in (1, 6)):
        return True                                                                                  # every N, tenants 1 - 8 where ssq_out acts
    if kind in ("bmm", "bmmm"):
        return dtype == BD_F16
    if forced >= 0:
        return kind in ("d2t", "hc", "hp", "w8", "q4", "lin", "linm", "tl")
    if flags:
        return kind in ("d2t", "fnt", "fst", "hc", "hp", "w8", "q4") and dtype == BD_F16 and (flags != 32 or K == 4096) and \
            (K, N) in ((4096, 6144), (2048, 512))                                                    # every flag set, tenants 1 and 6 (and all, nt off)
    if dtype != BD_F16:
        return False
    if N != 6144:
        return kind in ("d1", "d2t", "fst", "hc", "linm", "tl") and t in (1, 6)                      # every N
    if K != 4096:
        return kind in ("d1", "d2", "d2t", "fnt", "hc", "w8", "q4", "lin", "linm") and t in (1, 6)   # every K
    return kind in ("d1", "d2t", "fnt", "fst", "hc", "hp", "w8", "q4", "lin", "linm", "tl")          # every tenant count


def select(lines):
    """core(), then the first line of the pool that reaches each shipped form still missing, and the first refusal of each kind x tenant count x code"""
    cs = pool()
    keep = {i for i, c in enumerate(cs) if core(c)}
    accepted = lambda l: l.split("|")[1].split()[0] == "0"
    reached = {form_of(lines[i]) for i in keep if accepted(lines[i])}
    refusals = {(cs[i][0], cs[i][2], lines[i].split("|")[1]) for i in keep if not accepted(lines[i])}
    for i, l in enumerate(lines):
        if accepted(l) and form_of(l) not in reached:
            reached.add(form_of(l))
            keep.add(i)
        elif not accepted(l) and (cs[i][0], cs[i][2], l.split("|")[1]) not in refusals:
            refusals.add((cs[i][0], cs[i][2], l.split("|")[1]))
            keep.add(i)
    return [lines[i] for i in sorted(keep)]


def inputs_of(line):
    """the case a line of the file records"""
    kind, dt, t, K, N, flags, forced = line.split("|")[0].split()
    return kind, "hb".index(dt), int(t), int(K), int(N), int(flags), int(forced)


def load():
    sys.path.insert(0, ROOT)
    from bitdelta_amd import _lib
    return _lib.lib(), _lib.BD_DECODE_PLAN_INTS


def sweep(L, n_ints, cases):
    """One line per case, from library L."""
    rec = (ctypes.c_int32 * n_ints)()
    lines = []
    L.bd_set_decode_dry_run(1)
    try:
        for kind, dtype, t, K, N, flags, forced in cases:
            assert issued(kind, t, forced), (kind, t, forced)
            L.bd_set_stream_tuning(flags)
            L.bd_set_gemm_variant(forced)
            rc = call(L, kind, dtype, t, K, N)
            line = f"{kind} {'hb'[dtype]} {t} {K} {N} {flags} {forced} | {rc}"
            if rc == 0:
                assert KINDS[kind][0] == "tenant" or L.bd_last_gemm_variant() == 600, f"{line}: left the streaming kernel"
                L.bd_last_decode_plan(rec, n_ints)
                assert rec[0] == 0, line
                line += " " + " ".join(str(v) for v in rec[1:])
            lines.append(line)
    finally:
        L.bd_set_decode_dry_run(0)
        L.bd_set_stream_tuning(0)
        L.bd_set_gemm_variant(-1)
    return lines


def form_of(line):
    """the stream_kernel_forms.txt spelling of an accepted line's instantiation"""
    f = line.split("|")[1].split()[1:13]
    f[2] = "true" if f[2] == "1" else "false"
    return "gemv_stream_kernel<" + ", ".join(f) + ">(bd::StreamParams)"


def coverage(lines):
    """(forms no case reaches, share of refusals)"""
    reached = {form_of(l) for l in lines if l.split("|")[1].split()[0] == "0"}
    shipped = [l.strip() for l in open(FORMS) if l.strip()]
    refused = sum(1 for l in lines if l.split("|")[1].split()[0] != "0")
    return [s for s in shipped if s not in reached], refused / len(lines)


if __name__ == "__main__":
    L, n = load()
    lines = select(sweep(L, n, pool()))
    with open(OUT, "w") as fh:
        fh.write("\n".join(lines) + "\n")
    missing, refusals = coverage(lines)
    print(f"{len(lines)} cases, {refusals:.1%} refusals, {os.path.getsize(OUT)} bytes, {len(missing)} shipped forms not reached")
    for m in missing:
        print("  not reached:", m)
